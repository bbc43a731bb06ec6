// FNO layer tail in one kernel at any channel count (the wide companion of fno_c2r_pw.hip, which keeps
// every shape with Cin, Cout <= 32):
//
//   y[b,o,h,w] = act( sum_{k<m} s_k Re(Y[b,o,h,k] e^{2 pi i k w/W}) + sum_i Wc[o,i] x[b,i,h,w] + bias[o] )
//
// PW = false is the spectral-only form (fno_c2r: no x, no 1x1 convolution, no activation).
// The tail is one GEMM per 64-pixel tile with the spectral term as extra K slabs; the full-resolution
// spectral output never reaches HBM.
//
// GEMM orientation, as fno_pointwise_mfma.hip: C[m = pixel][n = out channel].  A wave holds 64 pixels x
// 64 output channels of fp32 accumulators (a lane: 4 consecutive pixels of one channel per tile);
// output channels go in groups of 64, K in slabs of 32.
//   spectral slabs (KS = ceil(m / 16), 16 complex modes = 32 K rows each):
//          A = G[k'][px], the s_k cos / -s_k sin block of one 64-pixel chunk (fno_c2r_tables, chunk 64:
//              the C2R_F32 table; bf16 I/O reads its hi plane only), identical for every chunk and
//              staged once per workgroup;
//          B = the (b, h) row of Y for the channel group, 4 modes per lane and tile read from global
//              memory (16-byte loads when m is even), rotated by the chunk's phase e^{2 pi i k w0/W}
//              (rot table, LDS) and rounded (bf16 I/O) or split hi/lo (fp32 I/O) in registers.
//              Channels >= Cout and modes >= m are loaded as zeros.
//   conv slabs (ceil(Cin / 32)), as fno_pointwise_mfma.hip:
//          A = x[i][px] through a per-wave channel-planar LDS slab [32][64] (bf16: ds_read_b64_tr_b16;
//              fp32: scalar reads, split hi/lo); rows >= Cin and pixels >= W are WRITTEN as zeros
//              (0 * stale NaN is NaN);
//          B = Wc^T fragments, rounded (bf16) or split (fp32).  WL = true: the whole matrix is staged
//              once per workgroup in LDS in fragment order; WL = false (it does not fit beside the
//              tables in half a CU's LDS): every wave builds its fragments from global memory per slab.
//   fp32 I/O: hi*hi + hi*lo + lo*hi on both halves (bf16x3); GELU the A&S erf form of csrc/nn/gelu.h.
//   bf16 I/O: bf16 operands, fp32 accumulation, gelu_erf_fit.
// Scheduling: the (b, h, chunk) units are split into equal contiguous ranges, one per wave (persistent
// grid, no barrier after the setup); a unit never straddles two (b, h) rows.  Per unit the wave runs the
// channel groups in turn; groups after the first re-read the x slabs (L2).  Tiles past Cout issue no
// MFMAs, columns o >= Cout and pixels >= W are never stored.  The next spectral slab's rows and (bf16) the next
// step's x slab are loaded into registers before the current slab's MFMAs.  No atomics: bit-reproducible.
//
// LDS per workgroup (dynamic): G KS x 4 (bf16) / 8 (fp32) KB + rot 128 KS ceil(W / 64) B (<= 16 KB) +
//   x slabs 4 x 5120 (bf16, pitch 80) / 4 x 8704 (fp32, pitch 68) + W fragments ceil(Cin / 32) x
//   ceil(Cout / 16) x 1 (bf16) / 2 (fp32) KB when WL.  64 -> 64 at 720 x 1440, m = 32: bf16 42 KB, fp32
//   73 KB.  WL needs the total <= 80 KB (two workgroups per CU); without W it is at most 82 KB.
// Registers (scripts/kernel_resources.py, gfx950; VGPRs, no AGPRs, no scratch in any instance; bounded to 256 by
// amdgpu_waves_per_eu(2, 2)): bf16 184 (spectral-only) / 244 (W in LDS) / 256 (W from global memory); fp32 157 /
// 234 / 247 -> 2 waves per SIMD = 2 workgroups per CU wherever the LDS total is <= 80 KB.  fp32 holds no operand
// a step ahead (PREF below): with the x and spectrum prefetch registers it spilled 52 - 92 bytes.
// Measured against c2r + fno_pointwise at 720 x 1440: profiles/fno_tail_wide_r8.txt (bench/bench_fno_tail_wide.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>

#include "../nn/bf16_pack.h"
#include "../nn/gelu.h"
#include "../ops/tuning.h"
#include "dft_gemm.h"

namespace amd_dft {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s lds_v4s;

constexpr int kCH = kFnoWideChunk;  // pixels per unit
constexpr int kPT = kCH / 16;       // MFMA pixel tiles per unit
constexpr int kGT = 4;              // output tiles per group
constexpr int kSlab = 32;           // input channels per conv slab

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <bool BF, bool GELU>
__device__ __forceinline__ void act2(float& a, float& b) {
  if constexpr (GELU) {
    const gelu_f2 r = BF ? gelu_erf_fit2(gelu_f2{a, b}) : gelu_erf2(gelu_f2{a, b});
    a = r.x;
    b = r.y;
  }
}

// the B fragment of Wc^T for output channel o and input channels i0 .. i0 + 7 (zeros outside the matrix)
template <bool BF>
__device__ __forceinline__ void load_wfrag(const float* __restrict__ wc, int o, int i0, int Cin, int Cout, bf16x8& hi,
                                           bf16x8& lo) {
  float v[8];
  const bool ok = o < Cout;
  const float* row = wc + static_cast<int64_t>(min(o, Cout - 1)) * Cin;
  if ((Cin & 3) == 0 && i0 + 7 < Cin) {  // rows start 16-byte aligned
    const f32x4 a = *reinterpret_cast<const f32x4*>(row + i0), b = *reinterpret_cast<const f32x4*>(row + i0 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = ok ? a[j] : 0.f;
      v[4 + j] = ok ? b[j] : 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (ok && i0 + j < Cin) ? row[i0 + j] : 0.f;
  }
  uint32_t h[4], l[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if constexpr (BF) {
      h[j] = pk_bf16(v[2 * j], v[2 * j + 1]);
      l[j] = 0u;
    } else {
      split_pk(v[2 * j], v[2 * j + 1], h[j], l[j]);
    }
  }
  hi = __builtin_bit_cast(bf16x8, make_uint4(h[0], h[1], h[2], h[3]));
  lo = __builtin_bit_cast(bf16x8, make_uint4(l[0], l[1], l[2], l[3]));
}

template <bool BF, bool GELU, bool PW, bool WL>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
fno_c2r_pw_wide_kernel(const float2* __restrict__ yw, const void* __restrict__ x, const float* __restrict__ wc,
                       const float* __restrict__ bias, void* __restrict__ y, const bf16x8* __restrict__ g0,
                       const float2* __restrict__ rot, int Cin, int Cout, int H, int W, int m, int KS, int nch,
                       int64_t units) {
  static_assert(PW || (!GELU && !WL), "the spectral-only tail has no activation and no weights");
  constexpr int ES = BF ? 2 : 4;
  constexpr int XP = BF ? kCH + 16 : kCH + 4;  // LDS row pitch (elements) of the x slab
  constexpr int NP = BF ? 1 : 2;               // operand planes: hi (, lo)
  constexpr int NQ = kSlab / 4;                // channel rows per lane and slab (4 rows per wave instruction)
  constexpr int NR = BF ? 2 : 4;               // 32-bit words of 4 pixels
  constexpr int XB = PW ? kSlab * XP * ES : 0; // bytes of one wave's x slab
  // bf16: the next x slab and the next spectral slab's rows are held in registers one step ahead; fp32: with those
  // 64 registers beside the 64 accumulators and the split operands the kernel spilled, so it loads them in place
  constexpr bool PREF = BF;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int nslab = PW ? (Cin + kSlab - 1) / kSlab : 0;
  const int otiles = (Cout + 15) / 16;
  const int ngroup = (otiles + kGT - 1) / kGT;
  const int nrot = nch * 16 * KS;
  const int ng = KS * kPT * NP * 64;  // G fragments

  bf16x8* gs = reinterpret_cast<bf16x8*>(smem);                  // [ks][pt][plane][lane]
  float2* rots = reinterpret_cast<float2*>(smem + ng * 16);       // [chunk][16 KS]
  char* xs = smem + ng * 16 + nrot * 8 + wv * XB;                 // this wave's x slab
  bf16x8* wsm = reinterpret_cast<bf16x8*>(smem + ng * 16 + nrot * 8 + 4 * XB);  // [slab][otile][plane][lane]
  lds_v4s* xs_tr = (lds_v4s*)(xs);

  // ---- tables (and, WL, the weight fragments) into LDS, once per workgroup
  for (int t = threadIdx.x; t < ng; t += 256) {
    const int ln = t & 63, r = t >> 6;
    const int hl = r % NP, f = r / NP;  // f = ks * kPT + pt
    gs[t] = g0[(f * 2 + hl) * 64 + ln];
  }
  for (int t = threadIdx.x; t < nrot; t += 256) rots[t] = rot[t];
  if constexpr (WL) {
    for (int f = wv; f < nslab * otiles; f += 4) {
      const int s = f / otiles, t = f - s * otiles;
      bf16x8 hi, lo;
      load_wfrag<BF>(wc, 16 * t + l15, kSlab * s + 8 * lq, Cin, Cout, hi, lo);
      wsm[(f * NP) * 64 + lane] = hi;
      if constexpr (!BF) wsm[(f * NP + 1) * 64 + lane] = lo;
    }
  }
  __syncthreads();

  const int64_t nw = static_cast<int64_t>(gridDim.x) * 4;
  const int64_t gw = static_cast<int64_t>(blockIdx.x) * 4 + wv;
  const int64_t u0 = gw * units / nw, u1 = (gw + 1) * units / nw;
  if (u0 >= u1) return;  // no barriers below this point

  // unit u = (b * H + h) * nch + c, kept as counters advanced once per unit
  int c, h, b;
  {
    const int64_t row = u0 / nch;
    c = static_cast<int>(u0 - row * nch);
    b = static_cast<int>(row / H);
    h = static_cast<int>(row - static_cast<int64_t>(b) * H);
  }

  // x staging: the lane holds 4 pixels st_px.. of channel rows st_ch + 4 q of a slab
  const int st_ch = lane >> 4, st_px = (lane & 15) * 4;
  uint32_t xr[PW ? NQ : 1][NR];
  auto load_x = [&](int bb, int hh, int cc, int s) {
    if constexpr (PW) {
      const int gpx = cc * kCH + st_px;  // W % 4 == 0: the 4 pixels are all inside or all outside
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int ch = s * kSlab + st_ch + 4 * q;
#pragma unroll
        for (int t = 0; t < NR; ++t) xr[q][t] = 0u;
        if (ch < Cin && gpx < W) {
          const char* src =
              static_cast<const char*>(x) + (((static_cast<int64_t>(bb) * Cin + ch) * H + hh) * W + gpx) * ES;
          if constexpr (BF) {
            const uint2 v = *reinterpret_cast<const uint2*>(src);
            xr[q][0] = v.x;
            xr[q][1] = v.y;
          } else {
            const u32x4 v = *reinterpret_cast<const u32x4*>(src);
#pragma unroll
            for (int t = 0; t < 4; ++t) xr[q][t] = v[t];
          }
        }
      }
    }
  };
  // spectrum fragments of slab ks: the lane's modes 16 ks + 4 lq + 0..3 of channels o0 + 16 ot + l15
  float2 Yv[kGT][4];
  auto load_y = [&](int o0, int nt, int ks) {
    const int k0 = 16 * ks + 4 * lq;
    const bool vec = (m & 1) == 0 && k0 + 3 < m;
#pragma unroll
    for (int ot = 0; ot < kGT; ++ot) {
      const int o = o0 + 16 * ot + l15;
#pragma unroll
      for (int q = 0; q < 4; ++q) Yv[ot][q] = make_float2(0.f, 0.f);
      if (ot < nt && o < Cout) {
        const float2* src = yw + ((static_cast<int64_t>(b) * Cout + o) * H + h) * m + k0;
        if (vec) {
          const f32x4 v0 = reinterpret_cast<const f32x4*>(src)[0], v1 = reinterpret_cast<const f32x4*>(src)[1];
          Yv[ot][0] = make_float2(v0[0], v0[1]);
          Yv[ot][1] = make_float2(v0[2], v0[3]);
          Yv[ot][2] = make_float2(v1[0], v1[1]);
          Yv[ot][3] = make_float2(v1[2], v1[3]);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (k0 + q < m) Yv[ot][q] = src[q];
        }
      }
    }
  };

  if constexpr (PREF) load_x(b, h, c, 0);
  char* const yb = static_cast<char*>(y);
  for (int64_t u = u0; u < u1; ++u) {
    int cn = c + 1, hn = h, bn = b;  // the next unit
    if (cn == nch) {
      cn = 0;
      if (++hn == H) {
        hn = 0;
        ++bn;
      }
    }
    const int w0 = c * kCH;
    for (int g = 0; g < ngroup; ++g) {
      const int o0 = g * 16 * kGT;
      const int nt = min(kGT, otiles - g * kGT);  // live output tiles (wave-uniform)
      f32x4 acc[kPT][kGT];
#pragma unroll
      for (int ot = 0; ot < kGT; ++ot) {
        const int o = o0 + 16 * ot + l15;
        const float bo = (bias != nullptr && o < Cout) ? bias[o] : 0.f;
#pragma unroll
        for (int pt = 0; pt < kPT; ++pt) acc[pt][ot] = f32x4{bo, bo, bo, bo};
      }
      // ---- spectral slabs
      if constexpr (PREF) load_y(o0, nt, 0);
      for (int ks = 0; ks < KS; ++ks) {
        if constexpr (!PREF) load_y(o0, nt, ks);
        bf16x8 Bh[kGT], Bl[BF ? 1 : kGT];
        {
          uint32_t hi[kGT][4], lo[kGT][4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float2 r = rots[c * 16 * KS + 16 * ks + 4 * lq + q];
#pragma unroll
            for (int ot = 0; ot < kGT; ++ot) {
              const float2 v = Yv[ot][q];
              const float re = v.x * r.x - v.y * r.y, im = v.x * r.y + v.y * r.x;
              if constexpr (BF) hi[ot][q] = pk_bf16(re, im);
              else split_pk(re, im, hi[ot][q], lo[ot][q]);
            }
          }
#pragma unroll
          for (int ot = 0; ot < kGT; ++ot) {
            Bh[ot] = __builtin_bit_cast(bf16x8, make_uint4(hi[ot][0], hi[ot][1], hi[ot][2], hi[ot][3]));
            if constexpr (!BF) Bl[ot] = __builtin_bit_cast(bf16x8, make_uint4(lo[ot][0], lo[ot][1], lo[ot][2], lo[ot][3]));
          }
        }
        if constexpr (PREF)
          if (ks + 1 < KS) load_y(o0, nt, ks + 1);  // in flight during this slab's MFMAs
#pragma unroll
        for (int pt = 0; pt < kPT; ++pt) {
          const bf16x8 gh = gs[((ks * kPT + pt) * NP) * 64 + lane];
          bf16x8 gl;
          if constexpr (!BF) gl = gs[((ks * kPT + pt) * NP + 1) * 64 + lane];
#pragma unroll
          for (int ot = 0; ot < kGT; ++ot) {
            if (ot < nt) {
              acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gh, Bh[ot], acc[pt][ot], 0, 0, 0);
              if constexpr (!BF) {
                acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gh, Bl[ot], acc[pt][ot], 0, 0, 0);
                acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gl, Bh[ot], acc[pt][ot], 0, 0, 0);
              }
            }
          }
        }
      }
      // ---- conv slabs
      for (int s = 0; s < nslab; ++s) {
        if constexpr (!PREF) load_x(b, h, c, s);
        wave_lds_fence();  // this wave is done reading the previous slab
#pragma unroll
        for (int q = 0; q < (PW ? NQ : 0); ++q) {
          char* dst = xs + ((st_ch + 4 * q) * XP + st_px) * ES;
          if constexpr (BF) *reinterpret_cast<uint2*>(dst) = make_uint2(xr[q][0], xr[q][1]);
          else *reinterpret_cast<u32x4*>(dst) = u32x4{xr[q][0], xr[q][1], xr[q][2], xr[q][3]};
        }
        bf16x8 Wh[kGT], Wl[kGT];
#pragma unroll
        for (int ot = 0; ot < kGT; ++ot) {
          if (ot < nt) {
            if constexpr (WL) {
              const int f = s * otiles + g * kGT + ot;
              Wh[ot] = wsm[(f * NP) * 64 + lane];
              if constexpr (!BF) Wl[ot] = wsm[(f * NP + 1) * 64 + lane];
            } else {
              load_wfrag<BF>(wc, o0 + 16 * ot + l15, kSlab * s + 8 * lq, Cin, Cout, Wh[ot], Wl[ot]);
            }
          }
        }
        wave_lds_fence();
        // the next step's x, in flight during the MFMAs: next slab, next group's first slab, next unit's
        if constexpr (PREF) {
          const bool same = s + 1 < nslab || g + 1 < ngroup;
          if (same || u + 1 < u1) load_x(same ? b : bn, same ? h : hn, same ? c : cn, s + 1 < nslab ? s + 1 : 0);
        }
#pragma unroll
        for (int pt = 0; pt < kPT; ++pt) {
          bf16x8 ax, axl;
          if constexpr (BF) {
            // rows 8lq + (0..3) and 8lq + (4..7), cols 16pt..16pt+15: lane 4q'+p addresses row q', cols 4p..4p+3
            const int e0 = (8 * lq + (l15 >> 2)) * XP + 16 * pt + 4 * (l15 & 3);
            const v4s a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(xs_tr + e0 / 4);
            const v4s a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(xs_tr + (e0 + 4 * XP) / 4);
            const uint2 u0v = __builtin_bit_cast(uint2, a0), u1v = __builtin_bit_cast(uint2, a1);
            ax = __builtin_bit_cast(bf16x8, make_uint4(u0v.x, u0v.y, u1v.x, u1v.y));
          } else {
            uint32_t hi[4], lo[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float* rp = reinterpret_cast<const float*>(xs) + (8 * lq + 2 * j) * XP + 16 * pt + l15;
              split_pk(rp[0], rp[XP], hi[j], lo[j]);
            }
            ax = __builtin_bit_cast(bf16x8, make_uint4(hi[0], hi[1], hi[2], hi[3]));
            axl = __builtin_bit_cast(bf16x8, make_uint4(lo[0], lo[1], lo[2], lo[3]));
          }
#pragma unroll
          for (int ot = 0; ot < kGT; ++ot) {
            if (ot < nt) {
              acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax, Wh[ot], acc[pt][ot], 0, 0, 0);
              if constexpr (!BF) {
                acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax, Wl[ot], acc[pt][ot], 0, 0, 0);
                acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(axl, Wh[ot], acc[pt][ot], 0, 0, 0);
              }
            }
          }
        }
      }
      // ---- activation + store, 4 consecutive pixels of one channel per lane
#pragma unroll
      for (int ot = 0; ot < kGT; ++ot) {
        const int o = o0 + 16 * ot + l15;
        if (ot < nt && o < Cout) {
          char* row = yb + (((static_cast<int64_t>(b) * Cout + o) * H + h) * W) * ES;
#pragma unroll
          for (int pt = 0; pt < kPT; ++pt) {
            const int px = w0 + 16 * pt + 4 * lq;
            float v[4] = {acc[pt][ot][0], acc[pt][ot][1], acc[pt][ot][2], acc[pt][ot][3]};
            act2<BF, GELU>(v[0], v[1]);
            act2<BF, GELU>(v[2], v[3]);
            if (px < W) {  // W % 4 == 0: all four or none
              char* dst = row + static_cast<int64_t>(px) * ES;
              if constexpr (BF) *reinterpret_cast<uint2*>(dst) = make_uint2(pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]));
              else *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            }
          }
        }
      }
    }
    c = cn;
    h = hn;
    b = bn;
  }
}

struct WideGeo {
  int KS, nch, nslab, otiles;
  size_t lds_base, lds_w;  // bytes without / of the LDS-resident weight fragments
};

WideGeo wide_geo(int cin, int cout, int m, int W, bool bf16) {
  WideGeo g;
  g.KS = (m + 15) / 16;
  g.nch = (W + kCH - 1) / kCH;
  g.nslab = (cin + kSlab - 1) / kSlab;
  g.otiles = (cout + 15) / 16;
  const size_t np = bf16 ? 1 : 2;
  const size_t xslab = cin > 0 ? static_cast<size_t>(kSlab) * (bf16 ? (kCH + 16) * 2 : (kCH + 4) * 4) : 0;
  g.lds_base = static_cast<size_t>(g.KS) * kPT * np * 1024 + static_cast<size_t>(g.nch) * 16 * g.KS * 8 + 4 * xslab;
  g.lds_w = static_cast<size_t>(g.nslab) * g.otiles * np * 1024;
  return g;
}

constexpr size_t kWideLdsHalfCu = 80 * 1024;  // two workgroups per CU

int64_t device_cus() {
  static int64_t cache[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (cache[dev] == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    cache[dev] = cus;
  }
  return cache[dev];
}

// workgroups of one instance resident per CU at a dynamic LDS size (cached; the first call also lifts the
// instance's dynamic LDS limit to the CU's 160 KB)
int64_t resident_per_cu(const void* kern, size_t lds) {
  static std::mutex mu;
  static std::map<std::tuple<const void*, size_t, int>, int64_t> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  std::lock_guard<std::mutex> lk(mu);
  const auto key = std::make_tuple(kern, lds, dev);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
    (void)hipGetLastError();
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds) != hipSuccess || per_cu <= 0) {
    (void)hipGetLastError();
    per_cu = 1;
  }
  return cache[key] = per_cu;
}

template <bool BF, bool GELU, bool PW, bool WL>
void launch_i(const FnoC2RPwLaunch& p, const WideGeo& g, hipStream_t st) {
  const auto kern = &fno_c2r_pw_wide_kernel<BF, GELU, PW, WL>;
  const size_t lds = g.lds_base + (WL ? g.lds_w : 0);
  const int64_t units = static_cast<int64_t>(p.B) * p.H * g.nch;
  // persistent grid, as fno_c2r_pw.hip: one round of resident workgroups, >= 2 units per wave, a whole
  // number of workgroups per CU (tuning builds: MI_DFT_FNO_WIDE_UPW = minimum units per wave)
  static const int upw = [] {
    const char* e = tuning_env("MI_DFT_FNO_WIDE_UPW");
    return e ? std::max(1, std::atoi(e)) : 2;
  }();
  const int64_t cus = device_cus();
  const int64_t res = cus * resident_per_cu(reinterpret_cast<const void*>(kern), lds);
  int64_t nwg = std::max<int64_t>(std::min<int64_t>((units + 4 * upw - 1) / (4 * upw), res), 1);
  if (nwg > cus) nwg = nwg / cus * cus;
  hipLaunchKernelGGL(kern, dim3(static_cast<uint32_t>(nwg)), dim3(256), lds, st, static_cast<const float2*>(p.yw), p.x,
                     p.wc, p.bias, p.y, static_cast<const bf16x8*>(p.g0), static_cast<const float2*>(p.rot), p.Cin,
                     p.Cout, p.H, p.W, p.m, g.KS, g.nch, units);
}

template <bool BF>
void launch_bf(const FnoC2RPwLaunch& p, const WideGeo& g, hipStream_t st) {
  if (p.x == nullptr) return launch_i<BF, false, false, false>(p, g, st);
  const bool wl = fno_c2r_pw_wide_weights_in_lds(p.Cin, p.Cout, p.m, p.W, BF);
  if (p.gelu) {
    if (wl) launch_i<BF, true, true, true>(p, g, st);
    else launch_i<BF, true, true, false>(p, g, st);
  } else {
    if (wl) launch_i<BF, false, true, true>(p, g, st);
    else launch_i<BF, false, true, false>(p, g, st);
  }
}

}  // namespace

bool fno_c2r_pw_wide_supported(int cin, int cout, int m, int W, bool bf16) {
  (void)bf16;  // both dtypes take 64-pixel chunks
  if (!(cin >= 0 && cout >= 1 && m >= 1 && m <= 64 && 2 * (m - 1) <= W && W % 8 == 0)) return false;
  return static_cast<int64_t>((W + kCH - 1) / kCH) * 16 * ((m + 15) / 16) <= kFnoRotMax;
}

bool fno_c2r_pw_wide_weights_in_lds(int cin, int cout, int m, int W, bool bf16) {
  if (cin < 1) return false;
  const WideGeo g = wide_geo(cin, cout, m, W, bf16);
  return g.lds_base + g.lds_w <= kWideLdsHalfCu;
}

void launch_fno_c2r_pw_wide(const FnoC2RPwLaunch& p, void* stream) {
  if (p.B == 0 || p.H == 0) return;
  const int cin = p.x == nullptr ? 0 : p.Cin;
  if (p.x == nullptr && p.gelu) throw std::runtime_error("amd_dft: fno_c2r: the spectral-only tail takes no activation");
  if (p.x != nullptr && p.Cin < 1) throw std::runtime_error("amd_dft: fno_c2r_pw: Cin must be >= 1");
  if (!fno_c2r_pw_wide_supported(cin, p.Cout, p.m, p.W, p.bf16 != 0))
    throw std::runtime_error("amd_dft: fno_c2r_pw (wide): needs m <= 64, 2 (m - 1) <= W, W % 8 == 0 and "
                             "ceil(W / 64) * 16 ceil(m / 16) <= 2048");
  const WideGeo g = wide_geo(cin, p.Cout, p.m, p.W, p.bf16 != 0);
  if (g.lds_base > 160 * 1024) throw std::runtime_error("amd_dft: fno_c2r_pw (wide): tables exceed LDS");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (p.bf16) launch_bf<true>(p, g, st);
  else launch_bf<false>(p, g, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: fno_c2r_pw_wide launch: ") + hipGetErrorString(e));
}

}  // namespace amd_dft

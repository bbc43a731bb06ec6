// FNO pointwise epilogue at any channel count, on MFMA:
//   y[b, o, p] = act( spec[b, o, p] + sum_i w[o, i] * x[b, i, p] + bias[o] )
// (channel-first [B, C, P] tensors, fp32 or bf16 I/O, fp32 accumulation; spec and bias optional;
// act = none or erf-GELU).  fno_pointwise.hip keeps its seven register-resident instances; every
// other Cin runs here (fno_pointwise_route, spectral.h).
//
// GEMM orientation, as the conv half of fno_c2r_pw.hip: C[m = pixel][n = out channel], so a lane's
// accumulator holds 4 consecutive pixels of one channel (8 / 16-byte stores).
//   A = x[i][px] from a per-wave channel-planar LDS slab [32 channels][64 pixels], read transposed
//       (bf16: ds_read_b64_tr_b16, two reads give a lane its 8 channels of one pixel; fp32: 8 scalar
//       reads, split hi/lo in registers);
//   B = W^T[i][o], rounded (bf16 I/O: bf16 operands, the precision of a bf16 nn.Linear) or split hi/lo
//       (fp32 I/O: hi*hi + hi*lo + lo*hi, the bf16x3 fp32-class path) by the whole workgroup into LDS
//       in fragment order -- each element once per workgroup.
// A workgroup (4 waves) owns 256 consecutive pixels of one batch entry, a wave 64 of them.
//   K loop:  runtime loop over ceil(Cin / 32) slabs staged through LDS, no limit on Cin.  Rows i >= Cin
//            of the last slab and pixels >= P are WRITTEN as zeros (the padded weight columns are zero
//            too, but 0 * stale-NaN is NaN); nothing is read or written past P.
//   N loop:  output channels in groups of 4 tiles x 16 = 64 channels (64 pixels x 64 channels of fp32
//            accumulators per wave).  For Cout > 64 every further group RE-READS the x slabs from
//            global memory (L2 for the second and later passes): x traffic is ceil(Cout / 64) times
//            the tensor.  Tiles past Cout issue no MFMAs; columns o >= Cout are never stored.
//   I/O:     VEC = true: rows start 4-element aligned and P % 4 == 0 -- 8 / 16-byte loads and stores;
//            VEC = false (odd P, views at a storage offset): per-element loads and stores.
// The next step's x and W values are loaded into registers before the current step's MFMAs.
// No atomics: results are bit-reproducible run to run.
// GELU: fp32 output the A&S 7.1.26 erf form of csrc/nn/gelu.h (|erf error| <= 1.5e-7), as the fp32
// layer tail; bf16 output gelu_erf_fit (|error| <= 2.6e-5 absolute), as the bf16 tail.
//
// LDS per workgroup: fp32 4 x 8704 (x slabs, pitch 68 floats) + 8192 (W hi/lo) = 43008 B;
//                    bf16 4 x 5120 (pitch 80 bf16) + 4096 (W) = 24576 B.
// Registers (scripts/kernel_resources.py, gfx950; unified VGPR count, 64 of them AGPRs = the accumulators;
// no scratch): fp32 180 (no GELU) - 232, bf16 196 - 200 -> 2 waves per SIMD = 2 workgroups per CU
// (register-bound; LDS alone would allow 3 fp32 / 6 bf16).
//
// LN = true (fno_pointwise_ln): x is replaced by its LayerNorm over the Cin channels of each pixel.  The wave walks
// its slabs once more in front for the per-pixel moments (no barrier), then normalises each slab as it writes it to
// LDS, before the bf16 rounding / the hi-lo split.  The mean is never folded into the epilogue (rstd (W'x - mean W'1)
// cancels where |mean| >> std).  fp32 I/O under LN runs a three-plane bf16 split and six products (X6 below) and an
// erfc-based GELU (act2): with the two-plane split and the A&S GELU a field of W LN(x) measured 2e-5 .. 1e-4 rel-L2
// against fp64, with them 1e-7 .. 1.3e-6.  Registers: bf16 208 - 216 (2 waves per SIMD, LDS as above); fp32 212
// (VEC, no GELU) - 260, LDS 4 x 8704 + 12288 = 47104 B: three of the four fp32 LN instances are over 256 VGPRs and
// run one wave per SIMD.  No scratch.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "../nn/bf16_pack.h"
#include "../nn/gelu.h"
#include "spectral.h"

namespace amd_dft {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s lds_v4s;

constexpr int kPX = 64;           // pixels per wave
constexpr int kPT = kPX / 16;     // MFMA pixel tiles per wave
constexpr int kGT = kPwGroupTiles;  // output tiles per group

// EX: the six-product fp32 LN instances, whose product is good to 1e-7: x Phi(x) = x erfc(-x / sqrt2) / 2 with the
// library erfc (a few ulp RELATIVE).  The A&S form's 1.5e-7 is absolute in erf, and 1 + erf cancels for x < 0: a
// channel that GELU switches mostly off (x ~ -3, Phi ~ 1e-3) would carry 1e-4 of its norm.
template <bool BF, bool GELU, bool EX = false>
__device__ __forceinline__ void act2(float& a, float& b) {
  if constexpr (GELU && EX) {
    a = 0.5f * a * erfcf(-0.70710678118654752f * a);
    b = 0.5f * b * erfcf(-0.70710678118654752f * b);
  } else if constexpr (GELU) {
    const gelu_f2 r = BF ? gelu_erf_fit2(gelu_f2{a, b}) : gelu_erf2(gelu_f2{a, b});
    a = r.x;
    b = r.y;
  }
}

template <bool BF>
__device__ __forceinline__ float ld1(const char* p) {
  if constexpr (BF) return __uint_as_float(static_cast<uint32_t>(*reinterpret_cast<const uint16_t*>(p)) << 16);
  else return *reinterpret_cast<const float*>(p);
}
template <bool BF>
__device__ __forceinline__ void st1(char* p, float v) {
  if constexpr (BF) *reinterpret_cast<uint16_t*>(p) = __builtin_bit_cast(uint16_t, static_cast<__bf16>(v));
  else *reinterpret_cast<float*>(p) = v;
}

// 4 pixels of one channel row as staged (2 or 4 words) -> floats
template <bool BF, int NR>
__device__ __forceinline__ void px4(const uint32_t (&r)[NR], float (&v)[4]) {
  if constexpr (BF) {
    v[0] = __uint_as_float(r[0] << 16), v[1] = __uint_as_float(r[0] & 0xffff0000u);
    v[2] = __uint_as_float(r[1] << 16), v[3] = __uint_as_float(r[1] & 0xffff0000u);
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = __uint_as_float(r[t]);
  }
}

// the third bf16 plane of (a, b) after split_pk's (hi, lo): bf16(a - hi.a - lo.a, b - hi.b - lo.b); both
// subtractions are exact in fp32
__device__ __forceinline__ uint32_t third_pk(float a, float b, uint32_t hi, uint32_t lo) {
  return pk_bf16((a - __uint_as_float(hi << 16)) - __uint_as_float(lo << 16),
                 (b - __uint_as_float(hi & 0xffff0000u)) - __uint_as_float(lo & 0xffff0000u));
}

// Chan's update of (na, mean, m2) by (nb, mb, m2b); either count may be 0
__device__ __forceinline__ void chan_merge(float& na, float& mean, float& m2, float nb, float mb, float m2b) {
  const float nt = na + nb;
  const float fb = nt > 0.f ? nb / nt : 0.f;
  const float delta = mb - mean;
  mean = __builtin_fmaf(delta, fb, mean);
  m2 = __builtin_fmaf(delta * delta, na * fb, m2 + m2b);
  na = nt;
}

template <bool BF, bool VEC, bool GELU, bool LN>
__global__ void __launch_bounds__(256) fno_pointwise_mfma_kernel(const void* __restrict__ spec, const void* __restrict__ x,
                                                                  const float* __restrict__ w,
                                                                  const float* __restrict__ bias, void* __restrict__ y,
                                                                  int Cin, int Cout, int P,
                                                                  const float* __restrict__ ln_w,
                                                                  const float* __restrict__ ln_b, float ln_eps) {
  constexpr int ES = BF ? 2 : 4;
  constexpr int XP = BF ? kPX + 16 : kPX + 4;  // LDS row pitch (elements) of the x slab
  // fp32 I/O under LN: operands split in three bf16 planes (a = p0 + p1 + p2, residual 2^-25 |a|) and six products,
  // p0 p0 + p0 p1 + p1 p0 + p1 p1 + p0 p2 + p2 p0 (what is left out is below 2^-25 of a term): the two-plane split
  // leaves up to 2^-17 of each operand behind, which a field of LN(x) whose terms cancel shows as 2e-5 .. 1e-4
  constexpr bool X6 = LN && !BF;
  constexpr int NH = BF ? 1 : X6 ? 3 : 2;      // weight planes: hi (, lo (, lo2))
  constexpr int NQ = kPwSlab / 4;              // channel rows per lane and slab (4 rows per wave instruction)
  constexpr int NR = BF ? 2 : 4;               // 32-bit words of 4 pixels
  __shared__ __attribute__((aligned(16))) char xs_raw[4][kPwSlab * XP * ES];
  __shared__ bf16x8 ws[NH][kGT][64];

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int64_t b = blockIdx.y;
  const int px0 = (blockIdx.x * 4 + wv) * kPX;  // this wave's first pixel (may be >= P: the wave only stages W)
  char* xs = xs_raw[wv];
  lds_v4s* xs_tr = (lds_v4s*)(xs_raw[wv]);

  const int nslab = (Cin + kPwSlab - 1) / kPwSlab;
  const int ngroup = (Cout + 16 * kGT - 1) / (16 * kGT);
  const int nstep = nslab * ngroup;

  // staging roles: x -- lane holds 4 pixels st_px.. of channel rows st_ch + 4 q of the slab;
  // W -- thread (wave = tile ot, lane) holds the B fragment W[o0 + 16 ot + l15][k0 + 8 lq + 0..7]
  const int st_ch = lane >> 4, st_px = (lane & 15) * 4;
  const int gpx = px0 + st_px;  // first of this lane's 4 staged pixels
  const char* xb = static_cast<const char*>(x) + (b * Cin * static_cast<int64_t>(P) + gpx) * ES;
  uint32_t xr[NQ][NR];
  float wr[8];

  auto load_x = [&](int s) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int ch = s * kPwSlab + st_ch + 4 * q;
      const char* src = xb + static_cast<int64_t>(ch) * P * ES;
#pragma unroll
      for (int t = 0; t < NR; ++t) xr[q][t] = 0u;
      if (ch < Cin) {
        if constexpr (VEC) {
          if (gpx < P) {  // P % 4 == 0: the 4 pixels are all inside or all outside
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
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (gpx + e < P) {
              if constexpr (BF) {
                const uint32_t v = *reinterpret_cast<const uint16_t*>(src + 2 * e);
                xr[q][e >> 1] |= v << (16 * (e & 1));
              } else {
                xr[q][e] = *reinterpret_cast<const uint32_t*>(src + 4 * e);
              }
            }
          }
        }
      }
    }
  };
  auto load_step = [&](int s, int g) {
    load_x(s);
    const int o = g * 16 * kGT + 16 * wv + l15;
    const int i0 = s * kPwSlab + 8 * lq;
#pragma unroll
    for (int j = 0; j < 8; ++j) wr[j] = (o < Cout && i0 + j < Cin) ? w[static_cast<int64_t>(o) * Cin + i0 + j] : 0.f;
  };

  // LN: the wave walks its slabs once for the moments of its 64 pixels over the Cin channels.  A lane has 4 pixels x
  // 8 channel rows of a slab: d = x - K with K = x[b, 0, pixel] (so |mean| >> std costs nothing), a two-pass
  // (mean, M2) of the slab's rows, Chan's update into the running triple; then the four lane groups (rows st_ch = 0..3)
  // are merged across lanes in group order, every lane of a pixel column ending with the same bits.  No barrier.
  float lnK[4], lnM[4], lnR[4];
  if constexpr (LN) {
    float cnt = 0.f, m2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) lnM[e] = m2[e] = lnK[e] = 0.f;
    for (int s2 = 0; s2 < nslab; ++s2) {
      load_x(s2);
      float d[NQ][4];
#pragma unroll
      for (int q = 0; q < NQ; ++q) px4<BF, NR>(xr[q], d[q]);
      if (s2 == 0) {  // channel 0: row q = 0 of lane group 0
#pragma unroll
        for (int e = 0; e < 4; ++e) lnK[e] = __shfl(d[0][e], l15, 64);
      }
      const int nv = min(max((Cin - s2 * kPwSlab - st_ch + 3) / 4, 0), NQ);  // this lane's rows < Cin: q < nv
      const float fn = static_cast<float>(nv), rn = nv > 0 ? 1.f / fn : 0.f;
      float cnt_e = cnt;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float cm = 0.f, c2 = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          d[q][e] = q < nv ? d[q][e] - lnK[e] : 0.f;
          cm += d[q][e];
        }
        cm *= rn;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const float t = q < nv ? d[q][e] - cm : 0.f;
          c2 = __builtin_fmaf(t, t, c2);
        }
        cnt_e = cnt;
        chan_merge(cnt_e, lnM[e], m2[e], fn, cm, c2);
      }
      cnt = cnt_e;
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float cn = __shfl_xor(cnt, o, 64);
      const bool up = (lane & o) != 0;
      float ca = cnt;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float mo = __shfl_xor(lnM[e], o, 64), qo = __shfl_xor(m2[e], o, 64);
        float na = up ? cn : cnt, ma = up ? mo : lnM[e], qa = up ? qo : m2[e];
        chan_merge(na, ma, qa, up ? cnt : cn, up ? lnM[e] : mo, up ? m2[e] : qo);
        lnM[e] = ma, m2[e] = qa, ca = na;
      }
      cnt = ca;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) lnR[e] = 1.0f / sqrtf(m2[e] / static_cast<float>(Cin) + ln_eps);
  }

  f32x4 acc[kPT][kGT];
  load_step(0, 0);
  int s = 0, g = 0;
  for (int step = 0; step < nstep; ++step) {
    const int o0 = g * 16 * kGT;
    if (s == 0) {
      // accumulators start at bias + spec (lane: channel o0 + 16 ot + l15, pixels px0 + 16 pt + 4 lq + 0..3)
#pragma unroll
      for (int ot = 0; ot < kGT; ++ot) {
        const int o = o0 + 16 * ot + l15;
        const bool ok = o < Cout;
        const float bo = (ok && bias != nullptr) ? bias[o] : 0.f;
#pragma unroll
        for (int pt = 0; pt < kPT; ++pt) {
          acc[pt][ot] = f32x4{bo, bo, bo, bo};
          const int px = px0 + 16 * pt + 4 * lq;
          if (spec != nullptr && ok) {
            const char* sp = static_cast<const char*>(spec) + ((b * Cout + o) * static_cast<int64_t>(P) + px) * ES;
            if constexpr (VEC) {
              if (px < P) {
                if constexpr (BF) {
                  const uint2 v = *reinterpret_cast<const uint2*>(sp);
                  acc[pt][ot][0] += __uint_as_float(v.x << 16);
                  acc[pt][ot][1] += __uint_as_float(v.x & 0xffff0000u);
                  acc[pt][ot][2] += __uint_as_float(v.y << 16);
                  acc[pt][ot][3] += __uint_as_float(v.y & 0xffff0000u);
                } else {
                  const f32x4 v = *reinterpret_cast<const f32x4*>(sp);
                  acc[pt][ot] += v;
                }
              }
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (px + e < P) acc[pt][ot][e] += ld1<BF>(sp + e * ES);
            }
          }
        }
      }
    }
    // LN: per-channel scale and shift of this step's rows (0 for rows >= Cin), fetched across the barrier rather than
    // a step ahead with x and W: 16 registers less where the next step's operands are live
    float gr[LN ? NQ : 1], br[LN ? NQ : 1];
    if constexpr (LN) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int ch = s * kPwSlab + st_ch + 4 * q;
        gr[q] = ch < Cin ? (ln_w != nullptr ? ln_w[ch] : 1.f) : 0.f;
        br[q] = (ch < Cin && ln_b != nullptr) ? ln_b[ch] : 0.f;
      }
    }
    __syncthreads();  // every wave is done reading the previous step's slab and weights
    // ---- this step's x slab (channels x pixels, zeros where i >= Cin or p >= P) and W fragments into LDS
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      char* dst = xs + ((st_ch + 4 * q) * XP + st_px) * ES;
      if constexpr (LN) {  // normalised before the bf16 rounding (bf16) / the hi-lo split at the read (fp32)
        const bool rowok = s * kPwSlab + st_ch + 4 * q < Cin;
        float v[4];
        px4<BF, NR>(xr[q], v);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = __builtin_fmaf(((v[e] - lnK[e]) - lnM[e]) * lnR[e], gr[q], br[q]);
          if (!(rowok && gpx + e < P)) v[e] = 0.f;
        }
        if constexpr (BF) *reinterpret_cast<uint2*>(dst) = make_uint2(pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]));
        else *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
      } else if constexpr (BF) *reinterpret_cast<uint2*>(dst) = make_uint2(xr[q][0], xr[q][1]);
      else *reinterpret_cast<u32x4*>(dst) = u32x4{xr[q][0], xr[q][1], xr[q][2], xr[q][3]};
    }
    {
      uint32_t hi[4], lo[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) split_pk(wr[2 * j], wr[2 * j + 1], hi[j], lo[j]);
      ws[0][wv][lane] = __builtin_bit_cast(bf16x8, make_uint4(hi[0], hi[1], hi[2], hi[3]));
      if constexpr (!BF) ws[1][wv][lane] = __builtin_bit_cast(bf16x8, make_uint4(lo[0], lo[1], lo[2], lo[3]));
      if constexpr (X6) {
        uint32_t l2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) l2[j] = third_pk(wr[2 * j], wr[2 * j + 1], hi[j], lo[j]);
        ws[2][wv][lane] = __builtin_bit_cast(bf16x8, make_uint4(l2[0], l2[1], l2[2], l2[3]));
      }
    }
    __syncthreads();
    // ---- the next step's global loads, in flight during the MFMAs
    int sn = s + 1, gn = g;
    if (sn == nslab) {
      sn = 0;
      ++gn;
    }
    if (step + 1 < nstep) load_step(sn, gn);
    // ---- MFMAs: live output tiles only (wave-uniform)
    bf16x8 Wh[kGT], Wl[kGT], W2[kGT];
#pragma unroll
    for (int ot = 0; ot < kGT; ++ot) {
      Wh[ot] = ws[0][ot][lane];
      if constexpr (!BF) Wl[ot] = ws[1][ot][lane];
      if constexpr (X6) W2[ot] = ws[2][ot][lane];
    }
#pragma unroll
    for (int pt = 0; pt < kPT; ++pt) {
      bf16x8 ax, axl, ax2;
      if constexpr (BF) {
        // rows 8lq + (0..3) and 8lq + (4..7), cols 16pt..16pt+15: lane 4q'+p addresses row q', cols 4p..4p+3
        const int e0 = (8 * lq + (l15 >> 2)) * XP + 16 * pt + 4 * (l15 & 3);
        const v4s a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(xs_tr + e0 / 4);
        const v4s a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(xs_tr + (e0 + 4 * XP) / 4);
        const uint2 u0v = __builtin_bit_cast(uint2, a0), u1v = __builtin_bit_cast(uint2, a1);
        ax = __builtin_bit_cast(bf16x8, make_uint4(u0v.x, u0v.y, u1v.x, u1v.y));
      } else {
        uint32_t hi[4], lo[4], l2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float* rp = reinterpret_cast<const float*>(xs) + (8 * lq + 2 * j) * XP + 16 * pt + l15;
          split_pk(rp[0], rp[XP], hi[j], lo[j]);
          if constexpr (X6) l2[j] = third_pk(rp[0], rp[XP], hi[j], lo[j]);
        }
        ax = __builtin_bit_cast(bf16x8, make_uint4(hi[0], hi[1], hi[2], hi[3]));
        axl = __builtin_bit_cast(bf16x8, make_uint4(lo[0], lo[1], lo[2], lo[3]));
        if constexpr (X6) ax2 = __builtin_bit_cast(bf16x8, make_uint4(l2[0], l2[1], l2[2], l2[3]));
      }
#pragma unroll
      for (int ot = 0; ot < kGT; ++ot) {
        if (o0 + 16 * ot < Cout) {
          acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax, Wh[ot], acc[pt][ot], 0, 0, 0);
          if constexpr (!BF) {
            acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax, Wl[ot], acc[pt][ot], 0, 0, 0);
            acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(axl, Wh[ot], acc[pt][ot], 0, 0, 0);
          }
          if constexpr (X6) {
            acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(axl, Wl[ot], acc[pt][ot], 0, 0, 0);
            acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax, W2[ot], acc[pt][ot], 0, 0, 0);
            acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax2, Wh[ot], acc[pt][ot], 0, 0, 0);
          }
        }
      }
    }
    // ---- last slab of the group: activation + store, 4 consecutive pixels of one channel per lane
    if (s == nslab - 1) {
#pragma unroll
      for (int ot = 0; ot < kGT; ++ot) {
        const int o = o0 + 16 * ot + l15;
        if (o < Cout) {
#pragma unroll
          for (int pt = 0; pt < kPT; ++pt) {
            const int px = px0 + 16 * pt + 4 * lq;
            float v[4] = {acc[pt][ot][0], acc[pt][ot][1], acc[pt][ot][2], acc[pt][ot][3]};
            act2<BF, GELU, X6>(v[0], v[1]);
            act2<BF, GELU, X6>(v[2], v[3]);
            char* dst = static_cast<char*>(y) + ((b * Cout + o) * static_cast<int64_t>(P) + px) * ES;
            if constexpr (VEC) {
              if (px < P) {
                if constexpr (BF) *reinterpret_cast<uint2*>(dst) = make_uint2(pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]));
                else *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
              }
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (px + e < P) st1<BF>(dst + e * ES, v[e]);
            }
          }
        }
      }
    }
    s = sn;
    g = gn;
  }
}

template <bool BF, bool VEC>
void launch_act(const FnoPointwiseLaunch& p, hipStream_t st) {
  const dim3 grid((p.P + 4 * kPX - 1) / (4 * kPX), p.B);
#define L_(G, LN)                                                                                               \
  hipLaunchKernelGGL((fno_pointwise_mfma_kernel<BF, VEC, G, LN>), grid, dim3(256), 0, st, p.spec, p.x, p.w, p.bias, \
                     p.y, p.Cin, p.Cout, p.P, p.ln_w, p.ln_b, p.ln_eps)
  if (p.ln) {
    if (p.gelu) L_(true, true);
    else L_(false, true);
  } else if (p.gelu) L_(true, false);
  else L_(false, false);
#undef L_
}

}  // namespace

void launch_fno_pointwise_mfma(const FnoPointwiseLaunch& p, bool vec, void* stream) {
  if (p.B == 0 || p.P == 0 || p.Cout == 0) return;
  if (p.B > 65535) throw std::runtime_error("amd_dft: fno_pointwise: batch > 65535");
  if (p.Cin < 1) throw std::runtime_error("amd_dft: fno_pointwise: Cin must be >= 1");
  if (vec && p.P % 4 != 0) throw std::runtime_error("amd_dft: fno_pointwise: vector I/O needs P % 4 == 0");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (p.bf16) {
    if (vec) launch_act<true, true>(p, st);
    else launch_act<true, false>(p, st);
  } else {
    if (vec) launch_act<false, true>(p, st);
    else launch_act<false, false>(p, st);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: fno_pointwise_mfma launch: ") + hipGetErrorString(e));
}

}  // namespace amd_dft

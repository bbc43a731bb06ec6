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

template <bool BF, bool GELU>
__device__ __forceinline__ void act2(float& a, float& b) {
  if constexpr (GELU) {
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

template <bool BF, bool VEC, bool GELU>
__global__ void __launch_bounds__(256) fno_pointwise_mfma_kernel(const void* __restrict__ spec, const void* __restrict__ x,
                                                                  const float* __restrict__ w,
                                                                  const float* __restrict__ bias, void* __restrict__ y,
                                                                  int Cin, int Cout, int P) {
  constexpr int ES = BF ? 2 : 4;
  constexpr int XP = BF ? kPX + 16 : kPX + 4;  // LDS row pitch (elements) of the x slab
  constexpr int NH = BF ? 1 : 2;               // weight planes: hi (, lo)
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

  auto load_step = [&](int s, int g) {
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
    const int o = g * 16 * kGT + 16 * wv + l15;
    const int i0 = s * kPwSlab + 8 * lq;
#pragma unroll
    for (int j = 0; j < 8; ++j) wr[j] = (o < Cout && i0 + j < Cin) ? w[static_cast<int64_t>(o) * Cin + i0 + j] : 0.f;
  };

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
    __syncthreads();  // every wave is done reading the previous step's slab and weights
    // ---- this step's x slab (channels x pixels, zeros where i >= Cin or p >= P) and W fragments into LDS
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      char* dst = xs + ((st_ch + 4 * q) * XP + st_px) * ES;
      if constexpr (BF) *reinterpret_cast<uint2*>(dst) = make_uint2(xr[q][0], xr[q][1]);
      else *reinterpret_cast<u32x4*>(dst) = u32x4{xr[q][0], xr[q][1], xr[q][2], xr[q][3]};
    }
    {
      uint32_t hi[4], lo[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) split_pk(wr[2 * j], wr[2 * j + 1], hi[j], lo[j]);
      ws[0][wv][lane] = __builtin_bit_cast(bf16x8, make_uint4(hi[0], hi[1], hi[2], hi[3]));
      if constexpr (!BF) ws[NH - 1][wv][lane] = __builtin_bit_cast(bf16x8, make_uint4(lo[0], lo[1], lo[2], lo[3]));
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
    bf16x8 Wh[kGT], Wl[kGT];
#pragma unroll
    for (int ot = 0; ot < kGT; ++ot) {
      Wh[ot] = ws[0][ot][lane];
      if constexpr (!BF) Wl[ot] = ws[NH - 1][ot][lane];
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
        if (o0 + 16 * ot < Cout) {
          acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax, Wh[ot], acc[pt][ot], 0, 0, 0);
          if constexpr (!BF) {
            acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax, Wl[ot], acc[pt][ot], 0, 0, 0);
            acc[pt][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(axl, Wh[ot], acc[pt][ot], 0, 0, 0);
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
            act2<BF, GELU>(v[0], v[1]);
            act2<BF, GELU>(v[2], v[3]);
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
#define L_(G)                                                                                                  \
  hipLaunchKernelGGL((fno_pointwise_mfma_kernel<BF, VEC, G>), grid, dim3(256), 0, st, p.spec, p.x, p.w, p.bias, p.y, \
                     p.Cin, p.Cout, p.P)
  if (p.gelu) L_(true);
  else L_(false);
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

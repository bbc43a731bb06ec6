// AFNO block-diagonal complex MLP on an already-transformed spectrum, at any H and mode window:
//   for every token t (a kept mode of the 2-D spectrum) and channel block k, with z = [re(BS) | im(BS)]
//   gathered from the (c, re/im)-interleaved row x[t, k BS .. (k + 1) BS, 0..1]:
//     h = ReLU(z . W1' + b1'),   o = softshrink(h . W2' + b2', lambda),   o stored back interleaved
//   W' = [[W0, W1], [-W1, W0]] is the real 2BS x 2BS form of the complex block weight, in the packed layouts
//   of pack_afno_weights: [NB][n][k] bf16, or split (fp32-class path) k32-interleaved hi|lo pairs [NB][n][2k].
// afno_spectral.hip fuses this MLP with the H transforms for its 12 (H, block size) instances; every other
// shape transforms with the FFT kernels and runs the MLP here.  The block size is a runtime loop bound
// (16 <= BS <= 256, BS % 16 == 0: afno_mlp_route, spectral.h), so there is no instance list.
//
// One workgroup (4 waves) owns TOK = 16 MT token rows of one channel block (TOK from BS on the host):
//   load     the fp32 rows are read once (16-byte loads: two channels' re, im), de-interleaved and rounded to
//            bf16 (plain weights: the precision of the fused bf16 filter) or split hi + lo (split weights)
//            into the LDS operand tile A [TOK][2BS + 8].  Rows past T are WRITTEN as zeros (0 x stale NaN
//            is NaN); nothing is read or written past row T.
//   GEMM 1   [TOK x 2BS] = A . W1'^T on v_mfma_f32_16x16x32_bf16, fp32 accumulation (split: hi.hi + lo.hi +
//            hi.lo); a wave takes two 16-column tiles x MT row tiles per pass over K, the passes cover the
//            2BS columns.  The operands are swapped (transposed accumulator: a lane holds 4 consecutive columns
//            of one row), so bias + ReLU write 8-byte pieces of the hidden tile Hd (LDS, re-split on chip).
//   GEMM 2   the same loop on Hd with W2' rows permuted so the columns come out as (re, im) pairs: a lane holds
//            two channels' complex values of one token; bias + softshrink, one 16-byte store to global.
// The hidden activation never leaves LDS: one HBM read and one HBM write of the spectrum.
// Weight (B) fragments are per-lane 16-byte loads from L2, requested one k-step ahead of their MFMAs.
// No atomics: results are bit-reproducible run to run.
//
// LDS per workgroup: 2 tiles (A, Hd) x planes (1, split: 2) x TOK x (2BS + 8) x 2 bytes, <= 80 KB.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "spectral.h"

namespace amd_dft {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kNT = 256;  // threads

struct AfnoMlpArgs {
  const float* x;
  float* y;
  const uint16_t* w1t;
  const uint16_t* w2t;
  const float* b1;
  const float* b2;
  int64_t T;
  int C, NB, BS;
  float lambda;
};

__device__ __forceinline__ uint32_t f2bf16(float f) {
  return static_cast<uint32_t>(__builtin_bit_cast(uint16_t, static_cast<__bf16>(f)));
}
__device__ __forceinline__ float bf_up(uint32_t h) { return __uint_as_float(h << 16); }

// two consecutive values (idx2 in 32-bit words) as bf16, or as bf16 hi / lo pieces
template <bool X3>
__device__ __forceinline__ void put2(uint16_t* Ah, uint16_t* Al, int idx2, float a, float b) {
  const uint32_t ha = f2bf16(a), hb = f2bf16(b);
  reinterpret_cast<uint32_t*>(Ah)[idx2] = ha | (hb << 16);
  if constexpr (X3) reinterpret_cast<uint32_t*>(Al)[idx2] = f2bf16(a - bf_up(ha)) | (f2bf16(b - bf_up(hb)) << 16);
}
// four consecutive values (8-byte aligned idx, in elements)
template <bool X3>
__device__ __forceinline__ void put4(uint16_t* Ah, uint16_t* Al, int idx, float a, float b, float c, float d) {
  const uint32_t ha = f2bf16(a), hb = f2bf16(b), hc = f2bf16(c), hd = f2bf16(d);
  *reinterpret_cast<uint2*>(Ah + idx) = make_uint2(ha | (hb << 16), hc | (hd << 16));
  if constexpr (X3)
    *reinterpret_cast<uint2*>(Al + idx) = make_uint2(f2bf16(a - bf_up(ha)) | (f2bf16(b - bf_up(hb)) << 16),
                                                     f2bf16(c - bf_up(hc)) | (f2bf16(d - bf_up(hd)) << 16));
}

// One GEMM [16 MT x 2BS] = A (LDS, pitch AP) x Bt^T (global [n][k], split: k32-interleaved hi|lo rows) with its
// epilogue.  G2 = false: bias + ReLU -> Oh / Ol (LDS, natural [re | im] columns).  G2 = true: output column n'
// computes weight row (n' & 1) BS + (n' >> 1) (interleaved (re, im) pairs), bias + softshrink -> yout (global,
// rows < nrow only).
template <bool X3, int MT, bool G2>
__device__ __forceinline__ void mlp_gemm(const uint16_t* __restrict__ Ah, const uint16_t* __restrict__ Al,
                                         const uint16_t* __restrict__ Bt, const float* __restrict__ bias, int BS,
                                         uint16_t* __restrict__ Oh, uint16_t* __restrict__ Ol, float* __restrict__ yout,
                                         int64_t row_stride, int nrow, float lam) {
  const int K = 2 * BS, AP = K + 8, KS = K / 32, NCT = K / 16;
  const int KW = X3 ? 2 * K : K;    // weight row length (elements)
  constexpr int KST = X3 ? 64 : 32;  // weight elements per k-step
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  // NCT = BS / 8 is even: a wave's two tiles are both inside or both outside (wave-uniform loop bound)
  for (int ct = 2 * w; ct < NCT; ct += 8) {
    const uint16_t* brow[2];
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
      const int n = (ct + nj) * 16 + r16;
      const int row = G2 ? (n & 1) * BS + (n >> 1) : n;
      brow[nj] = Bt + static_cast<int64_t>(row) * KW + kq * 8;
    }
    f32x4 acc[MT][2];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int nj = 0; nj < 2; ++nj) acc[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 bh[2], bl[2], nh[2], nl[2];
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
      bh[nj] = *reinterpret_cast<const bf16x8*>(brow[nj]);
      if constexpr (X3) bl[nj] = *reinterpret_cast<const bf16x8*>(brow[nj] + 32);
    }
    for (int ks = 0; ks < KS; ++ks) {
      // the next k-step's weight fragments, in flight during this step's MFMAs (the last step re-requests
      // its own: in bounds, and the loop body stays branch-free)
      const int kn = ks + 1 < KS ? ks + 1 : ks;
#pragma unroll
      for (int nj = 0; nj < 2; ++nj) {
        nh[nj] = *reinterpret_cast<const bf16x8*>(brow[nj] + kn * KST);
        if constexpr (X3) nl[nj] = *reinterpret_cast<const bf16x8*>(brow[nj] + kn * KST + 32);
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of its use (afno_spectral.hip gemm_tile_x3)
      bf16x8 ah[MT], al[MT];
#pragma unroll
      for (int mi = 0; mi < MT; ++mi) {
        const int e = (mi * 16 + r16) * AP + ks * 32 + kq * 8;
        ah[mi] = *reinterpret_cast<const bf16x8*>(Ah + e);
        if constexpr (X3) al[mi] = *reinterpret_cast<const bf16x8*>(Al + e);
      }
      // transposed tile (weights as the first MFMA operand): a lane holds columns n0 .. n0 + 3 of row m
#pragma unroll
      for (int pr = 0; pr < (X3 ? 3 : 1); ++pr)
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
          for (int nj = 0; nj < 2; ++nj) {
            const bf16x8 av = (X3 && pr == 0) ? al[mi] : ah[mi];
            const bf16x8 bv = (X3 && pr == 1) ? bl[nj] : bh[nj];
            acc[mi][nj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bv, av, acc[mi][nj], 0, 0, 0);
          }
#pragma unroll
      for (int nj = 0; nj < 2; ++nj) {
        bh[nj] = nh[nj];
        if constexpr (X3) bl[nj] = nl[nj];
      }
    }
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
      const int n0 = (ct + nj) * 16 + 4 * kq;
      if constexpr (!G2) {
        const float4 b = *reinterpret_cast<const float4*>(bias + n0);
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) {
          const int m = mi * 16 + r16;
          put4<X3>(Oh, Ol, m * AP + n0, fmaxf(acc[mi][nj][0] + b.x, 0.f), fmaxf(acc[mi][nj][1] + b.y, 0.f),
                   fmaxf(acc[mi][nj][2] + b.z, 0.f), fmaxf(acc[mi][nj][3] + b.w, 0.f));
        }
      } else {
        const int c0 = n0 >> 1;  // channels c0, c0 + 1 of the block
        const float2 bre = *reinterpret_cast<const float2*>(bias + c0);
        const float2 bim = *reinterpret_cast<const float2*>(bias + BS + c0);
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) {
          const int m = mi * 16 + r16;
          if (m < nrow) {
            const float v0 = acc[mi][nj][0] + bre.x, v1 = acc[mi][nj][1] + bim.x;
            const float v2 = acc[mi][nj][2] + bre.y, v3 = acc[mi][nj][3] + bim.y;
            *reinterpret_cast<float4*>(yout + m * row_stride + 2 * c0) =
                make_float4(v0 - __builtin_amdgcn_fmed3f(v0, -lam, lam), v1 - __builtin_amdgcn_fmed3f(v1, -lam, lam),
                            v2 - __builtin_amdgcn_fmed3f(v2, -lam, lam), v3 - __builtin_amdgcn_fmed3f(v3, -lam, lam));
          }
        }
      }
    }
  }
}

template <bool X3, int MT>
__global__ void __launch_bounds__(kNT) afno_mlp_kernel(const AfnoMlpArgs a) {
  constexpr int TOK = 16 * MT, NPL = X3 ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  const int BS = a.BS, K = 2 * BS, AP = K + 8, NP = BS / 2;
  const int plane = TOK * AP;  // bf16 elements per plane
  uint16_t* Ah = lds;          // [TOK][AP] operand tile, hi
  uint16_t* Al = Ah + (NPL - 1) * plane;
  uint16_t* Hh = lds + NPL * plane;  // hidden tile
  uint16_t* Hl = Hh + (NPL - 1) * plane;
  const int tid = threadIdx.x;
  const int blk = blockIdx.x % a.NB;
  const int64_t t0 = static_cast<int64_t>(blockIdx.x / a.NB) * TOK;  // first token row of this tile (< T)
  const int64_t left = a.T - t0;
  const int nrow = left < TOK ? static_cast<int>(left) : TOK;
  const int64_t row_stride = static_cast<int64_t>(a.C) * 2;  // scalars between consecutive tokens
  const int64_t base = t0 * row_stride + static_cast<int64_t>(blk) * K;
  const float* xin = a.x + base;
  float* yout = a.y + base;
  // ---- load + de-interleave: item = (row r, channel pair tp); rows >= nrow become zeros
  for (int i = tid; i < TOK * NP; i += kNT) {
    const int r = i / NP, tp = i - r * NP;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < nrow) v = *reinterpret_cast<const float4*>(xin + r * row_stride + 4 * tp);
    const int idx2 = (r * AP) / 2 + tp;
    put2<X3>(Ah, Al, idx2, v.x, v.z);
    put2<X3>(Ah, Al, idx2 + NP, v.y, v.w);
  }
  __syncthreads();
  const int64_t wo = static_cast<int64_t>(blk) * K * (X3 ? 2 * K : K);
  mlp_gemm<X3, MT, false>(Ah, Al, a.w1t + wo, a.b1 + blk * K, BS, Hh, Hl, nullptr, 0, nrow, 0.f);
  __syncthreads();
  mlp_gemm<X3, MT, true>(Hh, Hl, a.w2t + wo, a.b2 + blk * K, BS, nullptr, nullptr, yout, row_stride, nrow, a.lambda);
}

using KernFn = void (*)(AfnoMlpArgs);

KernFn pick_kernel(bool x3, int tok) {
  if (x3) return tok == 64 ? afno_mlp_kernel<true, 4> : (tok == 32 ? afno_mlp_kernel<true, 2> : afno_mlp_kernel<true, 1>);
  return tok == 64 ? afno_mlp_kernel<false, 4> : (tok == 32 ? afno_mlp_kernel<false, 2> : afno_mlp_kernel<false, 1>);
}

}  // namespace

void launch_afno_mlp(const AfnoMlpLaunch& p, void* stream) {
  if (p.NB <= 0 || p.C <= 0 || p.C % p.NB) throw std::runtime_error("amd_dft: afno_mlp: C must be a multiple of NB");
  const int bs = p.C / p.NB;
  const AfnoMlpRoute r = afno_mlp_route(bs, p.x3 != 0, p.T);
  if (!r.ok) throw std::runtime_error(std::string("amd_dft: afno_mlp: ") + r.why);
  if (p.T <= 0) return;
  if (reinterpret_cast<uintptr_t>(p.x) % 16 != 0 || reinterpret_cast<uintptr_t>(p.y) % 16 != 0)
    throw std::runtime_error("amd_dft: afno_mlp: x and y must be 16-byte aligned");
  const int64_t nblocks = r.tiles * p.NB;
  if (nblocks >= (int64_t(1) << 31)) throw std::runtime_error("amd_dft: afno_mlp: too many token tiles for one launch");
  AfnoMlpArgs a;
  a.x = p.x;
  a.y = p.y;
  a.w1t = p.w1t;
  a.w2t = p.w2t;
  a.b1 = p.b1;
  a.b2 = p.b2;
  a.T = p.T;
  a.C = p.C;
  a.NB = p.NB;
  a.BS = bs;
  a.lambda = p.lambda;
  KernFn kern = pick_kernel(p.x3 != 0, r.tok);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(r.lds));
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: afno_mlp attr: ") + hipGetErrorString(e));
  hipLaunchKernelGGL(kern, dim3(static_cast<uint32_t>(nblocks)), dim3(kNT), static_cast<size_t>(r.lds),
                     static_cast<hipStream_t>(stream), a);
  e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: afno_mlp launch: ") + hipGetErrorString(e));
}

}  // namespace amd_dft

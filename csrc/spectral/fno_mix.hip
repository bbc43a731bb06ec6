// FNO spectral mode mixing on MFMA (K4 in SURVEY §2.5):
//   y[b, o, m] = sum_i x[b, i, m] * w[i, o, m]        (complex, per retained mode m)
// as a batch of small real-block GEMMs  [Xr | Xi] (B x 2Cin) . [[Wr, Wi], [-Wi, Wr]] (2Cin x 2Cout)
// on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation: the same numerics as an
// fp32 einsum).  A workgroup owns MT consecutive modes: x, w and y tiles are moved between HBM
// and LDS in 8*MT-byte contiguous runs per (b, i) / (i, o) / (b, o), and each wave runs the
// GEMMs of its modes straight out of LDS.
//
// bf16 instances (x, w and y bf16, a (re, im) pair one 4-byte word; fp32 accumulation, one rounding at the store; no
// atomics): the stream kernel below with the pair type as a template parameter, and fno_mix_bf16_kernel, the per-mode
// GEMM on v_mfma_f32_16x16x32_bf16 -- one MFMA per fragment pair.  Which kernel a call takes: fno_mix_route
// (spectral.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "../nn/bf16_pack.h"
#include "spectral.h"

namespace amd_dft {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// one (re, im) pair as the kernels hold it in memory (float2, or a packed bf16 pair) <-> float2
__device__ __forceinline__ float2 pair_load(float2 v) { return v; }
__device__ __forceinline__ float2 pair_load(uint32_t v) {
  return make_float2(__uint_as_float(v << 16), __uint_as_float(v & 0xffff0000u));
}
__device__ __forceinline__ void pair_store(float2* p, float2 v) { *p = v; }
__device__ __forceinline__ void pair_store(uint32_t* p, float2 v) { *p = pk_bf16(v.x, v.y); }

constexpr int kMT = 8;     // modes per workgroup
constexpr int kNT = 256;   // threads (4 waves)

__global__ void __launch_bounds__(kNT) fno_mix_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      float* __restrict__ y, int B, int Cin, int Cout, int M) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int K = 2 * Cin, N = 2 * Cout;
  const int Kp = (K + 3) & ~3;             // k padded to the MFMA k-step
  const int Bp = (B + 15) & ~15, Np = (N + 15) & ~15;
  float* Xs = smem;                        // [kMT][Bp][Kp]
  float* Ws = Xs + kMT * Bp * Kp;          // [kMT][Kp][Np]
  float* Ys = Ws + kMT * Kp * Np;          // [kMT][Bp][Np]
  const int m0 = blockIdx.x * kMT;
  const int tid = threadIdx.x;
  // ---- zero-fill the padded tiles, then load (coalesced along the mode index)
  for (int i = tid; i < kMT * Bp * Kp; i += kNT) Xs[i] = 0.f;
  for (int i = tid; i < kMT * Kp * Np; i += kNT) Ws[i] = 0.f;
  __syncthreads();
  // x[b][i][m][2]: one thread per (b, i, mt, part)
  for (int idx = tid; idx < B * Cin * kMT * 2; idx += kNT) {
    const int part = idx & 1;
    const int mt = (idx >> 1) % kMT;
    const int bi = (idx >> 1) / kMT;
    const int i = bi % Cin, b = bi / Cin;
    const int m = m0 + mt;
    const float v = m < M ? x[(static_cast<int64_t>(bi) * M + m) * 2 + part] : 0.f;
    Xs[(mt * Bp + b) * Kp + part * Cin + i] = v;
  }
  // w[i][o][m][2] -> real block [[wr, wi], [-wi, wr]]
  for (int idx = tid; idx < Cin * Cout * kMT * 2; idx += kNT) {
    const int part = idx & 1;
    const int mt = (idx >> 1) % kMT;
    const int io = (idx >> 1) / kMT;
    const int o = io % Cout, i = io / Cout;
    const int m = m0 + mt;
    const float v = m < M ? w[(static_cast<int64_t>(io) * M + m) * 2 + part] : 0.f;
    float* Wm = Ws + mt * Kp * Np;
    if (part == 0) {
      Wm[i * Np + o] = v;                    // Wr
      Wm[(Cin + i) * Np + Cout + o] = v;     // Wr
    } else {
      Wm[i * Np + Cout + o] = v;             // Wi
      Wm[(Cin + i) * Np + o] = -v;           // -Wi
    }
  }
  __syncthreads();
  // ---- per-mode GEMMs on MFMA: wave wv handles modes wv, wv + 4, ...
  const int lane = tid & 63, wv = tid >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  for (int mt = wv; mt < kMT; mt += kNT / 64) {
    const float* Xm = Xs + mt * Bp * Kp;
    const float* Wm = Ws + mt * Kp * Np;
    float* Ym = Ys + mt * Bp * Np;
    for (int mi = 0; mi < Bp / 16; ++mi)
      for (int ni = 0; ni < Np / 16; ++ni) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < Kp / 4; ++ks) {
          const float a = Xm[(mi * 16 + r16) * Kp + ks * 4 + kq];
          const float bv = Wm[(ks * 4 + kq) * Np + ni * 16 + r16];
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) Ym[(mi * 16 + kq * 4 + i) * Np + ni * 16 + r16] = acc[i];
      }
  }
  __syncthreads();
  // ---- store y[b][o][m][2]
  for (int idx = tid; idx < B * Cout * kMT * 2; idx += kNT) {
    const int part = idx & 1;
    const int mt = (idx >> 1) % kMT;
    const int bo = (idx >> 1) / kMT;
    const int o = bo % Cout, b = bo / Cout;
    const int m = m0 + mt;
    if (m < M) y[(static_cast<int64_t>(bo) * M + m) * 2 + part] = Ys[(mt * Bp + b) * Np + part * Cout + o];
  }
}

// Small batch (B <= 8): the MFMA M dimension (batch) would be >= 50% padding and the op is
// a pure stream over the per-mode weights (Cin*Cout*M complex, 6.5 MB for 20x20x2048).  A
// workgroup owns 64 consecutive (o, m) outputs (coalesced along m); its 4 waves split the Cin
// sum (split-K, reduced through LDS) so a 20x2048-mode layer runs 2560 waves instead of 640 --
// with one wave per SIMD the per-thread chain of Cin dependent loads was the whole kernel time.
// Pair: float2, or uint32_t for the bf16 instance -- a packed pair per load and store, unpacked to fp32 (exact), the
// same fp32 FMAs and reduction, rounded once at the store.
template <int NB, typename Pair>
__global__ void __launch_bounds__(256) fno_mix_small_kernel(const Pair* __restrict__ x, const Pair* __restrict__ w,
                                                            Pair* __restrict__ y, int B, int Cin, int Cout, int M) {
  __shared__ float2 red[3][NB][64];
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 64 + lane;
  const bool live = t < static_cast<int64_t>(Cout) * M;
  const int o = live ? static_cast<int>(t / M) : 0;
  const int mm = live ? static_cast<int>(t - static_cast<int64_t>(o) * M) : 0;
  float2 acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = make_float2(0.f, 0.f);
  const int i0 = s * Cin / 4, i1 = (s + 1) * Cin / 4;
  if (live) {
#pragma unroll 8
    for (int i = i0; i < i1; ++i) {
      const float2 wv = pair_load(w[(static_cast<int64_t>(i) * Cout + o) * M + mm]);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b < B) {
          const float2 xv = pair_load(x[(static_cast<int64_t>(b) * Cin + i) * M + mm]);
          acc[b].x = fmaf(xv.x, wv.x, fmaf(-xv.y, wv.y, acc[b].x));
          acc[b].y = fmaf(xv.x, wv.y, fmaf(xv.y, wv.x, acc[b].y));
        }
      }
    }
  }
  if (s > 0) {
#pragma unroll
    for (int b = 0; b < NB; ++b) red[s - 1][b][lane] = acc[b];
  }
  __syncthreads();
  if (s != 0 || !live) return;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b < B) {
      float2 v = acc[b];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        v.x += red[r][b][lane].x;
        v.y += red[r][b][lane].y;
      }
      pair_store(&y[(static_cast<int64_t>(b) * Cout + o) * M + mm], v);
    }
  }
}

// The bf16 stream kernel, two modes per lane: the op streams the weights, and with one 4-byte pair per lane a wave's
// load is 256 bytes -- half a fp32 wave's -- so the narrow instance issues as many requests as fp32 for half the bytes.
// Here a lane owns the modes 2 mp and 2 mp + 1 of its output channel and every load and store is 8 bytes.  M must be
// even (row starts stay 8-byte aligned; an odd M runs the one-mode instance) and x, w, y 8-byte aligned.  The sums
// run in the order of the one-mode instance: the same bits.
template <int NB>
__global__ void __launch_bounds__(256) fno_mix_small2_kernel(const uint2* __restrict__ x, const uint2* __restrict__ w,
                                                             uint2* __restrict__ y, int B, int Cin, int Cout, int Mh) {
  __shared__ float4 red[3][NB][64];
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 64 + lane;
  const bool live = t < static_cast<int64_t>(Cout) * Mh;
  const int o = live ? static_cast<int>(t / Mh) : 0;
  const int mp = live ? static_cast<int>(t - static_cast<int64_t>(o) * Mh) : 0;
  float4 acc[NB];  // (re, im) of mode 2 mp, (re, im) of mode 2 mp + 1
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int i0 = s * Cin / 4, i1 = (s + 1) * Cin / 4;
  if (live) {
#pragma unroll 4
    for (int i = i0; i < i1; ++i) {
      const uint2 wp = w[(static_cast<int64_t>(i) * Cout + o) * Mh + mp];
      const float2 w0 = pair_load(wp.x), w1 = pair_load(wp.y);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b < B) {
          const uint2 xp = x[(static_cast<int64_t>(b) * Cin + i) * Mh + mp];
          const float2 x0 = pair_load(xp.x), x1 = pair_load(xp.y);
          acc[b].x = fmaf(x0.x, w0.x, fmaf(-x0.y, w0.y, acc[b].x));
          acc[b].y = fmaf(x0.x, w0.y, fmaf(x0.y, w0.x, acc[b].y));
          acc[b].z = fmaf(x1.x, w1.x, fmaf(-x1.y, w1.y, acc[b].z));
          acc[b].w = fmaf(x1.x, w1.y, fmaf(x1.y, w1.x, acc[b].w));
        }
      }
    }
  }
  if (s > 0) {
#pragma unroll
    for (int b = 0; b < NB; ++b) red[s - 1][b][lane] = acc[b];
  }
  __syncthreads();
  if (s != 0 || !live) return;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b < B) {
      float4 v = acc[b];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float4 q = red[r][b][lane];
        v.x += q.x;
        v.y += q.y;
        v.z += q.z;
        v.w += q.w;
      }
      y[(static_cast<int64_t>(b) * Cout + o) * Mh + mp] = make_uint2(pk_bf16(v.x, v.y), pk_bf16(v.z, v.w));
    }
  }
}

// bf16, B > 8 (or on request): the per-mode real-block GEMM on v_mfma_f32_16x16x32_bf16.  The contraction is
// interleaved, k = 2 i for re and k = 2 i + 1 for im, so the K-major x tile [mode][b][k] is x's pair words copied
// unchanged; the K-major weight tile [mode][n][k] holds row n = 2 o as (wr, -wi) and row n = 2 o + 1 as (wi, wr) -- a
// sign flip and a rotate of the pair word, both exact.  The weights are the MFMA's A operand (rows n) and the batch its
// B operand (columns b): a lane's four accumulators are then (re, im) of two output channels of one sample, packed to
// two result words without a cross-lane exchange.  Rows b >= B, n >= 2 Cout, the K padding and the modes past M are
// zeros WRITTEN into the tile (0 * stale-NaN is NaN); nothing outside x, w or y is loaded or stored.  Each mode's tile
// starts 16 bytes (y: one word) further than a multiple of the row pitch, so lanes that walk the mode index hit
// different banks.  LDS: fno_mix_lds_bf16.
__global__ void __launch_bounds__(kNT) fno_mix_bf16_kernel(const uint32_t* __restrict__ x, const uint32_t* __restrict__ w,
                                                           uint32_t* __restrict__ y, int B, int Cin, int Cout, int M,
                                                           int MT, int pitch) {
  extern __shared__ __attribute__((aligned(16))) char smem_b[];
  const int Bp = (B + 15) & ~15, Np = (2 * Cout + 15) & ~15;
  const int ksteps = (pitch - 16) / 64;            // 32-deep k-steps
  const int xs = Bp * pitch + 16, ws = Np * pitch + 16, ys = Bp * (Np / 2) + 1;  // per-mode strides (bytes, bytes, words)
  char* Xs = smem_b;
  char* Ws = Xs + MT * xs;
  uint32_t* Ys = reinterpret_cast<uint32_t*>(Ws + MT * ws);
  const int m0 = blockIdx.x * MT;
  const int tid = threadIdx.x;
  const int sh = __ffs(MT) - 1;                    // MT is 4, 8 or 16
  for (int i = tid; i < MT * (xs + ws) / 16; i += kNT) reinterpret_cast<uint4*>(smem_b)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  // x[b][i][m]: one thread per (b, i, mode), the mode index fastest
  for (int idx = tid; idx < B * Cin * MT; idx += kNT) {
    const int mt = idx & (MT - 1), bi = idx >> sh;
    const int i = bi % Cin, b = bi / Cin;
    const int m = m0 + mt;
    if (m < M) *reinterpret_cast<uint32_t*>(Xs + mt * xs + b * pitch + 4 * i) = x[static_cast<int64_t>(bi) * M + m];
  }
  // w[i][o][m] -> rows 2 o: (wr, -wi), 2 o + 1: (wi, wr)
  for (int idx = tid; idx < Cin * Cout * MT; idx += kNT) {
    const int mt = idx & (MT - 1), io = idx >> sh;
    const int o = io % Cout, i = io / Cout;
    const int m = m0 + mt;
    if (m < M) {
      const uint32_t v = w[static_cast<int64_t>(io) * M + m];  // wr | wi << 16
      char* dst = Ws + mt * ws + 2 * o * pitch + 4 * i;
      *reinterpret_cast<uint32_t*>(dst) = v ^ 0x80000000u;
      *reinterpret_cast<uint32_t*>(dst + pitch) = (v >> 16) | (v << 16);
    }
  }
  __syncthreads();
  // ---- per-mode GEMMs: wave wv handles modes wv, wv + 4, ...
  const int lane = tid & 63, wv = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  for (int mt = wv; mt < MT && m0 + mt < M; mt += kNT / 64) {
    const char* Wm = Ws + mt * ws + l15 * pitch + 16 * lq;
    const char* Xm = Xs + mt * xs + l15 * pitch + 16 * lq;
    uint32_t* Ym = Ys + mt * ys;
    for (int ni = 0; ni < Np / 16; ++ni)
      for (int mi = 0; mi < Bp / 16; ++mi) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < ksteps; ++ks) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(Wm + ni * 16 * pitch + ks * 64);
          const bf16x8 bv = *reinterpret_cast<const bf16x8*>(Xm + mi * 16 * pitch + ks * 64);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bv, acc, 0, 0, 0);
        }
        // acc[i] = row n = 16 ni + 4 lq + i, column b = 16 mi + l15: channels 8 ni + 2 lq and + 1
        uint32_t* dst = Ym + (mi * 16 + l15) * (Np / 2) + ni * 8 + 2 * lq;
        dst[0] = pk_bf16(acc[0], acc[1]);
        dst[1] = pk_bf16(acc[2], acc[3]);
      }
  }
  __syncthreads();
  // ---- store y[b][o][m]
  for (int idx = tid; idx < B * Cout * MT; idx += kNT) {
    const int mt = idx & (MT - 1), bo = idx >> sh;
    const int o = bo % Cout, b = bo / Cout;
    const int m = m0 + mt;
    if (m < M) y[static_cast<int64_t>(bo) * M + m] = Ys[mt * ys + b * (Np / 2) + o];
  }
}

template <typename Pair>
void launch_stream(const Pair* x, const Pair* w, Pair* y, int B, int Cin, int Cout, int M, hipStream_t st) {
  const int64_t n = static_cast<int64_t>(Cout) * M;
  const dim3 grid(static_cast<uint32_t>((n + 63) / 64));
  if (B <= 1) hipLaunchKernelGGL((fno_mix_small_kernel<1, Pair>), grid, dim3(256), 0, st, x, w, y, B, Cin, Cout, M);
  else if (B <= 2) hipLaunchKernelGGL((fno_mix_small_kernel<2, Pair>), grid, dim3(256), 0, st, x, w, y, B, Cin, Cout, M);
  else if (B <= 4) hipLaunchKernelGGL((fno_mix_small_kernel<4, Pair>), grid, dim3(256), 0, st, x, w, y, B, Cin, Cout, M);
  else hipLaunchKernelGGL((fno_mix_small_kernel<8, Pair>), grid, dim3(256), 0, st, x, w, y, B, Cin, Cout, M);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: fno_mix launch: ") + hipGetErrorString(e));
}

void launch_stream2(const uint2* x, const uint2* w, uint2* y, int B, int Cin, int Cout, int Mh, hipStream_t st) {
  const int64_t n = static_cast<int64_t>(Cout) * Mh;
  const dim3 grid(static_cast<uint32_t>((n + 63) / 64));
  if (B <= 1) hipLaunchKernelGGL(fno_mix_small2_kernel<1>, grid, dim3(256), 0, st, x, w, y, B, Cin, Cout, Mh);
  else if (B <= 2) hipLaunchKernelGGL(fno_mix_small2_kernel<2>, grid, dim3(256), 0, st, x, w, y, B, Cin, Cout, Mh);
  else if (B <= 4) hipLaunchKernelGGL(fno_mix_small2_kernel<4>, grid, dim3(256), 0, st, x, w, y, B, Cin, Cout, Mh);
  else hipLaunchKernelGGL(fno_mix_small2_kernel<8>, grid, dim3(256), 0, st, x, w, y, B, Cin, Cout, Mh);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: fno_mix launch: ") + hipGetErrorString(e));
}

}  // namespace

void launch_fno_mix(const FnoMixLaunch& p, void* stream) {
  if (p.B <= 0 || p.M <= 0 || p.Cout <= 0) return;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool aligned8 = (reinterpret_cast<uintptr_t>(p.x) | reinterpret_cast<uintptr_t>(p.w) |
                         reinterpret_cast<uintptr_t>(p.y)) % 8 == 0;
  const FnoMixRoute r = fno_mix_route(p.B, p.Cin, p.Cout, p.M, p.bf16 != 0, p.mfma != 0, aligned8);
  if (r.kind != FnoMixKind::Mfma) {
    // up to 8 samples per launch (a tile beyond the MFMA kernel's LDS, e.g. fp32 width 40 at any batch: the split-K
    // stream kernel has no channel limit)
    for (int b0 = 0; b0 < p.B; b0 += 8) {
      const int nb = p.B - b0 < 8 ? p.B - b0 : 8;
      const int64_t xo = static_cast<int64_t>(b0) * p.Cin * p.M, yo = static_cast<int64_t>(b0) * p.Cout * p.M;
      if (r.vec == 2)  // M is even, so xo and yo are: the 8-byte alignment holds for every launch
        launch_stream2(reinterpret_cast<const uint2*>(static_cast<const uint32_t*>(p.x) + xo),
                       static_cast<const uint2*>(p.w), reinterpret_cast<uint2*>(static_cast<uint32_t*>(p.y) + yo), nb,
                       p.Cin, p.Cout, p.M / 2, st);
      else if (p.bf16)
        launch_stream(static_cast<const uint32_t*>(p.x) + xo, static_cast<const uint32_t*>(p.w),
                      static_cast<uint32_t*>(p.y) + yo, nb, p.Cin, p.Cout, p.M, st);
      else
        launch_stream(static_cast<const float2*>(p.x) + xo, static_cast<const float2*>(p.w),
                      static_cast<float2*>(p.y) + yo, nb, p.Cin, p.Cout, p.M, st);
    }
    return;
  }
  const void* fn = p.bf16 ? reinterpret_cast<const void*>(fno_mix_bf16_kernel) : reinterpret_cast<const void*>(fno_mix_kernel);
  if (r.lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(r.lds));
    if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: fno_mix attr: ") + hipGetErrorString(e));
  }
  const dim3 grid(static_cast<uint32_t>(r.wgs));
  if (p.bf16)
    hipLaunchKernelGGL(fno_mix_bf16_kernel, grid, dim3(kNT), static_cast<size_t>(r.lds), st,
                       static_cast<const uint32_t*>(p.x), static_cast<const uint32_t*>(p.w), static_cast<uint32_t*>(p.y),
                       p.B, p.Cin, p.Cout, p.M, r.mt, r.pitch);
  else
    hipLaunchKernelGGL(fno_mix_kernel, grid, dim3(kNT), static_cast<size_t>(r.lds), st, static_cast<const float*>(p.x),
                       static_cast<const float*>(p.w), static_cast<float*>(p.y), p.B, p.Cin, p.Cout, p.M);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: fno_mix launch: ") + hipGetErrorString(e));
}

}  // namespace amd_dft

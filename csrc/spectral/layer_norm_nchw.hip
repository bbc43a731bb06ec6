// LayerNorm over the channels of a channel-first field (the pre-norm of a transformer block on [B, C, nlat, nlon]):
//   y[b, c, p] = (x[b, c, p] - mean[b, p]) * rsqrt(var[b, p] + eps) * gamma[c] + beta[c],
// mean and the biased variance over c, p over the flattened trailing dimensions.  bf16 or fp32 I/O, fp32 statistics
// and arithmetic, one rounding at a bf16 store.  A pure stream: the reduction runs over the strided dimension, so
// the work is split over pixels and no lane ever needs another lane's pixel.
//
// Work split (layer_norm_nchw_route, spectral.h).  A channel row is contiguous over pixels.  A lane owns V
// consecutive pixels (V = 4: 16-byte fp32 / 8-byte bf16 accesses), a wave 64 V pixels of one channel row per load, a
// 256-thread workgroup one tile of TP = 64 V pixels of one batch entry; its four waves take the channels round-robin
// (wave w: c = w, w + 4, ...).  Small calls narrow the tile (V = 2, V = 1) until the grid has kLnNchwFillWgs
// workgroups.
//
// Moments.  Every value enters as d = x - K with K = x[b, 0, p], the pixel's first channel, so a pixel with
// |mean| >> std keeps the precision of its deviations and C = 1 gives d = 0 and exactly beta.  A lane walks its
// channels in chunks of kCH held in registers; a chunk gives (n, mean of d, M2) by the two-pass form (sum, then
// squares about the chunk mean) and is merged into the lane's running triple by Chan's update.  The chunk sizes are
// wave-uniform, so the update's divisions are scalar work.  The four waves' (mean, M2) pairs meet in LDS (2 x 4 x TP
// floats, 8 KB at V = 4) behind the kernel's one barrier; every wave merges them in wave order and gets the same bits.
// E[x^2] - E[x]^2 is never formed.  No atomics: bit-identical run to run and under graph replay.
//
// Routes.
//   resident  C <= 4 kLnNchwResident (128): the lane's <= 32 channels x V pixels stay in registers (as d) between the
//             moment pass and the normalise pass -- one read and one write of the tensor.
//   reread    every larger C: the moment pass streams the chunks, the normalise pass reads the tile again.  The
//             tile is C rows of TP elements (C KB-sized pieces a workgroup just touched), so the second read comes
//             from L2 where the tile fits next to its neighbours'; HBM sees one read and one write there too.
//
// Edges.  VEC = false (P % V != 0, or x / y not on a V-element boundary): per-element loads and stores, each guarded
// by p < P; VEC = true: one guard per lane (P % V == 0: the V pixels are inside or outside together).  Pixels >= P
// and channels >= C are neither loaded nor stored.  The arithmetic is the same expression tree in every instance
// (explicit fma), so a view at an odd offset gives the bits of the aligned call.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "spectral.h"

namespace amd_dft {
namespace {

constexpr int kCH = 8;                // channels per register chunk and wave
constexpr int kKR = kLnNchwResident;  // channels a lane keeps on the resident route

__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ uint16_t f2bf(float f) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(f)); }
__device__ __forceinline__ uint32_t bfpack(float a, float b) {
  return static_cast<uint32_t>(f2bf(a)) | (static_cast<uint32_t>(f2bf(b)) << 16);
}

// V consecutive pixels p.. of the channel row at `row` (a pointer to pixel p); pixels >= P read as 0 and are not loaded
template <bool BF, int V, bool VEC>
__device__ __forceinline__ void ld_px(const char* row, int p, int P, float (&v)[V]) {
#pragma unroll
  for (int e = 0; e < V; ++e) v[e] = 0.f;
  if constexpr (VEC && V > 1) {
    if (p < P) {
      if constexpr (BF && V == 4) {
        const uint2 u = *reinterpret_cast<const uint2*>(row);
        v[0] = bf_lo(u.x), v[1] = bf_hi(u.x), v[2] = bf_lo(u.y), v[3] = bf_hi(u.y);
      } else if constexpr (BF) {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(row);
        v[0] = bf_lo(u), v[1] = bf_hi(u);
      } else if constexpr (V == 4) {
        const float4 u = *reinterpret_cast<const float4*>(row);
        v[0] = u.x, v[1] = u.y, v[2] = u.z, v[3] = u.w;
      } else {
        const float2 u = *reinterpret_cast<const float2*>(row);
        v[0] = u.x, v[1] = u.y;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (p + e < P) {
        if constexpr (BF) v[e] = bf_lo(reinterpret_cast<const uint16_t*>(row)[e]);
        else v[e] = reinterpret_cast<const float*>(row)[e];
      }
    }
  }
}

template <bool BF, int V, bool VEC>
__device__ __forceinline__ void st_px(char* row, int p, int P, const float (&v)[V]) {
  if constexpr (VEC && V > 1) {
    if (p < P) {
      if constexpr (BF && V == 4) *reinterpret_cast<uint2*>(row) = make_uint2(bfpack(v[0], v[1]), bfpack(v[2], v[3]));
      else if constexpr (BF) *reinterpret_cast<uint32_t*>(row) = bfpack(v[0], v[1]);
      else if constexpr (V == 4) *reinterpret_cast<float4*>(row) = make_float4(v[0], v[1], v[2], v[3]);
      else *reinterpret_cast<float2*>(row) = make_float2(v[0], v[1]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (p + e < P) {
        if constexpr (BF) reinterpret_cast<uint16_t*>(row)[e] = f2bf(v[e]);
        else reinterpret_cast<float*>(row)[e] = v[e];
      }
    }
  }
}

// Chan's update of (na, mean, m2) by a second triple (nb, mb, m2b); na, nb wave-uniform, nb > 0
__device__ __forceinline__ void chan_merge(float na, float& mean, float& m2, float nb, float mb, float m2b) {
  const float fb = nb / (na + nb);
  const float delta = mb - mean;
  mean = __builtin_fmaf(delta, fb, mean);
  m2 = __builtin_fmaf(delta * delta, na * fb, m2 + m2b);
}

template <bool BF, int V, bool VEC, bool RES>
__global__ void __launch_bounds__(256) layer_norm_nchw_kernel(const void* __restrict__ x, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, void* __restrict__ y,
                                                               int C, int P, int tiles, float eps) {
  constexpr int ES = BF ? 2 : 4;
  constexpr int TP = 64 * V;
  constexpr int NX = RES ? kKR : kCH;  // channel values a lane holds at a time
  __shared__ float part[4][2][TP];     // per wave: mean of d, M2, per pixel of the tile

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t b = blockIdx.x / tiles;
  const int p = (blockIdx.x % tiles) * TP + lane * V;  // first of this lane's V pixels (may be >= P)
  const int64_t base = b * C * static_cast<int64_t>(P) + p;
  const char* xb = static_cast<const char*>(x) + base * ES;
  char* yb = static_cast<char*>(y) + base * ES;
  const int64_t rowb = static_cast<int64_t>(P) * ES;  // bytes between channel rows
  const int nch = wv < C ? (C - wv + 3) / 4 : 0;      // channels of this wave: c = wv + 4 k, k < nch

  float K[V];
  ld_px<BF, V, VEC>(xb, p, P, K);

  float xr[NX][V];
  float cnt = 0.f, mean[V], m2[V];
#pragma unroll
  for (int e = 0; e < V; ++e) mean[e] = m2[e] = 0.f;

  // one chunk: kCH rows from channel index k0 of this wave into xr[r0 ..] as d = x - K, merged into the moments
  auto chunk = [&](int k0, auto r0c) {
    constexpr int r0 = decltype(r0c)::value;
    const int nv = min(kCH, nch - k0);
    if (nv <= 0) return;
#pragma unroll
    for (int j = 0; j < kCH; ++j)
      if (j < nv) ld_px<BF, V, VEC>(xb + (wv + 4 * static_cast<int64_t>(k0 + j)) * rowb, p, P, xr[r0 + j]);
    const float fn = static_cast<float>(nv), rn = 1.0f / fn;
    float cm[V], c2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) cm[e] = c2[e] = 0.f;
#pragma unroll
    for (int j = 0; j < kCH; ++j) {
      if (j < nv) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          xr[r0 + j][e] -= K[e];
          cm[e] += xr[r0 + j][e];
        }
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) cm[e] *= rn;
#pragma unroll
    for (int j = 0; j < kCH; ++j) {
      if (j < nv) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float t = xr[r0 + j][e] - cm[e];
          c2[e] = __builtin_fmaf(t, t, c2[e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) chan_merge(cnt, mean[e], m2[e], fn, cm[e], c2[e]);
    cnt += fn;
  };

  if constexpr (RES) {
    chunk(0 * kCH, std::integral_constant<int, 0 * kCH>{});
    chunk(1 * kCH, std::integral_constant<int, 1 * kCH>{});
    chunk(2 * kCH, std::integral_constant<int, 2 * kCH>{});
    chunk(3 * kCH, std::integral_constant<int, 3 * kCH>{});
    static_assert(kKR == 4 * kCH, "the resident route holds four chunks");
  } else {
    for (int k0 = 0; k0 < nch; k0 += kCH) chunk(k0, std::integral_constant<int, 0>{});
  }

  // ---- the four waves' partials meet in LDS; every wave merges them in wave order
#pragma unroll
  for (int e = 0; e < V; ++e) {
    part[wv][0][lane * V + e] = mean[e];
    part[wv][1][lane * V + e] = m2[e];
  }
  __syncthreads();
  float rstd[V];
  cnt = 0.f;
#pragma unroll
  for (int e = 0; e < V; ++e) mean[e] = m2[e] = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < C) {
      const float fn = static_cast<float>((C - w + 3) / 4);
#pragma unroll
      for (int e = 0; e < V; ++e) chan_merge(cnt, mean[e], m2[e], fn, part[w][0][lane * V + e], part[w][1][lane * V + e]);
      cnt += fn;
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) rstd[e] = 1.0f / sqrtf(m2[e] / static_cast<float>(C) + eps);

  // ---- normalise: ((d - mean_d) * rstd) * gamma[c] + beta[c]
  auto norm_rows = [&](int k0, auto r0c, bool reload) {
    constexpr int r0 = decltype(r0c)::value;
    const int nv = min(kCH, nch - k0);
    if (nv <= 0) return;
    if (reload) {
#pragma unroll
      for (int j = 0; j < kCH; ++j)
        if (j < nv) ld_px<BF, V, VEC>(xb + (wv + 4 * static_cast<int64_t>(k0 + j)) * rowb, p, P, xr[r0 + j]);
    }
#pragma unroll
    for (int j = 0; j < kCH; ++j) {
      if (j < nv) {
        const int c = wv + 4 * (k0 + j);
        const float g = gamma != nullptr ? gamma[c] : 1.0f;
        const float bt = beta != nullptr ? beta[c] : 0.0f;
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float d = reload ? xr[r0 + j][e] - K[e] : xr[r0 + j][e];
          o[e] = __builtin_fmaf((d - mean[e]) * rstd[e], g, bt);
        }
        st_px<BF, V, VEC>(yb + static_cast<int64_t>(c) * rowb, p, P, o);
      }
    }
  };
  if constexpr (RES) {
    norm_rows(0 * kCH, std::integral_constant<int, 0 * kCH>{}, false);
    norm_rows(1 * kCH, std::integral_constant<int, 1 * kCH>{}, false);
    norm_rows(2 * kCH, std::integral_constant<int, 2 * kCH>{}, false);
    norm_rows(3 * kCH, std::integral_constant<int, 3 * kCH>{}, false);
  } else {
    for (int k0 = 0; k0 < nch; k0 += kCH) norm_rows(k0, std::integral_constant<int, 0>{}, true);
  }
}

template <bool BF, int V, bool VEC>
void launch_route(const LayerNormNchwLaunch& p, const LayerNormNchwRoute& r, hipStream_t st) {
  const int tiles = static_cast<int>((p.P + r.TP - 1) / r.TP);
  const dim3 grid(static_cast<unsigned>(r.wgs));
#define L_(RES)                                                                                                     \
  hipLaunchKernelGGL((layer_norm_nchw_kernel<BF, V, VEC, RES>), grid, dim3(256), 0, st, p.x, p.w, p.b, p.y, p.C, p.P, \
                     tiles, p.eps)
  if (r.resident) L_(true);
  else L_(false);
#undef L_
}

template <bool BF>
void launch_dtype(const LayerNormNchwLaunch& p, const LayerNormNchwRoute& r, hipStream_t st) {
  if (r.V == 4) {
    if (r.vec) launch_route<BF, 4, true>(p, r, st);
    else launch_route<BF, 4, false>(p, r, st);
  } else if (r.V == 2) {
    if (r.vec) launch_route<BF, 2, true>(p, r, st);
    else launch_route<BF, 2, false>(p, r, st);
  } else {
    launch_route<BF, 1, false>(p, r, st);
  }
}

}  // namespace

void launch_layer_norm_nchw(const LayerNormNchwLaunch& p, void* stream) {
  if (p.B == 0 || p.P == 0) return;
  if (p.C < 1) throw std::runtime_error("amd_dft: layer_norm_nchw: C must be >= 1");
  const uintptr_t ptrs = reinterpret_cast<uintptr_t>(p.x) | reinterpret_cast<uintptr_t>(p.y);
  const LayerNormNchwRoute r = layer_norm_nchw_route(p.B, p.C, p.P, p.bf16 != 0, static_cast<int>((ptrs & 15) ? (ptrs & -ptrs) : 16));
  if (r.wgs >= (int64_t(1) << 31)) throw std::runtime_error("amd_dft: layer_norm_nchw: tensor too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (p.bf16) launch_dtype<true>(p, r, st);
  else launch_dtype<false>(p, r, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: layer_norm_nchw launch: ") + hipGetErrorString(e));
}

}  // namespace amd_dft

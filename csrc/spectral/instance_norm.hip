// Instance normalisation over the spatial plane of each (batch, channel) of an NCHW tensor (SFNO / FourCastNet-v2
// InstanceNorm2d):  y = (x - mean) * rsqrt(var + eps) * weight[c] + bias[c], biased variance over the P elements of
// a plane.  bf16 or fp32 I/O, fp32 statistics and arithmetic, one rounding at a bf16 store.  HBM-bound; two routes
// (instance_norm_route in spectral.h):
//
//   resident  one workgroup owns a plane, keeps it in LDS as fp32 and takes every pass but the first from there:
//             one HBM read, one write.
//   split     a plane is cut into S contiguous chunks.  in_chunk_kernel holds a chunk in LDS and writes its
//             (count, mean, M2) partial; in_split_norm_kernel merges the S partials of its plane in index order
//             (Chan's update; every chunk workgroup of a plane repeats the same merge and gets the same bits) and
//             normalises its chunk from HBM: two reads, one write.
//
// Statistics never form E[x^2] - E[x]^2.  All sums run over d = x - K with K the plane's first element, so a plane
// with |mean| >> std keeps the precision of its deviations and a constant plane gives d = 0, M2 = 0 and exactly
// `bias`.  Over the LDS copy: m1 = sum(d) / n, then e = d - m1, mean_d = m1 + sum(e) / n and
// M2 = sum(e^2) - sum(e)^2 / n (the corrected two-pass form).  The plane mean K + mean_d is carried as an fp32 pair
// (hi, lo) so that x - mean loses nothing where the mean is not an fp32 number.  (If K is an outlier of its plane the
// deviations d carry its rounding, up to 2^-24 sqrt(P) of the plane's std.)
//
// No atomics: per-thread strided sums, xor-butterfly wave sums, the waves' sums added in wave order.  Plane and
// chunk starts are p P + s chunk elements into the tensor, 16-byte aligned only by chance: every range is walked as
// a scalar head up to the next 16-byte boundary, 16-byte vectors, and a scalar tail (x and y start on a 16-byte
// boundary and share the pattern).  The LDS copy is shifted by `pad` floats so the vectors land 16-byte aligned in
// LDS too; only words written by this launch are read back.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "spectral.h"

namespace amd_dft {
namespace {

constexpr int kNT = kInThreads;
constexpr int kScratch = kInScratchBytes / 4;  // floats in front of the data image

__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float(static_cast<uint32_t>(h) << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(f)); }
__device__ __forceinline__ uint32_t bfpack(float a, float b) {
  return static_cast<uint32_t>(f2bf(a)) | (static_cast<uint32_t>(f2bf(b)) << 16);
}

template <bool BF>
__device__ __forceinline__ float ld_elem(const void* x, int64_t i) {
  if constexpr (BF) return bf2f(static_cast<const uint16_t*>(x)[i]);
  return static_cast<const float*>(x)[i];
}
template <bool BF>
__device__ __forceinline__ void st_elem(void* y, int64_t i, float v) {
  if constexpr (BF) static_cast<uint16_t*>(y)[i] = f2bf(v);
  else static_cast<float*>(y)[i] = v;
}

// A range of n elements starting g0 elements into a 16-byte-aligned tensor: head scalars, nv vectors of V, the rest
template <bool BF>
struct Range {
  static constexpr int V = BF ? 8 : 4;
  int head, nv, n, pad;
  __device__ Range(int64_t g0, int n_) : n(n_) {
    const int off = static_cast<int>(g0 % V);
    head = (V - off) % V;
    if (head > n) head = n;
    nv = (n - head) / V;
    pad = (4 - head % 4) % 4;  // LDS image shift: element `head` sits on a 16-byte boundary
  }
  __device__ int tail0() const { return head + nv * V; }
};

// the wave sums added in wave order; `slot` holds kNT / 64 floats and is used once per launch
__device__ __forceinline__ float block_sum(float v, float* slot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < kNT / 64; ++w) s += slot[w];
  return s;
}

template <bool BF>
__device__ __forceinline__ void load_range(const void* x, int64_t g0, const Range<BF>& r, float* d) {
  const int tid = threadIdx.x;
  for (int i = tid; i < r.head; i += kNT) d[i] = ld_elem<BF>(x, g0 + i);
  if constexpr (BF) {
    const uint16_t* xb = static_cast<const uint16_t*>(x) + g0 + r.head;
#pragma unroll 4
    for (int j = tid; j < r.nv; j += kNT) {
      const uint4 u = *reinterpret_cast<const uint4*>(xb + 8 * static_cast<int64_t>(j));
      float* o = d + r.head + 8 * j;
      *reinterpret_cast<float4*>(o) = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                                                  __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
      *reinterpret_cast<float4*>(o + 4) = make_float4(__uint_as_float(u.z << 16), __uint_as_float(u.z & 0xffff0000u),
                                                      __uint_as_float(u.w << 16), __uint_as_float(u.w & 0xffff0000u));
    }
  } else {
    const float* xf = static_cast<const float*>(x) + g0 + r.head;
#pragma unroll 4
    for (int j = tid; j < r.nv; j += kNT)
      *reinterpret_cast<float4*>(d + r.head + 4 * j) = *reinterpret_cast<const float4*>(xf + 4 * static_cast<int64_t>(j));
  }
  for (int i = r.tail0() + tid; i < r.n; i += kNT) d[i] = ld_elem<BF>(x, g0 + i);
}

// (mean of d = x - K, centred M2) of the n floats at d; red: 3 * kNT / 64 floats of scratch.  Every thread returns
// the same values.
struct Moments {
  float mean_d, m2;
};
__device__ __forceinline__ Moments lds_moments(const float* d, int n, float K, float* red) {
  const int tid = threadIdx.x;
  float s = 0.f;
  for (int i = tid; i < n; i += kNT) s += d[i] - K;
  const float m1 = block_sum(s, red) / static_cast<float>(n);
  float s2 = 0.f, q = 0.f;
  for (int i = tid; i < n; i += kNT) {
    const float e = (d[i] - K) - m1;
    s2 += e;
    q += e * e;
  }
  s2 = block_sum(s2, red + kNT / 64);
  q = block_sum(q, red + 2 * (kNT / 64));
  const float d2 = s2 / static_cast<float>(n);
  Moments m;
  m.mean_d = m1 + d2;
  m.m2 = fmaxf(q - s2 * d2, 0.f);
  return m;
}

// K + mean_d as an unevaluated fp32 pair (Knuth's two-sum)
__device__ __forceinline__ void two_sum(float a, float b, float& hi, float& lo) {
  hi = a + b;
  const float bb = hi - a;
  lo = (a - (hi - bb)) + (b - bb);
}

__device__ __forceinline__ float norm1(float v, float hi, float lo, float a, float b) {
  return fmaf((v - hi) - lo, a, b);
}

template <bool BF, bool STATS>
__global__ void __launch_bounds__(kNT) in_resident_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                          const float* __restrict__ w, const float* __restrict__ b,
                                                          float* __restrict__ stats, int P, int C, float eps) {
  extern __shared__ __attribute__((aligned(16))) float in_lds[];
  const int64_t plane = blockIdx.x;
  const int64_t g0 = plane * P;
  const Range<BF> r(g0, P);
  float* d = in_lds + kScratch + r.pad;
  load_range<BF>(x, g0, r, d);
  const float K = ld_elem<BF>(x, g0);
  __syncthreads();
  const Moments m = lds_moments(d, P, K, in_lds);
  const float rstd = 1.0f / sqrtf(m.m2 / static_cast<float>(P) + eps);
  float hi, lo;
  two_sum(K, m.mean_d, hi, lo);
  if constexpr (STATS) {
    if (threadIdx.x == 0) {
      stats[2 * plane] = hi;
      stats[2 * plane + 1] = rstd;
    }
    return;
  }
  const int c = static_cast<int>(plane % C);
  const float a = rstd * (w ? w[c] : 1.f);
  const float bb = b ? b[c] : 0.f;
  const int tid = threadIdx.x;
  for (int i = tid; i < r.head; i += kNT) st_elem<BF>(y, g0 + i, norm1(d[i], hi, lo, a, bb));
  if constexpr (BF) {
    uint16_t* yb = static_cast<uint16_t*>(y) + g0 + r.head;
#pragma unroll 2
    for (int j = tid; j < r.nv; j += kNT) {
      const float4 v0 = *reinterpret_cast<const float4*>(d + r.head + 8 * j);
      const float4 v1 = *reinterpret_cast<const float4*>(d + r.head + 8 * j + 4);
      *reinterpret_cast<uint4*>(yb + 8 * static_cast<int64_t>(j)) =
          make_uint4(bfpack(norm1(v0.x, hi, lo, a, bb), norm1(v0.y, hi, lo, a, bb)),
                     bfpack(norm1(v0.z, hi, lo, a, bb), norm1(v0.w, hi, lo, a, bb)),
                     bfpack(norm1(v1.x, hi, lo, a, bb), norm1(v1.y, hi, lo, a, bb)),
                     bfpack(norm1(v1.z, hi, lo, a, bb), norm1(v1.w, hi, lo, a, bb)));
    }
  } else {
    float* yf = static_cast<float*>(y) + g0 + r.head;
#pragma unroll 4
    for (int j = tid; j < r.nv; j += kNT) {
      const float4 v = *reinterpret_cast<const float4*>(d + r.head + 4 * j);
      *reinterpret_cast<float4*>(yf + 4 * static_cast<int64_t>(j)) =
          make_float4(norm1(v.x, hi, lo, a, bb), norm1(v.y, hi, lo, a, bb), norm1(v.z, hi, lo, a, bb),
                      norm1(v.w, hi, lo, a, bb));
    }
  }
  for (int i = r.tail0() + tid; i < r.n; i += kNT) st_elem<BF>(y, g0 + i, norm1(d[i], hi, lo, a, bb));
}

// split, first kernel: workgroup (plane, s) -> part[(plane S + s) * 4] = (count, mean of x - K, M2, unused)
template <bool BF>
__global__ void __launch_bounds__(kNT) in_chunk_kernel(const void* __restrict__ x, float* __restrict__ part, int64_t P,
                                                       int S, int chunk) {
  extern __shared__ __attribute__((aligned(16))) float in_lds[];
  const int64_t plane = blockIdx.x / S;
  const int s = static_cast<int>(blockIdx.x % S);
  const int64_t c0 = static_cast<int64_t>(s) * chunk;
  const int n = static_cast<int>(P - c0 < chunk ? P - c0 : chunk);
  const int64_t g0 = plane * P + c0;
  const Range<BF> r(g0, n);
  float* d = in_lds + kScratch + r.pad;
  load_range<BF>(x, g0, r, d);
  const float K = ld_elem<BF>(x, plane * P);
  __syncthreads();
  const Moments m = lds_moments(d, n, K, in_lds);
  if (threadIdx.x == 0)
    *reinterpret_cast<float4*>(part + 4 * static_cast<int64_t>(blockIdx.x)) =
        make_float4(static_cast<float>(n), m.mean_d, m.m2, 0.f);
}

// the S partials of a plane merged in index order (Chan et al.): mean of x - K and M2 over the whole plane
__device__ __forceinline__ Moments merge_parts(const float* __restrict__ part, int S) {
  float n = 0.f, mean = 0.f, m2 = 0.f;
  for (int s = 0; s < S; ++s) {
    const float4 pb = *reinterpret_cast<const float4*>(part + 4 * static_cast<int64_t>(s));
    const float nn = n + pb.x;
    const float delta = pb.y - mean;
    const float f = pb.x / nn;
    mean += delta * f;
    m2 += pb.z + delta * delta * n * f;
    n = nn;
  }
  Moments m;
  m.mean_d = mean;
  m.m2 = m2;
  return m;
}

// split, second kernel: merge, then normalise chunk (plane, s) from HBM
template <bool BF>
__global__ void __launch_bounds__(kNT) in_split_norm_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                            const float* __restrict__ w, const float* __restrict__ b,
                                                            const float* __restrict__ part, int64_t P, int C, int S,
                                                            int chunk, float eps) {
  extern __shared__ __attribute__((aligned(16))) float in_lds[];
  const int64_t plane = blockIdx.x / S;
  const int s = static_cast<int>(blockIdx.x % S);
  if (threadIdx.x == 0) {
    const Moments m = merge_parts(part + 4 * plane * S, S);
    float hi, lo;
    two_sum(ld_elem<BF>(x, plane * P), m.mean_d, hi, lo);
    in_lds[0] = hi;
    in_lds[1] = lo;
    in_lds[2] = 1.0f / sqrtf(m.m2 / static_cast<float>(P) + eps);
  }
  __syncthreads();
  const float hi = in_lds[0], lo = in_lds[1], rstd = in_lds[2];
  const int c = static_cast<int>(plane % C);
  const float a = rstd * (w ? w[c] : 1.f);
  const float bb = b ? b[c] : 0.f;
  const int64_t c0 = static_cast<int64_t>(s) * chunk;
  const int n = static_cast<int>(P - c0 < chunk ? P - c0 : chunk);
  const int64_t g0 = plane * P + c0;
  const Range<BF> r(g0, n);
  const int tid = threadIdx.x;
  for (int i = tid; i < r.head; i += kNT) st_elem<BF>(y, g0 + i, norm1(ld_elem<BF>(x, g0 + i), hi, lo, a, bb));
  if constexpr (BF) {
    const uint16_t* xb = static_cast<const uint16_t*>(x) + g0 + r.head;
    uint16_t* yb = static_cast<uint16_t*>(y) + g0 + r.head;
#pragma unroll 4
    for (int j = tid; j < r.nv; j += kNT) {
      const uint4 u = *reinterpret_cast<const uint4*>(xb + 8 * static_cast<int64_t>(j));
      const uint32_t wd[4] = {u.x, u.y, u.z, u.w};
      uint32_t o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        o[k] = bfpack(norm1(__uint_as_float(wd[k] << 16), hi, lo, a, bb),
                      norm1(__uint_as_float(wd[k] & 0xffff0000u), hi, lo, a, bb));
      *reinterpret_cast<uint4*>(yb + 8 * static_cast<int64_t>(j)) = make_uint4(o[0], o[1], o[2], o[3]);
    }
  } else {
    const float* xf = static_cast<const float*>(x) + g0 + r.head;
    float* yf = static_cast<float*>(y) + g0 + r.head;
#pragma unroll 4
    for (int j = tid; j < r.nv; j += kNT) {
      const float4 v = *reinterpret_cast<const float4*>(xf + 4 * static_cast<int64_t>(j));
      *reinterpret_cast<float4*>(yf + 4 * static_cast<int64_t>(j)) =
          make_float4(norm1(v.x, hi, lo, a, bb), norm1(v.y, hi, lo, a, bb), norm1(v.z, hi, lo, a, bb),
                      norm1(v.w, hi, lo, a, bb));
    }
  }
  for (int i = r.tail0() + tid; i < r.n; i += kNT)
    st_elem<BF>(y, g0 + i, norm1(ld_elem<BF>(x, g0 + i), hi, lo, a, bb));
}

// split, statistics only: one thread per plane merges its partials -> stats[plane] = (mean, rstd)
template <bool BF>
__global__ void __launch_bounds__(256) in_merge_stats_kernel(const void* __restrict__ x, const float* __restrict__ part,
                                                             float* __restrict__ stats, int64_t planes, int64_t P,
                                                             int S, float eps) {
  const int64_t plane = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (plane >= planes) return;
  const Moments m = merge_parts(part + 4 * plane * S, S);
  float hi, lo;
  two_sum(ld_elem<BF>(x, plane * P), m.mean_d, hi, lo);
  stats[2 * plane] = hi;
  stats[2 * plane + 1] = 1.0f / sqrtf(m.m2 / static_cast<float>(P) + eps);
}

void check(hipError_t e, const char* what) {
  if (e != hipSuccess)
    throw std::runtime_error(std::string("amd_dft: instance_norm: ") + what + ": " + hipGetErrorString(e));
}

template <bool BF>
void launch(const InstanceNormLaunch& p, const InstanceNormRoute& r, hipStream_t st) {
  const dim3 grid(static_cast<uint32_t>(r.wgs)), block(kNT);
  const size_t lds = static_cast<size_t>(r.lds);
  const int P = static_cast<int>(p.P), S = static_cast<int>(r.S), chunk = static_cast<int>(r.chunk);
  if (r.resident) {
    if (p.y)
      hipLaunchKernelGGL((in_resident_kernel<BF, false>), grid, block, lds, st, p.x, p.y, p.w, p.b, nullptr, P, p.C,
                         p.eps);
    else
      hipLaunchKernelGGL((in_resident_kernel<BF, true>), grid, block, lds, st, p.x, nullptr, nullptr, nullptr, p.stats,
                         P, p.C, p.eps);
    check(hipGetLastError(), "launch (resident)");
    return;
  }
  if (!p.part) throw std::invalid_argument("amd_dft: instance_norm: the split route needs its partials workspace");
  hipLaunchKernelGGL((in_chunk_kernel<BF>), grid, block, lds, st, p.x, p.part, p.P, S, chunk);
  check(hipGetLastError(), "launch (chunk statistics)");
  if (p.y) {
    hipLaunchKernelGGL((in_split_norm_kernel<BF>), grid, block, 16, st, p.x, p.y, p.w, p.b, p.part, p.P, p.C, S, chunk,
                       p.eps);
  } else {
    const dim3 g2(static_cast<uint32_t>((p.planes + 255) / 256));
    hipLaunchKernelGGL((in_merge_stats_kernel<BF>), g2, dim3(256), 0, st, p.x, p.part, p.stats, p.planes, p.P, S, p.eps);
  }
  check(hipGetLastError(), "launch (merge)");
}

}  // namespace

void launch_instance_norm(const InstanceNormLaunch& p, void* stream) {
  if (p.planes <= 0) return;
  if (p.P < 2 || p.P >= (int64_t(1) << 31) || p.C < 1 || (p.y == nullptr) == (p.stats == nullptr))
    throw std::invalid_argument("amd_dft: instance_norm: bad launch (2 <= P < 2^31, one of y / stats)");
  const InstanceNormRoute r = instance_norm_route(p.planes, p.P, p.bf16 != 0);
  if (r.wgs >= (int64_t(1) << 31)) throw std::invalid_argument("amd_dft: instance_norm: too many workgroups");
  if (p.bf16)
    launch<true>(p, r, static_cast<hipStream_t>(stream));
  else
    launch<false>(p, r, static_cast<hipStream_t>(stream));
}

}  // namespace amd_dft

// Discrete-continuous (DISCO) convolution on the sphere, the transposed (upsampling) half: a gather CSR over rows
// r = k * s + rho (output latitude k, longitude phase rho, s = nlon_out / nlon_in) applied to every coarse longitude,
//
//   y[n, k, s t + rho] = sum_e val[e] * z[n, p_e, k'_e, (d_e + t) mod nlon_in] (+ bias[n mod C]),   0 <= t < nlon_in,
//   e in [row_ptr[r], row_ptr[r + 1]),  idx[e] = (k'_e * K + p_e) * nlon_in + d_e sorted within a row.
//
// bf16 or fp32 z and y, fp32 val and bias, fp32 accumulation, the bias added in fp32, one rounding at a bf16 store.
//
// A workgroup owns one output latitude k, all s phases and PT planes (disco_t_route in spectral.h).  It reads the band
// of input latitudes [k'_lo, k'_hi] that its s rows touch from the table itself -- the first and the last entry of
// each row, idx is k'-major -- and stages that band of its planes into LDS as fp32, once for all phases, from the
// [p, k', j'] layout of z into the image [k' - lo][p][nlon_in], so idx - base is the LDS word of an entry.  The phases
// are the outer loop; within a phase lanes are (plane, t), kDiscoItems of them per lane and pass.  The entry stream of
// row k * s + rho is the same for every lane: it is fetched at wave-uniform addresses, four entries ahead, and walked
// in table order, so the summation order of an output depends on its row alone: results are bit-identical run to
// run, and no atomics are involved.  The longitude wrap is the compare-and-select of disco.hip with stride 1.
//
// A band taller than the LDS chunk (`rows` of the route) is walked in chunks of input latitudes: for each phase and
// pass the chunks of the phase's own band are staged one after the other, the entry pointer carries on where the
// previous chunk stopped and the accumulators stay in registers -- the order of the sum is unchanged.  The band is
// then staged once per (phase, pass) instead of once per workgroup.
//
// Store: y[plane, k, s t + rho], element stores at stride s (consecutive lanes are consecutive t).
//
// Nothing outside z, the table, bias and y is touched whatever the table holds: row_ptr values are clamped to
// [0, nnz], the band to the input grid, an entry below the chunk is skipped and one at or above its end stops the
// walk, so every LDS word read was written by this launch.  Workgroups are numbered from both poles inwards, all
// plane tiles of a latitude together: the rows near the poles carry the most entries and start first.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "spectral.h"

namespace amd_dft {
namespace {

constexpr int kNT = kDiscoThreads;
constexpr int kR = kDiscoItems;

__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float(static_cast<uint32_t>(h) << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(f)); }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

struct Args {
  const void* z;
  const int32_t* row_ptr;
  const int32_t* idx;
  const float* val;
  const float* bias;
  void* y;
  int64_t planes, C;
  int nlat_in, nlon_in, K, nlat_out, nlon_out, s, nnz, rows, ptiles;
};

// input latitudes [c0, c1) of the workgroup's planes, all K basis planes -> lds[pl][k' - c0][p][nlon_in] as fp32;
// planes past the end are not staged (no lane reads them).  LDS word i = ((k' - c0) K + p) nlon_in + j: a thread
// splits its first word once and then steps (k', p, j) by the split of kNT, no division in the loop.
template <bool BF, int PT>
__device__ __forceinline__ void stage(const Args& a, float* lds, int64_t plane0, int c0, int c1, int plane_stride) {
  const int W = a.nlon_in, K = a.K;
  const int n = (c1 - c0) * K * W;
  const int pin = a.nlat_in * W;
  const int i0 = static_cast<int>(threadIdx.x);
  const int q0 = i0 / W, step_q = kNT / W;
  const int j0 = i0 - q0 * W, step_j = kNT - step_q * W;
  const int k0 = q0 / K, step_k = step_q / K;
  const int p0 = q0 - k0 * K, step_p = step_q - step_k * K;
#pragma unroll
  for (int pl = 0; pl < PT; ++pl) {
    if (plane0 + pl >= a.planes) break;
    const int64_t g0 = (plane0 + pl) * static_cast<int64_t>(K) * pin + static_cast<int64_t>(c0) * W;
    float* d = lds + pl * plane_stride;
    int kk = k0, p = p0, j = j0;
    for (int i = i0; i < n; i += kNT) {
      const int src = p * pin + kk * W + j;  // < K * nlat_in * nlon_in < 2^31
      if constexpr (BF) d[i] = bf2f(static_cast<const uint16_t*>(a.z)[g0 + src]);
      else d[i] = static_cast<const float*>(a.z)[g0 + src];
      j += step_j;
      p += step_p;
      kk += step_k;
      if (j >= W) {
        j -= W;
        ++p;
      }
      if (p >= K) {  // p <= 2 K - 1 here
        p -= K;
        ++kk;
      }
    }
  }
}

// Entries [e, e1) with idx < lim, in table order; base = c0 * K * nlon_in is LDS word 0 of a plane.  Returns the
// entry it stopped at.  lane[r]: the lane's LDS offset pl * plane_stride + t of item r; thr[r] = nlon_in - t.
template <int RA>
__device__ __forceinline__ int walk(const Args& a, const float* lds, int e, int e1, int base, int lim,
                                    const int (&lane)[kR], const int (&thr)[kR], float (&acc)[kR]) {
  const int W = a.nlon_in;
  int row_start = base;
  auto one = [&](int id, float v) {
    if (id < row_start) return;  // not a sorted table: never read outside the chunk
    while (id - row_start >= W) row_start += W;
    const int d = id - row_start;
    const int off = id - base;
#pragma unroll
    for (int r = 0; r < RA; ++r) {
      const int w = off + lane[r] - (d >= thr[r] ? W : 0);
      acc[r] = fmaf(v, lds[w], acc[r]);
    }
  };
  while (e + 4 <= e1) {
    const int i0 = uni(a.idx[e]), i1 = uni(a.idx[e + 1]), i2 = uni(a.idx[e + 2]), i3 = uni(a.idx[e + 3]);
    if (i0 >= lim || i1 >= lim || i2 >= lim || i3 >= lim) break;
    const float v0 = a.val[e], v1 = a.val[e + 1], v2 = a.val[e + 2], v3 = a.val[e + 3];
    one(i0, v0);
    one(i1, v1);
    one(i2, v2);
    one(i3, v3);
    e += 4;
  }
  while (e < e1) {
    const int id = uni(a.idx[e]);
    if (id >= lim) break;
    one(id, a.val[e]);
    ++e;
  }
  return e;
}

template <bool BF, int PT>
__global__ void __launch_bounds__(kNT) disco_t_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) float disco_t_lds[];
  // heavy rows first: latitudes from both poles inwards, the plane tiles of one latitude together
  const int lin = blockIdx.x / a.ptiles;
  const int k = (lin & 1) ? a.nlat_out - 1 - (lin >> 1) : (lin >> 1);
  const int64_t plane0 = static_cast<int64_t>(blockIdx.x % a.ptiles) * PT;
  const int W = a.nlon_in;
  const int KW = a.K * W;
  const int plane_stride = a.rows * KW;
  const int nitems = PT * W;

  auto row_range = [&](int rho, int& e0, int& e1) {
    const int r = k * a.s + rho;
    e0 = min(max(uni(a.row_ptr[r]), 0), a.nnz);
    e1 = min(max(uni(a.row_ptr[r + 1]), e0), a.nnz);
  };
  auto band = [&](int e0, int e1, int& lo, int& hi) {  // input latitudes of a non-empty entry range
    lo = min(max(uni(a.idx[e0]) / KW, 0), a.nlat_in - 1);
    hi = min(max(uni(a.idx[e1 - 1]) / KW, lo), a.nlat_in - 1);
  };

  int klo = a.nlat_in, khi = -1;
  for (int rho = 0; rho < a.s; ++rho) {
    int e0, e1;
    row_range(rho, e0, e1);
    if (e1 > e0) {
      int lo, hi;
      band(e0, e1, lo, hi);
      klo = min(klo, lo);
      khi = max(khi, hi);
    }
  }
  const bool single = khi - klo + 1 <= a.rows;  // also when every row is empty
  if (single && khi >= klo) {
    stage<BF, PT>(a, disco_t_lds, plane0, klo, khi + 1, plane_stride);
    __syncthreads();
  }

  for (int rho = 0; rho < a.s; ++rho) {
    int e0, e1;
    row_range(rho, e0, e1);
    int plo = klo, phi = khi;
    if (!single && e1 > e0) band(e0, e1, plo, phi);
    if (e1 <= e0) phi = plo - 1;
    for (int item0 = 0; item0 < nitems; item0 += kNT * kR) {
      int lane[kR], thr[kR], to[kR], pls[kR];
      bool ok[kR];
      float acc[kR];
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        int item = item0 + r * kNT + static_cast<int>(threadIdx.x);
        int pl = item / W;
        ok[r] = item < nitems && plane0 + pl < a.planes;
        if (!ok[r]) {  // an idle lane follows item 0: plane0 is always there
          item = 0;
          pl = 0;
        }
        const int t = item - pl * W;
        to[r] = t;
        pls[r] = pl;
        lane[r] = pl * plane_stride + t;
        thr[r] = W - t;
        acc[r] = 0.f;
      }
      const int left = nitems - item0;
      const int ra = left >= kR * kNT ? kR : (left + kNT - 1) / kNT;  // slices of kNT items with any item
      bool any = false;
#pragma unroll
      for (int r = 0; r < kR; ++r) any |= ok[r];
      const bool busy = __builtin_amdgcn_ballot_w64(any) != 0;  // a wave without items still meets the barriers
      int e = e0;
      for (int c0 = plo; c0 <= phi; c0 += a.rows) {
        const int c1 = min(c0 + a.rows, phi + 1);
        if (!single) {
          __syncthreads();
          stage<BF, PT>(a, disco_t_lds, plane0, c0, c1, plane_stride);
          __syncthreads();
        }
        const int base = c0 * KW, lim = c1 * KW;  // a single band: c0 = klo, c1 = khi + 1
        if (!busy) continue;
        if (ra == 1) e = walk<1>(a, disco_t_lds, e, e1, base, lim, lane, thr, acc);
        else if (ra == 2) e = walk<2>(a, disco_t_lds, e, e1, base, lim, lane, thr, acc);
        else e = walk<kR>(a, disco_t_lds, e, e1, base, lim, lane, thr, acc);
        if (single) break;
      }
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        if (!ok[r]) continue;
        const int64_t n = plane0 + pls[r];
        const int64_t o = (n * a.nlat_out + k) * a.nlon_out + static_cast<int64_t>(a.s) * to[r] + rho;
        const float v = a.bias ? acc[r] + a.bias[n % a.C] : acc[r];
        if constexpr (BF) static_cast<uint16_t*>(a.y)[o] = f2bf(v);
        else static_cast<float*>(a.y)[o] = v;
      }
    }
  }
}

template <bool BF, int PT>
void launch(const Args& a, const DiscoTRoute& r, hipStream_t st) {
  hipLaunchKernelGGL((disco_t_kernel<BF, PT>), dim3(static_cast<uint32_t>(r.wgs)), dim3(kNT),
                     static_cast<size_t>(r.lds), st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: disco_t: launch: ") + hipGetErrorString(e));
}

}  // namespace

void launch_disco_t(const DiscoTLaunch& p, void* stream) {
  if (p.planes <= 0 || p.nlat_out <= 0 || p.nlon_out <= 0) return;
  if (p.nlat_in < 1 || p.nlon_in < 1 || p.K < 1 || p.C < 1 || p.nlon_out % p.nlon_in != 0 || p.nnz < 0 ||
      p.nnz >= (int64_t(1) << 31) ||
      static_cast<int64_t>(p.K) * p.nlat_in * p.nlon_in >= (int64_t(1) << 31) ||
      static_cast<int64_t>(p.nlat_out) * (p.nlon_out / p.nlon_in) >= (int64_t(1) << 31) - 1)
    throw std::invalid_argument("amd_dft: disco_t: bad launch (nlon_out % nlon_in, sizes below 2^31)");
  const DiscoTRoute r =
      disco_t_route(p.planes, p.nlat_in, p.nlon_in, p.K, p.nlat_out, p.nlon_out, p.nnz, p.bf16 != 0);
  if (r.lds > kDiscoLdsBytes)
    throw std::invalid_argument("amd_dft: disco_t: the K basis planes of an input latitude do not fit the LDS chunk");
  if (r.wgs >= (int64_t(1) << 31) || 4 * static_cast<int64_t>(p.nlon_in) >= (int64_t(1) << 31))
    throw std::invalid_argument("amd_dft: disco_t: too many workgroups");
  Args a;
  a.z = p.z;
  a.row_ptr = p.row_ptr;
  a.idx = p.idx;
  a.val = p.val;
  a.bias = p.bias;
  a.y = p.y;
  a.planes = p.planes;
  a.C = p.C;
  a.nlat_in = p.nlat_in;
  a.nlon_in = p.nlon_in;
  a.K = p.K;
  a.nlat_out = p.nlat_out;
  a.nlon_out = p.nlon_out;
  a.s = p.nlon_out / p.nlon_in;
  a.nnz = static_cast<int>(p.nnz);
  a.rows = r.rows;
  a.ptiles = static_cast<int>(r.ptiles);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (p.bf16) {
    if (r.pt == 4) launch<true, 4>(a, r, st);
    else launch<true, 1>(a, r, st);
  } else {
    if (r.pt == 4) launch<false, 4>(a, r, st);
    else launch<false, 1>(a, r, st);
  }
}

}  // namespace amd_dft

// Discrete-continuous (DISCO) convolutions on the sphere, both directions from one kernel template: a sparse,
// longitude-invariant filter tensor in CSR applied at every longitude of an output row.  bf16 or fp32 input and y,
// fp32 val (and bias), fp32 accumulation, one rounding at a bf16 store.
//
// The shared scheme.  A workgroup owns one output latitude and PT planes (disco_route in spectral.h) and walks the
// CSR rows of that latitude one after the other (the outer loop).  It reads the band of input latitudes [lo, hi]
// that those rows touch from the table itself -- the first and the last entry of each row, idx is sorted -- and stages
// that band of its planes into LDS as fp32, once for all its rows, so that idx - base is the LDS word of an entry
// within a plane.  Lanes are (plane, item), kDiscoItems of them per lane and pass.  The entry stream (idx, val) of a
// row is the same for every lane: it is fetched with uniform (scalar) loads, four entries ahead, and walked in table
// order, so the summation order of an output depends on its row alone: results are bit-identical run to run, and no
// atomics are involved.
//
// Longitude wrap: the start of the current nlon_in-word run of LDS is tracked as the stream advances (idx is sorted,
// so it only moves forward: scalar compare-and-add, no division), which gives d_e; an item at input longitude
// offset o reads LDS word idx - base + o, less nlon_in where d_e >= nlon_in - o (one compare and select per entry
// and lane, no integer modulo).
//
// A band taller than the LDS chunk (`rows` of the route) is walked in chunks of input latitudes: for each CSR row
// and pass the chunks of the row's own band are staged one after the other and the entry pointer carries on where
// the previous chunk stopped, the accumulators staying in registers -- the order of the sum is unchanged.  The band
// is then staged once per (row, pass) instead of once per workgroup.
//
// Nothing outside the input, the table, bias and y is touched whatever the table holds: row_ptr values are clamped to
// [0, nnz], the band to the input grid, an entry below the chunk is skipped and one at or above its end stops the
// walk, so every LDS word read was written by this launch.  Rows near the poles carry about nlon_in * band entries,
// rows near the equator about band^2: workgroups are numbered from both poles inwards, all plane tiles of a latitude
// together, so the heavy rows start first.
//
// Forward (TR = false, the gather half), s = nlon_in / nlon_out:
//   y[n, p, k', j'] = sum_e val[e] * x[n, k_e, (d_e + s j') mod nlon_in],   e in [row_ptr[r], row_ptr[r + 1]),
//   r = p * nlat_out + k',  idx[e] = k_e * nlon_in + d_e sorted within a row.
// The outer loop is the K basis rows p.  An LDS row is one input row, nlon_in words, staged by a straight copy; the
// items of a plane are the nlon_out output longitudes j' at offset s j'; the store is y[n, p, k', j'].
//
// Transposed (TR = true, the upsampling half), s = nlon_out / nlon_in:
//   y[n, k, s t + rho] = sum_e val[e] * z[n, p_e, k'_e, (d_e + t) mod nlon_in] (+ bias[n mod C]),   0 <= t < nlon_in,
//   r = k * s + rho,  idx[e] = (k'_e * K + p_e) * nlon_in + d_e sorted within a row (k'-major).
// The outer loop is the s phases rho.  An LDS row is the K basis planes of one input latitude, K * nlon_in words,
// staged from the [p, k', j'] layout of z into the image [k' - lo][p][nlon_in]; the items of a plane are the nlon_in
// coarse longitudes t at offset t; the store adds the bias in fp32 and writes y[n, k, s t + rho], element stores at
// stride s (consecutive lanes are consecutive t).
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

// A kernel argument that only the transposed direction has.  In the forward instances it takes no bytes, so each
// direction's argument block, and with it the scalar loads and the register allocation of the whole kernel, is what
// it is without the other direction (a trailing or a dead member moved either one by 1 - 4 % when measured).
template <class T, bool TR>
struct TrOnly {
  T v;
};
template <class T>
struct TrOnly<T, false> {};

template <bool TR>
struct Args {
  const void* x;  // x, or z in the transposed direction
  const int32_t* row_ptr;
  const int32_t* idx;
  const float* val;
  [[no_unique_address]] TrOnly<const float*, TR> bias;
  void* y;
  int64_t planes;
  [[no_unique_address]] TrOnly<int64_t, TR> C;
  int nlat_in, nlon_in, K, nlat_out, nlon_out, s, nnz, rows, ptiles;
};

// input latitudes [c0, c1) of the workgroup's planes -> lds[pl][k' - c0][LDS row] as fp32; planes past the end are
// not staged (no lane reads them).  Forward: the rows are contiguous in x.  Transposed: LDS word
// i = ((k' - c0) K + p) nlon_in + j comes from z[p, k', j]: a thread splits its first word once and then steps
// (k', p, j) by the split of kNT, no division in the loop.
template <bool BF, int PT, bool TR>
__device__ __forceinline__ void stage(const Args<TR>& a, float* lds, int64_t plane0, int c0, int c1, int plane_stride) {
  const int W = a.nlon_in, K = a.K;
  if constexpr (!TR) {
    const int n = (c1 - c0) * W;
    const int64_t pin = static_cast<int64_t>(a.nlat_in) * W;
#pragma unroll
    for (int pl = 0; pl < PT; ++pl) {
      if (plane0 + pl >= a.planes) break;
      const int64_t g0 = (plane0 + pl) * pin + static_cast<int64_t>(c0) * W;
      float* d = lds + pl * plane_stride;
      if constexpr (BF) {
        const uint16_t* xb = static_cast<const uint16_t*>(a.x) + g0;
#pragma unroll 4
        for (int i = threadIdx.x; i < n; i += kNT) d[i] = bf2f(xb[i]);
      } else {
        const float* xf = static_cast<const float*>(a.x) + g0;
#pragma unroll 4
        for (int i = threadIdx.x; i < n; i += kNT) d[i] = xf[i];
      }
    }
  } else {
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
        if constexpr (BF) d[i] = bf2f(static_cast<const uint16_t*>(a.x)[g0 + src]);
        else d[i] = static_cast<const float*>(a.x)[g0 + src];
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
}

// Entries [e, e1) with idx < lim, in table order; base = c0 * (LDS row) is LDS word 0 of a plane.  Returns the entry
// it stopped at.  lane[r]: the lane's LDS offset pl * plane_stride + o of item r, o its input longitude offset;
// thr[r] = nlon_in - o.
template <int RA, bool TR>
__device__ __forceinline__ int walk(const Args<TR>& a, const float* lds, int e, int e1, int base, int lim,
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

template <bool BF, int PT, bool TR>
__global__ void __launch_bounds__(kNT) disco_kernel(const Args<TR> a) {
  extern __shared__ __attribute__((aligned(16))) float disco_lds[];
  // heavy rows first: latitudes from both poles inwards, the plane tiles of one latitude together
  const int lin = blockIdx.x / a.ptiles;
  const int ko = (lin & 1) ? a.nlat_out - 1 - (lin >> 1) : (lin >> 1);
  const int64_t plane0 = static_cast<int64_t>(blockIdx.x % a.ptiles) * PT;
  const int W = a.nlon_in;
  const int RW = TR ? a.K * W : W;          // words of an LDS row
  const int nouter = TR ? a.s : a.K;        // CSR rows of this latitude: phases rho, or basis rows p
  const int nj = TR ? W : a.nlon_out;       // items of a plane
  const int sj = TR ? 1 : a.s;              // their stride along the input longitude
  const int plane_stride = a.rows * RW;
  const int nitems = PT * nj;

  auto row_range = [&](int o, int& e0, int& e1) {
    const int r = TR ? ko * a.s + o : o * a.nlat_out + ko;
    e0 = min(max(uni(a.row_ptr[r]), 0), a.nnz);
    e1 = min(max(uni(a.row_ptr[r + 1]), e0), a.nnz);
  };
  auto band = [&](int e0, int e1, int& lo, int& hi) {  // input latitudes of a non-empty entry range
    lo = min(max(uni(a.idx[e0]) / RW, 0), a.nlat_in - 1);
    hi = min(max(uni(a.idx[e1 - 1]) / RW, lo), a.nlat_in - 1);
  };

  int klo = a.nlat_in, khi = -1;
  for (int o = 0; o < nouter; ++o) {
    int e0, e1;
    row_range(o, e0, e1);
    if (e1 > e0) {
      int lo, hi;
      band(e0, e1, lo, hi);
      klo = min(klo, lo);
      khi = max(khi, hi);
    }
  }
  const bool single = khi - klo + 1 <= a.rows;  // also when every row is empty
  if (single && khi >= klo) {
    stage<BF, PT, TR>(a, disco_lds, plane0, klo, khi + 1, plane_stride);
    __syncthreads();
  }

  for (int o = 0; o < nouter; ++o) {
    int e0, e1;
    row_range(o, e0, e1);
    int plo = klo, phi = khi;
    if (!single && e1 > e0) band(e0, e1, plo, phi);
    if (e1 <= e0) phi = plo - 1;
    for (int item0 = 0; item0 < nitems; item0 += kNT * kR) {
      int lane[kR], thr[kR], jo[kR], pls[kR];
      bool ok[kR];
      float acc[kR];
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        int item = item0 + r * kNT + static_cast<int>(threadIdx.x);
        int pl = item / nj;
        ok[r] = item < nitems && plane0 + pl < a.planes;
        if (!ok[r]) {  // an idle lane follows item 0: plane0 is always there
          item = 0;
          pl = 0;
        }
        const int j = item - pl * nj;
        jo[r] = j;
        pls[r] = pl;
        lane[r] = pl * plane_stride + sj * j;
        thr[r] = W - sj * j;
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
          stage<BF, PT, TR>(a, disco_lds, plane0, c0, c1, plane_stride);
          __syncthreads();
        }
        const int base = c0 * RW, lim = c1 * RW;  // a single band: c0 = klo, c1 = khi + 1
        if (!busy) continue;
        if (ra == 1) e = walk<1>(a, disco_lds, e, e1, base, lim, lane, thr, acc);
        else if (ra == 2) e = walk<2>(a, disco_lds, e, e1, base, lim, lane, thr, acc);
        else e = walk<kR>(a, disco_lds, e, e1, base, lim, lane, thr, acc);
        if (single) break;
      }
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        if (!ok[r]) continue;
        const int64_t n = plane0 + pls[r];
        int64_t out;
        float v = acc[r];
        if constexpr (TR) {
          out = (n * a.nlat_out + ko) * a.nlon_out + static_cast<int64_t>(a.s) * jo[r] + o;
          if (a.bias.v) v += a.bias.v[n % a.C.v];
        } else {
          out = ((n * a.K + o) * a.nlat_out + ko) * a.nlon_out + jo[r];
        }
        if constexpr (BF) static_cast<uint16_t*>(a.y)[out] = f2bf(v);
        else static_cast<float*>(a.y)[out] = v;
      }
    }
  }
}

template <bool BF, int PT, bool TR>
void launch(const Args<TR>& a, const DiscoRoute& r, hipStream_t st) {
  hipLaunchKernelGGL((disco_kernel<BF, PT, TR>), dim3(static_cast<uint32_t>(r.wgs)), dim3(kNT),
                     static_cast<size_t>(r.lds), st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string(TR ? "amd_dft: disco_t: launch: " : "amd_dft: disco: launch: ") +
                             hipGetErrorString(e));
}

// fills the direction's arguments and picks the (dtype, PT) instance of the route
template <bool TR>
void run(const DiscoLaunch& p, const DiscoRoute& r, hipStream_t st) {
  Args<TR> a;
  a.x = p.x;
  a.row_ptr = p.row_ptr;
  a.idx = p.idx;
  a.val = p.val;
  a.y = p.y;
  a.planes = p.planes;
  if constexpr (TR) {
    a.bias.v = p.bias;
    a.C.v = p.C;
  }
  a.nlat_in = p.nlat_in;
  a.nlon_in = p.nlon_in;
  a.K = p.K;
  a.nlat_out = p.nlat_out;
  a.nlon_out = p.nlon_out;
  a.s = TR ? p.nlon_out / p.nlon_in : p.nlon_in / p.nlon_out;
  a.nnz = static_cast<int>(p.nnz);
  a.rows = r.rows;
  a.ptiles = static_cast<int>(r.ptiles);
  if (p.bf16) {
    if (r.pt == 4) launch<true, 4, TR>(a, r, st);
    else launch<true, 1, TR>(a, r, st);
  } else {
    if (r.pt == 4) launch<false, 4, TR>(a, r, st);
    else launch<false, 1, TR>(a, r, st);
  }
}

}  // namespace

void launch_disco(const DiscoLaunch& p, void* stream) {
  const bool tr = p.transposed != 0;
  const std::string op = tr ? "amd_dft: disco_t" : "amd_dft: disco";
  constexpr int64_t k2p31 = int64_t(1) << 31;
  if (p.planes <= 0 || p.nlat_out <= 0 || p.nlon_out <= 0 || (!tr && p.K <= 0)) return;
  bool bad = p.nlat_in < 1 || p.nlon_in < 1 || p.nnz < 0 || p.nnz >= k2p31;
  if (tr)
    bad = bad || p.K < 1 || p.C < 1 || p.nlon_out % p.nlon_in != 0 ||
          static_cast<int64_t>(p.K) * p.nlat_in * p.nlon_in >= k2p31 ||
          static_cast<int64_t>(p.nlat_out) * (p.nlon_out / p.nlon_in) >= k2p31 - 1;
  else
    bad = bad || p.nlon_in % p.nlon_out != 0 || static_cast<int64_t>(p.nlat_in) * p.nlon_in >= k2p31 ||
          static_cast<int64_t>(p.K) * p.nlat_out >= k2p31 - 1;
  if (bad)
    throw std::invalid_argument(op + (tr ? ": bad launch (nlon_out % nlon_in, sizes below 2^31)"
                                         : ": bad launch (nlon_in % nlon_out, sizes below 2^31)"));
  const DiscoRoute r =
      disco_route(tr, p.planes, p.nlat_in, p.nlon_in, p.K, p.nlat_out, p.nlon_out, p.nnz, p.bf16 != 0);
  if (r.lds > kDiscoLdsBytes)
    throw std::invalid_argument(op + (tr ? ": the K basis planes of an input latitude do not fit the LDS chunk"
                                         : ": an input row does not fit the LDS chunk"));
  const int64_t items = tr ? p.nlon_in : p.nlon_out;  // per plane
  if (r.wgs >= k2p31 || 4 * items >= k2p31) throw std::invalid_argument(op + ": too many workgroups");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (tr) run<true>(p, r, st);
  else run<false>(p, r, st);
}

}  // namespace amd_dft

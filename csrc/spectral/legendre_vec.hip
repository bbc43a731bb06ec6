// Vector Legendre transform along latitude, per longitudinal mode, on MFMA -- the latitude half of a vector
// spherical harmonic transform (spheroidal / toroidal coefficients of a tangential vector field and back):
//   y[n, 0, r, m] = sum_q A[m, r, q] x[n, 0, q, m] - i B[m, r, q] x[n, 1, q, m]
//   y[n, 1, r, m] = sum_q A[m, r, q] x[n, 1, q, m] + i B[m, r, q] x[n, 0, q, m]
// x [N, 2, Q, M, 2] (complex as trailing re/im), A, B [M, R, Q] real, y [N, 2, R, M, 2].  Forward: Q = nlat,
// R = lmax, (A, B) = w_k (dPb/dtheta, m Pb / sin theta) / (l (l + 1)); inverse: Q = lmax, R = nlat, (A, B) the two
// derivative tables transposed.  One kernel serves both.
//
// This is legendre.hip's kernel (same precision, table format, tiling, staging, tri and edge rules: read its
// header) run over the 2 N component planes of x, [2 N, Q, M, 2], with one addition.  A 16-column MFMA tile holds
// 4 fields: column = 4 n + 2 component + (re | im).  In that order the operand of B, the other component
// rotated by -i (component 0: (re, im) <- (im, -re) of x1) or +i (component 1: (re, im) <- (-im, re) of x0), is
// the SAME tile with its columns permuted, column c <- column c ^ 3, negated where c & 3 is 1 or 2.  So the slab
// image is staged once, as legendre does; a lane reads its plain fragment at column c and its rotated fragment at
// column c ^ 3 (the same 16 columns in another order: as conflict-free as the plain read), flips the sign bits
// of the bf16 values (exact, in both planes of the split), and
//   acc[tile] += A . plain + B . rotated
// lands both components of y in one accumulator tile.  Every A fragment is fetched once per slab and feeds
// A.x0 -> y0 and A.x1 -> y1 of every tile, every B fragment B.rot(x1) -> y0 and B.rot'(x0) -> y1; the output goes
// through legendre's LDS image unchanged, since y is [2 N, R, M, 2].
//   The alternative -- separate accumulators for B.x0 and B.x1, rotated in the output image -- would double the
//   accumulators (128 VGPRs at 8 modes x 8 fields); rotated copies staged beside the plain ones would double the
//   slab image.  The permuted read costs one more 16-byte LDS read and 4 v_xor per fragment and plane instead.
// Accumulators: MW x 4 row tiles x CT column tiles x 4 registers, one set (the components share it): 64 at
// MT = 8, CT = 2; 32 at 8 x 1 and 4 x 2; 16 at 4 x 1.  LDS per workgroup is legendre_lds_bytes.
// Shipped instances (VGPRs + AGPRs as compiled -> waves per SIMD; LDS bytes):
//   fp32  4 x 2: 158 + 32 -> 2, 20992 B    4 x 1: 134 + 16 -> 3, 10752 B
//   bf16  8 x 2: 173 + 64 -> 2, 20736 B    8 x 1: 136 + 32 -> 3, 10496 B    4 x 2: 102 + 32 -> 3, 10496 B
//         4 x 1:  90 + 16 -> 4,  5376 B
// fp32 has no 8-mode instance: two modes per wave hold 4 planes x 2 tables x 4 row tiles of fragments, 128
// registers, and the 8 x 2 kernel compiles to 256 + 76 registers, one wave per SIMD (8 x 1: 216 + 32, no better
// than 4 x 2, which reads each table half as often).
//   tri applies to both tables (1: rows r < m are zero; 2: columns q < m are zero and x[q < m] is not read).
//   The m = 0 plane of B is zero in a vector SHT, but the op takes any table, so it is multiplied like the rest.
// No atomics: bit-reproducible run to run.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "spectral.h"

namespace amd_dft {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// two floats -> packed bf16x2 (v_cvt_pk_bf16_f32, round-to-nearest-even)
__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  bf16x2 v;
  v[0] = static_cast<__bf16>(a);
  v[1] = static_cast<__bf16>(b);
  return __builtin_bit_cast(uint32_t, v);
}
// hi = bf16(a, b); lo = bf16(a - hi.a, b - hi.b)
__device__ __forceinline__ void split_pk(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = pk_bf16(a, b);
  lo = pk_bf16(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}
// 8 bf16 with their sign bits flipped where sgn = 0x80008000 (sgn = 0: as they are)
__device__ __forceinline__ bf16x8 flip(uint4 v, uint32_t sgn) {
  v.x ^= sgn;
  v.y ^= sgn;
  v.z ^= sgn;
  v.w ^= sgn;
  return __builtin_bit_cast(bf16x8, v);
}

// x and y are the 2 N component planes: N2 = 2 N "fields" of legendre.hip
template <int CT, int MW, bool BF>
__global__ void __launch_bounds__(256)
    legendre_vec_kernel(const void* __restrict__ x, const uint16_t* __restrict__ ath, const uint16_t* __restrict__ atl,
                        const uint16_t* __restrict__ bth, const uint16_t* __restrict__ btl, void* __restrict__ y,
                        int64_t N2, int Q, int R, int M, int Rp, int Qp, int tri) {
  constexpr int MT = 4 * MW;                       // modes per workgroup
  constexpr int NT = 8 * CT;                       // component planes per workgroup (4 CT fields)
  constexpr int NC = 16 * CT;                      // real columns per workgroup
  constexpr int RT = kLegRowTiles;
  constexpr int MLS = NC * kLegXPitch + 256 / MT;  // bytes per mode of a slab plane
  constexpr int PLANE = MT * MLS;                  // bytes per plane (hi, lo)
  constexpr int XI = NT * MT / 16;                 // staged (n, q pair, mode) items per thread and slab
  constexpr int YP = 2 * MT + 2;                   // floats per (r, n) row of the output image
  constexpr int YR = NT * YP + 4;                  // floats per r of the output image
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int m0 = blockIdx.x * MT;
  const int64_t n0 = static_cast<int64_t>(blockIdx.y) * NT;
  const int r0 = blockIdx.z * 16 * RT;
  const float2* x2 = reinterpret_cast<const float2*>(x);      // fp32: one (re, im) pair
  const uint32_t* xb2 = reinterpret_cast<const uint32_t*>(x);  // bf16: one (re, im) pair
  // the rotated operand of this lane's column: column l15 ^ 3, negated where (l15 & 3) is 1 or 2
  const int lrot = l15 ^ 3;
  const uint32_t sgn = ((l15 ^ (l15 >> 1)) & 1) ? 0x80008000u : 0u;

  const int nslab = (Q + kLegSlab - 1) / kLegSlab;
  // tri = 2: all columns q < m0 are zero for every mode here; tri = 1: a row group below m0 is all zero
  int s0 = tri == 2 ? m0 / kLegSlab : 0;
  if (tri == 1 && r0 + 16 * RT <= m0) s0 = nslab;

  // which (mode, row tile) pairs of this wave are live (wave-uniform)
  bool live[MW][RT];
#pragma unroll
  for (int j = 0; j < MW; ++j) {
    const int m = m0 + wv * MW + j;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int rg = r0 + 16 * rt;
      live[j][rt] = m < M && rg < R && !(tri == 1 && rg + 15 < m);
    }
  }

  float xr[BF ? 1 : XI][4];      // fp32: (re, im) of q and q + 1
  uint32_t xb[BF ? XI : 1][2];   // bf16: the packed (re, im) of q and of q + 1
  auto load_slab = [&](int s) {
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int idx = tid + 256 * i;
      const int ml = idx % MT, qp = (idx / MT) & 15, nl = idx / (MT * 16);
      const int m = m0 + ml, q = s * kLegSlab + 2 * qp;
      const int64_t n = n0 + nl;
      if constexpr (BF) {
        uint32_t a = 0u, b = 0u;
        if (m < M && n < N2) {
          const uint32_t* src = xb2 + ((n * Q + q) * M + m);
          const int qmin = tri == 2 ? m : 0;
          if (q < Q && q >= qmin) a = src[0];
          if (q + 1 < Q && q + 1 >= qmin) b = src[M];
        }
        xb[i][0] = a;
        xb[i][1] = b;
      } else {
        float2 a = make_float2(0.f, 0.f), b = a;
        if (m < M && n < N2) {
          const float2* src = x2 + ((n * Q + q) * M + m);
          const int qmin = tri == 2 ? m : 0;
          if (q < Q && q >= qmin) a = src[0];
          if (q + 1 < Q && q + 1 >= qmin) b = src[M];
        }
        xr[i][0] = a.x;
        xr[i][1] = a.y;
        xr[i][2] = b.x;
        xr[i][3] = b.y;
      }
    }
  };

  f32x4 acc[MW][RT][CT];
#pragma unroll
  for (int j = 0; j < MW; ++j)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[j][rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (s0 < nslab) load_slab(s0);
  for (int s = s0; s < nslab; ++s) {
    // ---- this slab's fragments of both tables (global, both planes): lane = T[m][rg + l15][32 s + 8 lq + 0..7]
    uint4 ah[MW][RT], al[BF ? 1 : MW][BF ? 1 : RT], bh[MW][RT], bl[BF ? 1 : MW][BF ? 1 : RT];
#pragma unroll
    for (int j = 0; j < MW; ++j) {
      const int m = m0 + wv * MW + j;
      const bool mode_live = !(tri == 2 && s * kLegSlab + kLegSlab - 1 < m);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        if (live[j][rt] && mode_live) {
          const int64_t off = (static_cast<int64_t>(m) * Rp + r0 + 16 * rt + l15) * Qp + s * kLegSlab + 8 * lq;
          ah[j][rt] = *reinterpret_cast<const uint4*>(ath + off);
          bh[j][rt] = *reinterpret_cast<const uint4*>(bth + off);
          if constexpr (!BF) {
            al[j][rt] = *reinterpret_cast<const uint4*>(atl + off);
            bl[j][rt] = *reinterpret_cast<const uint4*>(btl + off);
          }
        }
      }
    }
    __syncthreads();  // every wave is done reading the previous slab
    // ---- the slab image: x split into bf16 (hi, lo) (bf16: as it is), q pairs packed, zeros outside x
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int idx = tid + 256 * i;
      const int ml = idx % MT, qp = (idx / MT) & 15, nl = idx / (MT * 16);
      char* dst = smem + ml * MLS + 2 * nl * kLegXPitch + 4 * qp;
      if constexpr (BF) {
        const uint32_t a = xb[i][0], b = xb[i][1];  // (re | im << 16) of q and of q + 1
        *reinterpret_cast<uint32_t*>(dst) = (a & 0xffffu) | (b << 16);
        *reinterpret_cast<uint32_t*>(dst + kLegXPitch) = (a >> 16) | (b & 0xffff0000u);
      } else {
        uint32_t hr, lr, hi, li;
        split_pk(xr[i][0], xr[i][2], hr, lr);
        split_pk(xr[i][1], xr[i][3], hi, li);
        *reinterpret_cast<uint32_t*>(dst) = hr;
        *reinterpret_cast<uint32_t*>(dst + kLegXPitch) = hi;
        *reinterpret_cast<uint32_t*>(dst + PLANE) = lr;
        *reinterpret_cast<uint32_t*>(dst + PLANE + kLegXPitch) = li;
      }
    }
    __syncthreads();
    // ---- the next slab's global loads, in flight during the MFMAs
    if (s + 1 < nslab) load_slab(s + 1);
    // ---- MFMAs: live (mode, row tile) pairs only; per column tile the plain fragment (for A) and the rotated one
    // (for B): the other component's columns of the same tile, signs flipped where the rotation negates
#pragma unroll
    for (int j = 0; j < MW; ++j) {
      const int ml = wv * MW + j;
      const bool mode_live = !(tri == 2 && s * kLegSlab + kLegSlab - 1 < m0 + ml);
      if (!mode_live) continue;
      bf16x8 ph[CT], pl[BF ? 1 : CT], rh[CT], rl[BF ? 1 : CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const char* src = smem + ml * MLS + (16 * ct + l15) * kLegXPitch + 16 * lq;
        const char* rot = smem + ml * MLS + (16 * ct + lrot) * kLegXPitch + 16 * lq;
        ph[ct] = *reinterpret_cast<const bf16x8*>(src);
        rh[ct] = flip(*reinterpret_cast<const uint4*>(rot), sgn);
        if constexpr (!BF) {
          pl[ct] = *reinterpret_cast<const bf16x8*>(src + PLANE);
          rl[ct] = flip(*reinterpret_cast<const uint4*>(rot + PLANE), sgn);
        }
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        if (live[j][rt]) {
          const bf16x8 Ah = __builtin_bit_cast(bf16x8, ah[j][rt]);
          const bf16x8 Bh = __builtin_bit_cast(bf16x8, bh[j][rt]);
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            acc[j][rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, ph[ct], acc[j][rt][ct], 0, 0, 0);
            acc[j][rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Bh, rh[ct], acc[j][rt][ct], 0, 0, 0);
            if constexpr (!BF) {
              const bf16x8 Al = __builtin_bit_cast(bf16x8, al[j][rt]);
              const bf16x8 Bl = __builtin_bit_cast(bf16x8, bl[j][rt]);
              acc[j][rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, ph[ct], acc[j][rt][ct], 0, 0, 0);
              acc[j][rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Bl, rh[ct], acc[j][rt][ct], 0, 0, 0);
              acc[j][rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, pl[ct], acc[j][rt][ct], 0, 0, 0);
              acc[j][rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Bh, rl[ct], acc[j][rt][ct], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  // ---- store, one 16-row tile at a time through LDS: image [r][n][mode][re | im], so a thread writes one
  // mode's (re, im) and consecutive threads consecutive modes of one (n, r) row of y
  float* ys = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int rg0 = r0 + 16 * rt;
    if (rg0 >= R) break;  // block-uniform
    __syncthreads();      // the slab image (rt = 0) or the previous tile's image has been read
#pragma unroll
    for (int j = 0; j < MW; ++j) {
      const int ml = wv * MW + j;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int col = 16 * ct + l15;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          ys[(4 * lq + i) * YR + (col >> 1) * YP + 2 * ml + (col & 1)] = acc[j][rt][ct][i];
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int idx = tid + 256 * i;
      const int ml = idx % MT, r = (idx / MT) & 15, nl = idx / (MT * 16);
      const int m = m0 + ml, rg = rg0 + r;
      const int64_t n = n0 + nl;
      if (m < M && rg < R && n < N2) {
        float2 v = *reinterpret_cast<const float2*>(ys + r * YR + nl * YP + 2 * ml);
        if (tri == 1 && rg < m) v = make_float2(0.f, 0.f);
        if constexpr (BF) reinterpret_cast<uint32_t*>(y)[(n * R + rg) * M + m] = pk_bf16(v.x, v.y);
        else reinterpret_cast<float2*>(y)[(n * R + rg) * M + m] = v;
      }
    }
  }
}

template <int CT, int MW, bool BF>
void launch_prec(const LegendreVecLaunch& p, const LegendreRoute& r, hipStream_t st) {
  const dim3 grid(r.mgroups, r.ctiles, r.rgroups);
  hipLaunchKernelGGL((legendre_vec_kernel<CT, MW, BF>), grid, dim3(256), static_cast<size_t>(r.lds), st, p.x, p.ah,
                     p.al, p.bh, p.bl, p.y, 2 * p.N, p.Q, p.R, p.M, r.rtiles * 16, r.slabs * kLegSlab, p.tri);
}
}  // namespace

void launch_legendre_vec(const LegendreVecLaunch& p, void* stream) {
  if (p.N == 0 || p.R == 0 || p.M == 0) return;
  if (p.Q < 1) throw std::runtime_error("amd_dft: legendre_vec: Q must be >= 1");
  if (p.tri < 0 || p.tri > 2) throw std::runtime_error("amd_dft: legendre_vec: tri must be 0, 1 or 2");
  const LegendreRoute r = legendre_vec_route(p.Q, p.R, p.M, 4 * p.N, p.tri, p.bf16 != 0);
  if (r.ctiles > 65535 || r.rgroups > 65535) throw std::runtime_error("amd_dft: legendre_vec: tensor too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  // fp32 has no 8-mode instances (legendre_vec_route): four planes of table fragments for two modes per wave
  // leave one wave per SIMD
  if (r.mt == 8 && !p.bf16) throw std::runtime_error("amd_dft: legendre_vec: no fp32 instance with 8 modes");
  if (r.mt == 8) {
    if (r.ct == 2) launch_prec<2, 2, true>(p, r, st);
    else launch_prec<1, 2, true>(p, r, st);
  } else if (p.bf16) {
    if (r.ct == 2) launch_prec<2, 1, true>(p, r, st);
    else launch_prec<1, 1, true>(p, r, st);
  } else {
    if (r.ct == 2) launch_prec<2, 1, false>(p, r, st);
    else launch_prec<1, 1, false>(p, r, st);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: legendre_vec launch: ") + hipGetErrorString(e));
}

}  // namespace amd_dft

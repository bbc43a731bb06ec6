// Legendre transform along latitude, per longitudinal mode, on MFMA -- the second half of a spherical
// harmonic transform (the first is the truncated real FFT along longitude, csrc/fft):
//   y[n, r, m, :] = sum_q T[m, r, q] * x[n, q, m, :]
// x [N, Q, M, 2] fp32 (complex as trailing re/im), T [M, R, Q] real, y [N, R, M, 2] fp32; n runs over
// batch x channels.  Forward: Q = nlat, R = lmax, T = w_k P_l^m(cos theta_k); inverse: Q = lmax, R = nlat,
// T = P transposed.  One kernel serves both.
//
// Precision: the project's bf16x3 form, A.B = Ah.Bh + Al.Bh + Ah.Bl on v_mfma_f32_16x16x32_bf16 with fp32
// accumulation.  T arrives split on the host side as two bf16 planes (hi, lo), zero-padded to
// [M, Rp = ceil16(R), Qp = ceil32(Q)], so every A fragment is one aligned 16-byte global load that cannot
// leave the table; x is split as it is staged into LDS.
//
// GEMM orientation per mode m: C[r][col] with the 2 N real columns col = 2 n + (re | im).
//   A = T[m][r][q]: lane holds T[r0 + l15][q0 + 8 lq + 0..7] of both planes, straight from global memory
//       (waves own different modes, so a table element is read by one wave of the workgroup);
//   B = x[q][col]: from the LDS slab image [plane][mode][col][32 q] bf16, column pitch 80 B (16-byte reads
//       of 16 consecutive columns touch all 64 banks once), modes 256 / MT bytes further apart so the
//       staging stores of a wave (modes x q pairs) touch 64 different banks.
// A workgroup (4 waves) owns MT = 4 MW consecutive modes (wave w: modes m0 + w MW + 0..MW-1), NT = 8 CT
// fields n (CT 16-column tiles) and one group of 4 row tiles (64 rows r; grid z walks the groups), and loops
// over Q in 32-deep slabs.  Global reads of x: every (n, q) row is one contiguous run of 8 MT bytes; global
// writes of y go through LDS one 16-row tile at a time so every (n, r) row is one contiguous run of 8 MT bytes.
//   Edges: q >= Q, n >= N and m >= M are WRITTEN as zeros into the slab image (the padded table is zero
//   there too, but 0 * stale-NaN is NaN); nothing is loaded or stored outside x, the padded table or y.
//   The mode count M is a run-time value without a limit.
//   tri = 1 (rows r < m of T are zero, the forward transform): 16-row tiles entirely below m issue no table
//   loads and no MFMAs, a row group entirely below the workgroup's first mode reads nothing at all, and
//   rows r < m are stored as exact zeros.  tri = 2 (columns q < m are zero, the inverse transform): slabs
//   entirely below the workgroup's first mode are skipped, a wave skips the slabs below its own mode, and
//   x[q < m] is staged as zero.  Either way the result is the dense product with that part of T zero.
// The next slab's x values are loaded into registers before the current slab's MFMAs; the table fragments
// of a slab are requested before the slab is written to LDS.  No atomics: bit-reproducible run to run.
//
// bf16 instances (BF): x and y are bf16, T is the one plane bf16(T) (the hi plane alone), so a fragment pair is one
// MFMA instead of three; accumulation stays fp32 and the result is rounded once, at the store.  A (re, im) pair is
// one 4-byte load or store (global rows are runs of 4 MT bytes), staging packs the q pairs of the bf16 values as
// they are, and the slab image is the one plane.  Tiling, tri, the edge zeros and the prefetch are the same code.
//
// LDS per workgroup (legendre_lds_bytes): 41472 B at MT = 8, CT = 2; 20992 B at 4 x 2; 10752 B at 4 x 1
// (bf16: 20736, 10496, 5376).
//
// Vector instances (VEC) -- the latitude half of a vector spherical harmonic transform (spheroidal / toroidal
// coefficients of a tangential vector field and back):
//   y[n, 0, r, m] = sum_q A[m, r, q] x[n, 0, q, m] - i B[m, r, q] x[n, 1, q, m]
//   y[n, 1, r, m] = sum_q A[m, r, q] x[n, 1, q, m] + i B[m, r, q] x[n, 0, q, m]
// x [N, 2, Q, M, 2], A, B [M, R, Q] real, y [N, 2, R, M, 2].  Forward: Q = nlat, R = lmax, (A, B) = w_k
// (dPb/dtheta, m Pb / sin theta) / (l (l + 1)); inverse: Q = lmax, R = nlat, (A, B) the two derivative tables
// transposed.
// This is the kernel above (same precision, table format, tiling, staging, tri and edge rules) run over the 2 N
// component planes of x, [2 N, Q, M, 2], with one addition.  A 16-column MFMA tile holds 4 fields: column =
// 4 n + 2 component + (re | im).  In that order the operand of B, the other component rotated by -i (component 0:
// (re, im) <- (im, -re) of x1) or +i (component 1: (re, im) <- (-im, re) of x0), is the SAME tile with its columns
// permuted, column c <- column c ^ 3, negated where c & 3 is 1 or 2.  So the slab image is staged once; a lane
// reads its plain fragment at column c and its rotated fragment at column c ^ 3 (the same 16 columns in another
// order: as conflict-free as the plain read), flips the sign bits of the bf16 values (exact, in both planes of the
// split), and
//   acc[tile] += A . plain + B . rotated
// lands both components of y in one accumulator tile.  Every A fragment is fetched once per slab and feeds
// A.x0 -> y0 and A.x1 -> y1 of every tile, every B fragment B.rot(x1) -> y0 and B.rot'(x0) -> y1; the output goes
// through the LDS image unchanged, since y is [2 N, R, M, 2].
//   The alternative -- separate accumulators for B.x0 and B.x1, rotated in the output image -- would double the
//   accumulators (128 VGPRs at 8 modes x 8 fields); rotated copies staged beside the plain ones would double the
//   slab image.  The permuted read costs one more 16-byte LDS read and 4 v_xor per fragment and plane instead.
// Accumulators: MW x 4 row tiles x CT column tiles x 4 registers, one set (the components share it): 64 at
// MT = 8, CT = 2; 32 at 8 x 1 and 4 x 2; 16 at 4 x 1.
// Shipped vector instances (VGPRs + AGPRs as compiled -> waves per SIMD; LDS bytes):
//   fp32  4 x 2: 158 + 32 -> 2, 20992 B    4 x 1: 134 + 16 -> 3, 10752 B
//   bf16  8 x 2: 173 + 64 -> 2, 20736 B    8 x 1: 136 + 32 -> 3, 10496 B    4 x 2: 102 + 32 -> 3, 10496 B
//         4 x 1:  90 + 16 -> 4,  5376 B
// fp32 has no 8-mode vector instance: two modes per wave hold 4 planes x 2 tables x 4 row tiles of fragments, 128
// registers, and the 8 x 2 kernel compiles to 256 + 76 registers, one wave per SIMD (8 x 1: 216 + 32, no better
// than 4 x 2, which reads each table half as often).
//   tri applies to both tables (1: rows r < m are zero; 2: columns q < m are zero and x[q < m] is not read).
//   The m = 0 plane of B is zero in a vector SHT, but the op takes any table, so it is multiplied like the rest.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "../nn/bf16_pack.h"
#include "spectral.h"

namespace amd_dft {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// 8 bf16 with their sign bits flipped where sgn = 0x80008000 (sgn = 0: as they are)
__device__ __forceinline__ bf16x8 flip(uint4 v, uint32_t sgn) {
  v.x ^= sgn;
  v.y ^= sgn;
  v.z ^= sgn;
  v.w ^= sgn;
  return __builtin_bit_cast(bf16x8, v);
}

// N counts the [Q, M, 2] planes of x and y (VEC: the 2 x fields component planes); bth, btl are read only if VEC
template <int CT, int MW, bool BF, bool VEC>
__global__ void __launch_bounds__(256)
    legendre_kernel(const void* __restrict__ x, const uint16_t* __restrict__ ath, const uint16_t* __restrict__ atl,
                    const uint16_t* __restrict__ bth, const uint16_t* __restrict__ btl, void* __restrict__ y,
                    int64_t N, int Q, int R, int M, int Rp, int Qp, int tri) {
  constexpr int MT = 4 * MW;                       // modes per workgroup
  constexpr int NT = 8 * CT;                       // fields n per workgroup
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
  // VEC: the rotated operand of this lane's column: column l15 ^ 3, negated where (l15 & 3) is 1 or 2
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
        if (m < M && n < N) {
          const uint32_t* src = xb2 + ((n * Q + q) * M + m);
          const int qmin = tri == 2 ? m : 0;
          if (q < Q && q >= qmin) a = src[0];
          if (q + 1 < Q && q + 1 >= qmin) b = src[M];
        }
        xb[i][0] = a;
        xb[i][1] = b;
      } else {
        float2 a = make_float2(0.f, 0.f), b = a;
        if (m < M && n < N) {
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
    // ---- this slab's table fragments (global, both planes, VEC: of both tables):
    // lane = T[m][rg + l15][32 s + 8 lq + 0..7]
    uint4 ah[MW][RT], al[BF ? 1 : MW][BF ? 1 : RT];
    uint4 bh[VEC ? MW : 1][VEC ? RT : 1], bl[VEC && !BF ? MW : 1][VEC && !BF ? RT : 1];
#pragma unroll
    for (int j = 0; j < MW; ++j) {
      const int m = m0 + wv * MW + j;
      const bool mode_live = !(tri == 2 && s * kLegSlab + kLegSlab - 1 < m);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        if (live[j][rt] && mode_live) {
          const int64_t off = (static_cast<int64_t>(m) * Rp + r0 + 16 * rt + l15) * Qp + s * kLegSlab + 8 * lq;
          ah[j][rt] = *reinterpret_cast<const uint4*>(ath + off);
          if constexpr (VEC) bh[j][rt] = *reinterpret_cast<const uint4*>(bth + off);
          if constexpr (!BF) {
            al[j][rt] = *reinterpret_cast<const uint4*>(atl + off);
            if constexpr (VEC) bl[j][rt] = *reinterpret_cast<const uint4*>(btl + off);
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
    // ---- MFMAs: live (mode, row tile) pairs only; per column tile the plain fragment (for A) and, VEC, the rotated
    // one (for B): the other component's columns of the same tile, signs flipped where the rotation negates
#pragma unroll
    for (int j = 0; j < MW; ++j) {
      const int ml = wv * MW + j;
      const bool mode_live = !(tri == 2 && s * kLegSlab + kLegSlab - 1 < m0 + ml);
      if (!mode_live) continue;
      bf16x8 ph[CT], pl[BF ? 1 : CT], rh[VEC ? CT : 1], rl[VEC && !BF ? CT : 1];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const char* src = smem + ml * MLS + (16 * ct + l15) * kLegXPitch + 16 * lq;
        const char* rot = smem + ml * MLS + (16 * ct + lrot) * kLegXPitch + 16 * lq;
        ph[ct] = *reinterpret_cast<const bf16x8*>(src);
        if constexpr (VEC) rh[ct] = flip(*reinterpret_cast<const uint4*>(rot), sgn);
        if constexpr (!BF) {
          pl[ct] = *reinterpret_cast<const bf16x8*>(src + PLANE);
          if constexpr (VEC) rl[ct] = flip(*reinterpret_cast<const uint4*>(rot + PLANE), sgn);
        }
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        if (live[j][rt]) {
          const bf16x8 Ah = __builtin_bit_cast(bf16x8, ah[j][rt]);
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            acc[j][rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, ph[ct], acc[j][rt][ct], 0, 0, 0);
            if constexpr (VEC) {
              const bf16x8 Bh = __builtin_bit_cast(bf16x8, bh[j][rt]);
              acc[j][rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Bh, rh[ct], acc[j][rt][ct], 0, 0, 0);
            }
            if constexpr (!BF) {
              const bf16x8 Al = __builtin_bit_cast(bf16x8, al[j][rt]);
              acc[j][rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, ph[ct], acc[j][rt][ct], 0, 0, 0);
              if constexpr (VEC) {
                const bf16x8 Bl = __builtin_bit_cast(bf16x8, bl[j][rt]);
                acc[j][rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Bl, rh[ct], acc[j][rt][ct], 0, 0, 0);
              }
              acc[j][rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, pl[ct], acc[j][rt][ct], 0, 0, 0);
              if constexpr (VEC) {
                const bf16x8 Bh = __builtin_bit_cast(bf16x8, bh[j][rt]);
                acc[j][rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Bh, rl[ct], acc[j][rt][ct], 0, 0, 0);
              }
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
      if (m < M && rg < R && n < N) {
        float2 v = *reinterpret_cast<const float2*>(ys + r * YR + nl * YP + 2 * ml);
        if (tri == 1 && rg < m) v = make_float2(0.f, 0.f);
        if constexpr (BF) reinterpret_cast<uint32_t*>(y)[(n * R + rg) * M + m] = pk_bf16(v.x, v.y);
        else reinterpret_cast<float2*>(y)[(n * R + rg) * M + m] = v;
      }
    }
  }
}

template <int CT, int MW, bool BF, bool VEC>
void launch_prec(const LegendreLaunch& p, const LegendreRoute& r, hipStream_t st) {
  const dim3 grid(r.mgroups, r.ctiles, r.rgroups);
  hipLaunchKernelGGL((legendre_kernel<CT, MW, BF, VEC>), grid, dim3(256), static_cast<size_t>(r.lds), st, p.x, p.th,
                     p.tl, p.bh, p.bl, p.y, p.N, p.Q, p.R, p.M, r.rtiles * 16, r.slabs * kLegSlab, p.tri);
}
// the 8 scalar and 6 vector instances: fp32 has no 8-mode vector kernel (one wave per SIMD, see the header;
// legendre_route does not pick it)
template <int CT, int MW, bool VEC>
void launch_inst(const LegendreLaunch& p, const LegendreRoute& r, hipStream_t st) {
  if (p.bf16) launch_prec<CT, MW, true, VEC>(p, r, st);
  else if constexpr (VEC && MW == 2) throw std::runtime_error("amd_dft: legendre_vec: no fp32 instance with 8 modes");
  else launch_prec<CT, MW, false, VEC>(p, r, st);
}

template <bool VEC>
void launch(const LegendreLaunch& p, void* stream) {
  const std::string op = VEC ? "amd_dft: legendre_vec" : "amd_dft: legendre";
  if (p.N == 0 || p.R == 0 || p.M == 0) return;
  if (p.Q < 1) throw std::runtime_error(op + ": Q must be >= 1");
  if (p.tri < 0 || p.tri > 2) throw std::runtime_error(op + ": tri must be 0, 1 or 2");
  const LegendreRoute r = legendre_route(p.Q, p.R, p.M, 2 * p.N, p.tri, p.bf16 != 0, VEC);
  if (r.ctiles > 65535 || r.rgroups > 65535) throw std::runtime_error(op + ": tensor too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (r.mt == 8) {
    if (r.ct == 2) launch_inst<2, 2, VEC>(p, r, st);
    else launch_inst<1, 2, VEC>(p, r, st);
  } else {
    if (r.ct == 2) launch_inst<2, 1, VEC>(p, r, st);
    else launch_inst<1, 1, VEC>(p, r, st);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(op + " launch: " + hipGetErrorString(e));
}

}  // namespace

void launch_legendre(const LegendreLaunch& p, void* stream) { launch<false>(p, stream); }
void launch_legendre_vec(const LegendreLaunch& p, void* stream) { launch<true>(p, stream); }

}  // namespace amd_dft

// amd_dft-build-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
// DISCO convolution on the sphere in the longitude-Fourier domain, on MFMA.  Every DISCO row is a circular
// correlation along longitude,
//   y[p, k', j'] = sum_{k, d} Psi[p, k', k, d] x[k, (d + s j') mod nlon_in],        s = nlon_in / nlon_out,
// so after an unnormalised R2C along longitude, Xh[k, mu], it is one small banded complex matrix per mode:
//   Yh[p, k', m'] = (1 / s) sum_{r < s} sum_k G[p, k', k, mu] Xh[k, mu],  mu = m' + r nlon_out,  0 <= m' < Mo,
//   G[p, k', k, mu] = conj(sum_d Psi[p, k', k, d] e^{-2 pi i mu d / nlon_in}),      0 <= mu < nlon_in,
// with Xh[k, mu] = conj(Xh[k, nlon_in - mu]) above the stored half spectrum; y = irfft(Yh, nlon_out).  The fold of s
// input modes onto one output mode is the subsampling to the coarse grid.  A polar row, whose filter support wraps
// the whole circle, costs exactly what an equatorial row costs: the band is U input latitudes either way.
//
// Xh [N, nlat_in, Mi, 2] fp32 (complex as trailing re/im), Yh [N, K, nlat_out, Mo, 2] fp32.  The table arrives
// packed on the host side (ops.disco.disco_spectral_tables): output latitudes in groups of R consecutive k', R the
// largest of 8, 4, 2, 1 with R K <= 16, so that a group's rows (k' - g R) K + p are the rows of ONE 16-row MFMA tile;
// group g reads the input latitudes lo[g] .. lo[g] + U - 1;
//   T[g, m', row, kappa],  kappa = 2 (r U + k - lo[g]) + c,  c = 0: Re G / s, c = 1: Im G / s,
// zero-padded to KD = ceil32(2 s U) and split into two bf16 planes (hi, lo), so every A fragment is one aligned
// 16-byte global load that cannot leave the table.
//
// Precision: the project's bf16x3 form, A.B = Ah.Bh + Al.Bh + Ah.Bl on v_mfma_f32_16x16x32_bf16 with fp32
// accumulation (as legendre.hip, sfno_mix.hip); Xh is split as it is staged into LDS.
//
// GEMM orientation per (group, mode): C[row][col] over the real columns col = 2 n + (re | im), contraction kappa:
//   A = T[g][m'][row][kappa]: lane holds T[l15][32 st + 8 lq + 0..7] of both planes, straight from global memory
//       (waves own different modes, so a table element is read by one wave of the workgroup);
//   B: the real column of plane n takes (Xr, -Xi) against (Re G, Im G), its imaginary column (Xi, Xr) -- the
//       interleaving of sfno_mix.  The LDS image holds each (re, im) ONCE, as one packed word per (mode, plane, j):
//       the lane of a real column flips the sign bit of the upper half of the word it read, the lane of an imaginary
//       column rotates it by 16 bits (both exact, in both planes of the split).  Rows are KD / 2 words + 16 bytes
//       apart: the 16-byte reads of the 8 planes of a column tile touch all 64 banks once, and the two lanes of a
//       plane read the same address.  Modes are PTL rows + 8 words apart (8 mod 64 words for either PTL), so the
//       staging stores of a wave, 8 modes x 8 consecutive j, touch 64 different banks.
// A workgroup (4 waves) owns one group g (grid z), MT = 4 MW consecutive output modes (grid x; wave w: modes w,
// w + 4, ...: a wave's MFMA chain needs no cross-wave reduction) and PTL = 8 CT planes (grid y).  The whole band
// of the tile goes through LDS once: for every fold r and band row the MT modes mu = m' + r nlon_out are one
// contiguous run of Xh, ascending below the Nyquist mode and descending (read at nlon_in - mu, conjugated) above
// it.  Then KD / 32 steps of 3 MFMAs per column tile; the results are collected in LDS (the same space) and
// stored as runs of MT modes per (n, p, k').
//   Edges: band rows at or beyond nlat_in, planes n >= N, modes m' >= Mo and the padding j >= s U are WRITTEN as
//   zeros into the image, never read (the padded table is zero there too, but 0 * stale-NaN is NaN); lo[g] is
//   clamped to [0, nlat_in - 1]; rows of a ragged last group (zero in the table) and planes n >= N are not
//   stored.  Nothing is loaded or stored outside Xh, the table, lo or Yh, whatever lo holds.
// Plain vector stores, one rounding, no atomics: bit-reproducible run to run and under hipGraph replay.
//
// bf16 instances (BF): Xh and Yh are bf16, the table the one plane bf16(T) (the hi plane alone): one MFMA per
// fragment pair, one LDS plane, a (re, im) pair one 4-byte load or store; accumulation stays fp32 and the result is
// rounded once, at the store.
//
// LDS per workgroup (disco_spectral_lds_bytes): planes x MT x (PTL x (2 KD + 16) + 32) B, e.g. 53760 B for fp32 at
// KD = 96, 8 modes x 16 planes; the tile shrinks to 8 planes, then 4 modes, to stay within 64 KiB.
//
// The transposed (upsampling) direction (TR; the disco_spectral_t op): Zh [N, K, nlat_in, Mi, 2] on the coarse grid,
// Yh [N, nlat_out, Mo, 2] on the fine one, s = nlon_out / nlon_in.  y is the circular convolution of PsiT with z
// upsampled by zeros, whose spectrum is the periodic extension of the coarse one, so
//   Yh[n, k, mu] = sum_{p, k'} H[p, k', k, mu] Zh[n, p, k', mu mod nlon_in],    0 <= mu < Mo,
//   H[p, k', k, mu] = sum_D PsiT[p, k', k, D] e^{-2 pi i mu D / nlon_out}   (a convolution: no conjugate),
// with no fold and no 1 / s.  The output has no basis index: a group is 16 consecutive OUTPUT latitudes, row = k - 16 g,
// and the K basis planes sit in the contraction, kappa = 2 (p U + k' - lo[g]) + c, KD = ceil32(2 K U), any K.  The
// A fragments, column_of, the MFMA step, the result image and the mode-run stores are the code of the forward
// direction; what differs:
//   staging: word (mode mt, plane pl, j = p U + dk) = Zh[n0 + pl, p, l0 + dk, nu], nu = (m0 + mt) mod nlon_in, read at
//     nlon_in - nu and conjugated where nu >= Mi: inside a tile the runs ascend, descend conjugated and wrap to 0;
//   chunks: KD grows with K U, so the tile stays 8 modes x 16 planes and the contraction is walked in chunks of KC
//     (disco_spectral_t_route: 96 fp32, 224 bf16) through LDS, the accumulators kept in registers: stage, barrier,
//     chunk / 32 MFMA steps against the table at chunk0 + 32 st, barrier.  j is flat, so a chunk edge may fall inside
//     a basis plane.  The forward direction is the one-chunk case, KC = KD;
//   epilogue: runs of MT modes to Yh[n, k, mu]; nlon_out bias[n mod C], the spectrum of the constant field, is added
//     to Re Yh[n, k, 0] in fp32 before the one rounding.  Rows k >= nlat_out, planes >= N, modes >= Mo are not stored.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "../nn/bf16_pack.h"
#include "spectral.h"

namespace amd_dft {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// the B fragment of a column from the four (re, im) words of its plane: (re, -im) for a real column, (im, re) for an
// imaginary one
__device__ __forceinline__ bf16x8 column_of(uint4 v, bool imag) {
  if (imag) {
    v.x = (v.x >> 16) | (v.x << 16);
    v.y = (v.y >> 16) | (v.y << 16);
    v.z = (v.z >> 16) | (v.z << 16);
    v.w = (v.w >> 16) | (v.w << 16);
  } else {
    v.x ^= 0x80000000u;
    v.y ^= 0x80000000u;
    v.z ^= 0x80000000u;
    v.w ^= 0x80000000u;
  }
  return __builtin_bit_cast(bf16x8, v);
}

template <bool BF, int MW, int CT, bool TR>
__global__ void __launch_bounds__(256)
    disco_spectral_kernel(const void* __restrict__ x, const uint16_t* __restrict__ th, const uint16_t* __restrict__ tl,
                          const int32_t* __restrict__ lo, void* __restrict__ y, const float* __restrict__ bias,
                          int64_t N, int64_t C, int nlat_in, int nlon_in, int K, int U, int nlat_out, int nlon_out,
                          int R, int KD, int KC_) {
  constexpr int MT = 4 * MW;    // modes per workgroup
  constexpr int PTL = 8 * CT;   // planes per workgroup
  constexpr int YP = 2 * MT + 2;  // floats per (row, plane) of the result image
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int g = blockIdx.z, m0 = blockIdx.x * MT;
  const int64_t n0 = static_cast<int64_t>(blockIdx.y) * PTL;
  const int Mi = nlon_in / 2 + 1, Mo = nlon_out / 2 + 1;
  const int KC = TR ? KC_ : KD;      // the forward direction is one chunk, known to the compiler
  const int PW = KC / 2 + 4;         // words between image rows: the (re, im) words of a whole chunk + 16 bytes
  const int MS = PTL * PW + kDiscoSpecModePad;  // words between modes
  const int PLANE = MT * MS;         // words per precision plane (hi, lo)
  const int JU = (TR ? K : nlon_in / nlon_out) * U;  // band words before the padding: K U, forward s U
  int l0 = lo[g];
  l0 = l0 < 0 ? 0 : l0 > nlat_in - 1 ? nlat_in - 1 : l0;

  // one (re, im) pair: a float2, or a packed bf16 pair
  using Pair = typename std::conditional<BF, uint32_t, float2>::type;
  const Pair* x2 = reinterpret_cast<const Pair*>(x);
  Pair* y2 = reinterpret_cast<Pair*>(y);

  f32x4 acc[MW][CT];
#pragma unroll
  for (int mw = 0; mw < MW; ++mw)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[mw][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool imag = l15 & 1;

  // the contraction in chunks of KC through LDS (forward: one chunk, KC = KD), the accumulators kept in registers
  for (int c0 = 0; c0 < KD; c0 += KC) {
    const int CH = (KD - c0 < KC ? KD - c0 : KC) / 2;  // (re, im) words per image row of this chunk
    if (c0) __syncthreads();                           // every wave is done reading the chunk before
    // ---- stage: word (mode mt, plane pl, j) with modes innermost (the contiguous runs of the spectrum);
    // forward j = r U + dk: Xh[n0 + pl, l0 + dk, m0 + mt + r nlon_out]; TR j = p U + dk: Zh[n0 + pl, p, l0 + dk, nu]
    for (int it = tid; it < PTL * CH * MT; it += 256) {
      const int mt = it % MT, rest = it / MT;
      const int jj = rest % CH, pl = rest / CH, j = c0 / 2 + jj;
      const int m = m0 + mt;
      const int64_t n = n0 + pl;
      Pair v;
      if constexpr (BF) v = 0u;
      else v = make_float2(0.f, 0.f);
      bool conj = false;
      if (j < JU && m < Mo && n < N) {
        const int r = j / U, k = l0 + (j - r * U);  // r: the fold (forward), the basis plane p (TR)
        if (k < nlat_in) {
          int mu = TR ? m % nlon_in : m + r * nlon_out;  // < nlon_in
          if (mu >= Mi) {  // above the stored half: the conjugate of mode nlon_in - mu in [1, Mi)
            mu = nlon_in - mu;
            conj = true;
          }
          v = x2[((TR ? n * K + r : n) * nlat_in + k) * Mi + mu];
        }
      }
      uint32_t* dst = smem + mt * MS + pl * PW + jj;
      if constexpr (BF) {
        *dst = conj ? v ^ 0x80000000u : v;  // re | im << 16
      } else {
        uint32_t h, l;
        split_pk(v.x, conj ? -v.y : v.y, h, l);
        dst[0] = h;
        dst[PLANE] = l;
      }
    }
    __syncthreads();

    // ---- MFMAs: wave wv owns modes wv, wv + 4, ... of the tile against both column tiles
    const int nstep = CH / 16;
#pragma unroll
    for (int mw = 0; mw < MW; ++mw) {
      const int mt = wv + 4 * mw;
      if (m0 + mt >= Mo) continue;  // wave-uniform: a mode past the spectrum
      // lane = T[g][m0 + mt][l15][c0 + 32 st + 8 lq + 0..7]
      const int64_t aoff = ((static_cast<int64_t>(g) * Mo + m0 + mt) * 16 + l15) * KD + c0 + 8 * lq;
      const uint32_t* brow = smem + mt * MS + (l15 >> 1) * PW + 4 * lq;
      for (int st = 0; st < nstep; ++st) {
        const bf16x8 Ah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(th + aoff + 32 * st));
        bf16x8 Al;
        if constexpr (!BF) Al = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(tl + aoff + 32 * st));
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const uint32_t* bs = brow + 8 * ct * PW + 16 * st;
          const bf16x8 Bh = column_of(*reinterpret_cast<const uint4*>(bs), imag);
          acc[mw][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh, acc[mw][ct], 0, 0, 0);
          if constexpr (!BF) {
            const bf16x8 Bl = column_of(*reinterpret_cast<const uint4*>(bs + PLANE), imag);
            acc[mw][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, Bh, acc[mw][ct], 0, 0, 0);
            acc[mw][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bl, acc[mw][ct], 0, 0, 0);
          }
        }
      }
    }
  }
  __syncthreads();  // every wave is done reading the band

  // ---- collect: acc[mw][ct][i] = row 4 lq + i, real column 16 ct + l15 -> image [row][plane][mode][re | im]
  float* yo = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int mw = 0; mw < MW; ++mw) {
    const int mt = wv + 4 * mw;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        yo[((4 * lq + i) * PTL + 8 * ct + (l15 >> 1)) * YP + 2 * mt + (l15 & 1)] = acc[mw][ct][i];
  }
  __syncthreads();
  // ---- store: runs of MT modes per (n, p, k'), row = (k' - g R) K + p; TR: per (n, k), row = k - 16 g
  for (int it = tid; it < 16 * PTL * MT; it += 256) {
    const int mt = it % MT, rest = it / MT;
    const int pl = rest % PTL, row = rest / PTL, m = m0 + mt;
    const int64_t n = n0 + pl;
    const float* src = yo + (row * PTL + pl) * YP + 2 * mt;
    float re = src[0];
    int64_t o;
    if constexpr (TR) {
      const int k = g * 16 + row;
      if (k >= nlat_out || m >= Mo || n >= N) continue;
      if (bias != nullptr && m == 0) re += static_cast<float>(nlon_out) * bias[n % C];
      o = (n * nlat_out + k) * Mo + m;
    } else {
      const int kl = row / K, p = row - kl * K, kp = g * R + kl;
      if (kl >= R || kp >= nlat_out || m >= Mo || n >= N) continue;
      o = (((n * K + p) * nlat_out + kp) * Mo + m);
    }
    if constexpr (BF) y2[o] = pk_bf16(re, src[1]);
    else y2[o] = make_float2(re, src[1]);
  }
}

template <bool BF, int MW, int CT, bool TR = false>
void launch_instance(const DiscoSpectralLaunch& p, const DiscoSpectralRoute& r, hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>((r.Mo + r.mt - 1) / r.mt), static_cast<unsigned>((p.N + r.ptl - 1) / r.ptl),
                  static_cast<unsigned>(r.G));
  hipLaunchKernelGGL((disco_spectral_kernel<BF, MW, CT, TR>), grid, dim3(256), static_cast<size_t>(r.lds), stream, p.x,
                     p.th, p.tl, p.lo, p.y, p.bias, p.N, p.C, p.nlat_in, p.nlon_in, p.K, p.U, p.nlat_out, p.nlon_out,
                     r.R, r.KD, r.KC);
}

}  // namespace

void launch_disco_spectral(const DiscoSpectralLaunch& p, void* stream_) {
  if (p.N == 0 || p.nlat_out == 0) return;
  const bool tr = p.transposed != 0;
  if (p.nlat_in < 1 || p.nlon_in < 1 || p.nlon_out < 1 || p.K < 1 || p.U < 1 || p.C < 1 ||
      (tr ? p.nlon_out % p.nlon_in : p.nlon_in % p.nlon_out) != 0)
    throw std::runtime_error("amd_dft: disco_spectral: bad sizes");
  const DiscoSpectralRoute r = (tr ? disco_spectral_t_route : disco_spectral_route)(
      p.N, p.nlat_in, p.nlon_in, p.K, p.nlat_out, p.nlon_out, p.U, p.bf16 != 0);
  if (!r.ok) throw std::runtime_error("amd_dft: disco_spectral: no instance (K > 16, or the band does not fit LDS)");
  if (r.G > 65535 || (p.N + r.ptl - 1) / r.ptl > 65535)
    throw std::runtime_error("amd_dft: disco_spectral: tensor too large");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int key = (tr ? 1000 : 0) + (p.bf16 ? 100 : 0) + 10 * r.mt + r.ptl / 8;
  switch (key) {
    case 82: launch_instance<false, 2, 2>(p, r, stream); break;
    case 81: launch_instance<false, 2, 1>(p, r, stream); break;
    case 41: launch_instance<false, 1, 1>(p, r, stream); break;
    case 182: launch_instance<true, 2, 2>(p, r, stream); break;
    case 181: launch_instance<true, 2, 1>(p, r, stream); break;
    case 141: launch_instance<true, 1, 1>(p, r, stream); break;
    case 1082: launch_instance<false, 2, 2, true>(p, r, stream); break;
    case 1182: launch_instance<true, 2, 2, true>(p, r, stream); break;
    default: throw std::runtime_error("amd_dft: disco_spectral: no instance for the route");
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: disco_spectral launch: ") + hipGetErrorString(e));
}

}  // namespace amd_dft

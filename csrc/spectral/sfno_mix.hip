// Per-degree channel mixing of a spherical harmonic spectrum on MFMA -- the middle step of an SFNO layer:
//   y[b, o, l, m] = sum_i c[b, i, l, m] * w[i, o, l]          (complex; one weight per degree l, shared by all m)
// c [B, Cin, L, M, 2] fp32 (complex as trailing re/im), w [Cin, Cout, L, 2] fp32, y [B, Cout, L, M, 2] fp32.
//
// Per degree l one complex GEMM, run as a real one with Cout output rows (not 2 Cout): the contraction is
// K = 2 Cin, interleaved -- k = 2 i carries Wr[i, o, l] against X[i], k = 2 i + 1 carries Wi[i, o, l] against
// i X[i], the pair (re, im) staged as (-im, re) -- over the real columns (b, m, re | im), so the result lands in
// the natural interleaved [.., m, 2] layout.
//
// Precision: the project's bf16x3 form, A.B = Ah.Bh + Al.Bh + Ah.Bl on v_mfma_f32_16x16x32_bf16 with fp32
// accumulation (as legendre.hip).  The weights arrive split on the host side as two bf16 planes (hi, lo),
// repacked degree-major and zero-padded to [L, Op = ceil16(Cout), Kp = ceil32(2 Cin)], so every A fragment is one
// aligned 16-byte global load that cannot leave the table; the spectrum is split as it is staged into LDS.
//
//   A = W[l][o][k]: lane holds W[o0 + 16 rt + l15][32 s + 8 lq + 0..7] of both planes, straight from global memory
//       (the four waves of a workgroup read the same fragments: one trip to L2, three hits in L1);
//   B = X[k][col]: from the LDS slab image [plane][col][32 k] bf16, column pitch 80 B (16-byte reads of 16
//       consecutive columns touch all 64 banks once).
// A workgroup (4 waves) owns one degree l (grid z), one group of up to 64 output channels (four 16-row tiles,
// grid y) and one tile of 64 complex = 128 real columns (grid x); wave w owns the tile's real columns
// 32 w .. 32 w + 31 (two 16-column MFMA tiles) against all four row tiles, and stages exactly those columns, a
// lane always the same one.  The columns of a degree are flattened over (b, m): complex column j = b Ml + m with
// Ml the live orders of the degree, so low degrees with few live orders still fill a tile from the batch.  It
// loops over K in 32-deep slabs (16 input channels); global reads of c are runs of 16 consecutive orders
// (128 B), global writes of y runs of 8 consecutive orders (64 B) per output row.
//   tri = 0: Ml = M, the dense product.  tri = 1 (the spectrum of a real field, zero where l < m): Ml =
//   min(M, l + 1) -- only the orders m <= l are read and computed; y[.., l, m > l] is stored as exact 0.0 (the
//   workgroups of a (degree, channel group) share those stores, the ones whose column tile is empty included:
//   those issue no loads at all).
//   Edges: i >= Cin and dead columns are WRITTEN as zeros into the slab image (the padded table is zero there
//   too, but 0 * stale-NaN is NaN); rows o >= Cout of the last tile are computed on the table's zero padding and
//   not stored.  Nothing is loaded or stored outside c, the padded table or y.
// The next slab's spectrum values are loaded into registers before the current slab's MFMAs; the table fragments
// of a slab are requested before the slab is written to LDS.  No atomics: bit-reproducible run to run.
//
// bf16 instance (BF): c and y are bf16, the weights the one plane bf16(W) (the hi plane alone), so a fragment pair
// is one MFMA instead of three; accumulation stays fp32 and the result is rounded once, at the store.  A (re, im)
// pair is one 4-byte load or store: staging builds (re, -im) and (im, re) from the packed pair with a sign flip and
// a rotate, the slab image is the one plane, and at the store the two lanes of an order exchange halves of their
// rows so that each writes packed pairs.  Column flattening, tri, the empty-tile exit and the edge zeros are the
// same code.
//
// LDS per workgroup (sfno_mix_lds_bytes): 2 planes x 128 columns x 80 B = 20480 B (bf16: 1 plane, 10240 B).
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

template <bool BF>
__global__ void __launch_bounds__(256) sfno_mix_kernel(const void* __restrict__ c, const uint16_t* __restrict__ wh,
                                                       const uint16_t* __restrict__ wl, void* __restrict__ y, int B,
                                                       int Cin, int Cout, int L, int M, int Op, int Kp, int tri) {
  constexpr int NJ = kSfnoColTile;              // complex columns per workgroup
  constexpr int RT = kSfnoRowTiles;
  constexpr int PLANE = 2 * NJ * kSfnoXPitch;   // bytes per plane (hi, lo)
  constexpr int XI = kSfnoSlab / 8;             // staged (channel, column) items per thread and slab
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int l = blockIdx.z, o0 = blockIdx.y * 16 * RT;
  const int Ml = tri == 1 && l + 1 < M ? l + 1 : M;  // live orders of this degree
  const int64_t ncols = static_cast<int64_t>(B) * Ml;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * NJ;
  // one (re, im) pair: a float2, or a packed bf16 pair
  using Pair = typename std::conditional<BF, uint32_t, float2>::type;
  const Pair* c2 = reinterpret_cast<const Pair*>(c);
  Pair* y2 = reinterpret_cast<Pair*>(y);
  const auto zero = [] {
    if constexpr (BF) return 0u;
    else return make_float2(0.f, 0.f);
  };

  // ---- the structurally zero part y[b, o0.., l, Ml..M-1]: shared by the workgroups of this (degree, group)
  if (Ml < M) {
    const int no = Cout - o0 < 16 * RT ? Cout - o0 : 16 * RT, zr = M - Ml;
    const int64_t total = static_cast<int64_t>(B) * no * zr;
    for (int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + tid; idx < total;
         idx += static_cast<int64_t>(gridDim.x) * 256) {
      const int mz = static_cast<int>(idx % zr);
      const int64_t t = idx / zr;
      const int ol = static_cast<int>(t % no), b = static_cast<int>(t / no);
      y2[((static_cast<int64_t>(b) * Cout + o0 + ol) * L + l) * M + Ml + mz] = zero();
    }
  }
  if (j0 >= ncols) return;  // empty column tile (block-uniform): no loads

  // ---- the column this lane stages, slab after slab: complex column 16 wv + l15 of the tile, channels 4 q + lq
  const int jl = 16 * wv + l15;
  const bool col_ok = j0 + jl < ncols;
  const int64_t chs = static_cast<int64_t>(L) * M;  // pair stride between input channels
  const Pair* src = c2;
  if (col_ok) {
    const int64_t j = j0 + jl;
    const int b = static_cast<int>(j / Ml), m = static_cast<int>(j % Ml);
    src = c2 + (static_cast<int64_t>(b) * Cin * L + l) * M + m;
  }
  const bool wave_live = j0 + 16 * wv < ncols;  // wave-uniform: any of the wave's columns inside the degree

  bool live[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) live[rt] = wave_live && o0 + 16 * rt < Cout;

  Pair xr[XI];
  auto load_slab = [&](int s) {
#pragma unroll
    for (int q = 0; q < XI; ++q) {
      const int i = s * (kSfnoSlab / 2) + 4 * q + lq;
      xr[q] = col_ok && i < Cin ? src[i * chs] : zero();
    }
  };

  f32x4 acc[RT][2];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nslab = Kp / kSfnoSlab;
  load_slab(0);
  for (int s = 0; s < nslab; ++s) {
    // ---- this slab's weight fragments (global, both planes): lane = W[l][o0 + 16 rt + l15][32 s + 8 lq + 0..7]
    uint4 ah[RT], al[BF ? 1 : RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      if (live[rt]) {
        const int64_t off = (static_cast<int64_t>(l) * Op + o0 + 16 * rt + l15) * Kp + s * kSfnoSlab + 8 * lq;
        ah[rt] = *reinterpret_cast<const uint4*>(wh + off);
        if constexpr (!BF) al[rt] = *reinterpret_cast<const uint4*>(wl + off);
      }
    }
    __syncthreads();  // every wave is done reading the previous slab
    // ---- the slab image: k = 2 i holds X[i], k = 2 i + 1 holds i X[i]; split into bf16 (hi, lo), k pairs packed
#pragma unroll
    for (int q = 0; q < XI; ++q) {
      char* dst = smem + 2 * jl * kSfnoXPitch + 4 * (4 * q + lq);
      if constexpr (BF) {
        const uint32_t v = xr[q];  // re | im << 16
        *reinterpret_cast<uint32_t*>(dst) = v ^ 0x80000000u;                  // real column: (re, -im)
        *reinterpret_cast<uint32_t*>(dst + kSfnoXPitch) = (v >> 16) | (v << 16);  // imaginary column: (im, re)
      } else {
        uint32_t hr, lr, hi, li;
        split_pk(xr[q].x, -xr[q].y, hr, lr);  // real column: (re, -im)
        split_pk(xr[q].y, xr[q].x, hi, li);   // imaginary column: (im, re)
        *reinterpret_cast<uint32_t*>(dst) = hr;
        *reinterpret_cast<uint32_t*>(dst + kSfnoXPitch) = hi;
        *reinterpret_cast<uint32_t*>(dst + PLANE) = lr;
        *reinterpret_cast<uint32_t*>(dst + PLANE + kSfnoXPitch) = li;
      }
    }
    __syncthreads();
    // ---- the next slab's global loads, in flight during the MFMAs
    if (s + 1 < nslab) load_slab(s + 1);
    // ---- MFMAs: live row tiles of a live wave only
    if (wave_live) {
      bf16x8 bh[2], bl[BF ? 1 : 2];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const char* bs = smem + (32 * wv + 16 * ct + l15) * kSfnoXPitch + 16 * lq;
        bh[ct] = *reinterpret_cast<const bf16x8*>(bs);
        if constexpr (!BF) bl[ct] = *reinterpret_cast<const bf16x8*>(bs + PLANE);
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        if (live[rt]) {
          const bf16x8 Ah = __builtin_bit_cast(bf16x8, ah[rt]);
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) {
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, bh[ct], acc[rt][ct], 0, 0, 0);
            if constexpr (!BF) {
              const bf16x8 Al = __builtin_bit_cast(bf16x8, al[rt]);
              acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, bh[ct], acc[rt][ct], 0, 0, 0);
              acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, bl[ct], acc[rt][ct], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  // ---- store: acc[rt][ct][i] = y row o0 + 16 rt + 4 lq + i, real column 32 wv + 16 ct + l15 of the tile; the 16
  // lanes of a row hold 8 consecutive orders' (re, im): one 64-byte run of y (split where the batch index steps)
  if (!wave_live) return;
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int64_t j = j0 + 16 * wv + 8 * ct + (l15 >> 1);
    if (j >= ncols) continue;
    const int b = static_cast<int>(j / Ml), m = static_cast<int>(j % Ml);
    if constexpr (BF) {
      // the even lane of an order holds re, the odd lane im, of rows i = 0..3: the even lane takes rows 0 and 2, the
      // odd lane rows 1 and 3, each sending the other the half it does not store (both lanes of a pair are live here:
      // j depends on l15 >> 1 alone)
      uint32_t* dst = reinterpret_cast<uint32_t*>(y) + ((static_cast<int64_t>(b) * Cout + o0) * L + l) * M + m;
      const bool odd = l15 & 1;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
        for (int i = 0; i < 4; i += 2) {
          const float own0 = acc[rt][ct][i], own1 = acc[rt][ct][i + 1];
          const float got = __shfl_xor(odd ? own0 : own1, 1);
          const int ol = 16 * rt + 4 * lq + i + (odd ? 1 : 0);
          const uint32_t v = odd ? pk_bf16(got, own1) : pk_bf16(own0, got);
          if (o0 + ol < Cout) dst[ol * chs] = v;
        }
      }
    } else {
      float* dst = reinterpret_cast<float*>(y) + (((static_cast<int64_t>(b) * Cout + o0) * L + l) * M + m) * 2 + (l15 & 1);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ol = 16 * rt + 4 * lq + i;
          if (o0 + ol < Cout) dst[ol * chs * 2] = acc[rt][ct][i];
        }
      }
    }
  }
}

}  // namespace

void launch_sfno_mix(const SfnoMixLaunch& p, void* stream) {
  if (p.B == 0 || p.Cout == 0 || p.L == 0 || p.M == 0) return;
  if (p.Cin < 1) throw std::runtime_error("amd_dft: sfno_mix: Cin must be >= 1");
  if (p.tri < 0 || p.tri > 1) throw std::runtime_error("amd_dft: sfno_mix: tri must be 0 or 1");
  const SfnoMixRoute r = sfno_mix_route(p.B, p.Cin, p.Cout, p.L, p.M, p.tri, p.bf16 != 0);
  if (r.ogroups > 65535 || p.L > 65535 || static_cast<int64_t>(p.B) * p.M >= (int64_t(1) << 30))
    throw std::runtime_error("amd_dft: sfno_mix: tensor too large");
  const dim3 grid(static_cast<unsigned>(r.ctiles), r.ogroups, p.L);
  if (p.bf16)
    hipLaunchKernelGGL(sfno_mix_kernel<true>, grid, dim3(256), static_cast<size_t>(r.lds),
                       static_cast<hipStream_t>(stream), p.c, p.wh, p.wl, p.y, p.B, p.Cin, p.Cout, p.L, p.M,
                       r.otiles * 16, r.slabs * kSfnoSlab, p.tri);
  else
    hipLaunchKernelGGL(sfno_mix_kernel<false>, grid, dim3(256), static_cast<size_t>(r.lds),
                       static_cast<hipStream_t>(stream), p.c, p.wh, p.wl, p.y, p.B, p.Cin, p.Cout, p.L, p.M,
                       r.otiles * 16, r.slabs * kSfnoSlab, p.tri);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: sfno_mix launch: ") + hipGetErrorString(e));
}

}  // namespace amd_dft

// amd_dft-build-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
// Global attention on the sphere on MFMA: dense flash attention of every output point over ALL input points.
//   score(k, j)       = scale * sum_c q[b, h, c, k', j'] k[b, h, c, k, j] + logw[k]
//   y[b, h, :, k', j'] = sum_{all (k, j)} softmax(score)(k, j) v[b, h, :, k, j]
// q [B, heads * d, nlat_out, nlon_out], k and v [B, heads * d, nlat_in, nlon_in], all fp32 or all bf16 (NCHW); y as
// q.  1 <= d <= 128.  Any two grids: no table, no divisibility rule.
//
// Problem view.  The grids are flat: Nq = nlat_out nlon_out queries, Nk = nlat_in nlon_in keys.  In NCHW a channel
// plane is contiguous over pixels, so 64 consecutive keys are one coalesced segment per channel; a chunk may cross
// latitude rows, and only the bias knows about rows.
//
// Work split.  A workgroup of 256 threads owns one (b, head) and QW * 4 consecutive queries, QW = 16 NQ per wave:
// NQ = 2 MFMA column tiles (1 for fp32 at DP = 128, where the registers demand it), so every K and V fragment read
// from LDS feeds NQ query tiles.  Queries past Nq are loaded as zeros and never stored.  Q is loaded once,
// channel-minor and zero-padded to DP = 32, 64 or 128 channels, and kept as B fragments (fp32: hi and lo).
//
// Key walk.  Chunks of 64 keys go through LDS: K transposed at the write to [key][DP + 8], V natural [channel][64 +
// 8], fp32 three planes of each (hi, lo, rest), then the bias row of 64 floats.  Two buffers: the global loads of
// chunk t + 1 are issued before the MFMA work of chunk t and written to the other buffer after it; one barrier per
// chunk.  fp32 at DP = 128 has one buffer (three planes of two buffers do not fit 160 KB): the loads are still
// issued before the MFMA work, the write waits for a second barrier.  K and V past Nk and channels past d are
// WRITTEN as zeros (0 * stale NaN is NaN).
//
// The mask is the bias: bias2[key] = logw[key / nlon_in] log2 e, -inf for keys past Nk, added to the score, so the
// ragged last chunk needs no case of its own and the inner loop holds no compare on a key or a query.
//
// MFMA steps (v_mfma_f32_16x16x32_bf16; A: lane = row l15, k = 8 lq + 0..7; B: lane = column l15, k = 8 lq + 0..7;
// C: acc[i] = row 4 lq + i, column l15), per 32 keys of a chunk:
//   S = K . Q      rows = 16 keys (two tiles), columns = 16 queries (NQ tiles), contraction over channels: a lane's
//                  accumulators are 4 keys of ONE query per tile;
//   softmax        online, in base 2: the running maximum is reduced across the four lanes of a query, the running
//                  sum is kept per lane and reduced once, in the epilogue; the exponent is taken against 0 while the
//                  maximum is -inf;
//   O += V . P     rows = channels (DP / 16 tiles), columns = queries, contraction over the 32 keys.  P is the B
//                  operand straight from the score accumulators: contraction index 8 lq + 4 t + i stands for key
//                  16 t + 4 lq + i of the step, and the V fragment is read in that order, so P never goes through
//                  LDS.  O is rescaled only in a step where some query of the wave moved its maximum (a multiply by
//                  1 is exact, so skipping it changes no bit).
// Epilogue: O / sum, one rounding at the store, plain vector stores: no atomics, bit-identical run to run.
//
// Precision.  bf16: the operands as they are, P rounded to bf16, the sum taken from the unrounded P, fp32
// accumulation.  fp32: the bf16x3 split plus the rest of the staged operand, A.B = Ah.Bh + Al.Bh + Ah.Bl + Ar.Bh with
// A = K or V split three ways (x = hi + lo + rest up to 2^-27 x) and B = Q or P split two ways.  Measured on the
// module test: with the plain bf16x3 split the rests of K and V, about 2^-18 of every operand, left 1.1e-5 per field
// after the softmax; the fourth product costs a third LDS plane and brings it to the figure in the README.
//
// Deviations from the plan of record: the queries per workgroup are a function of the instance alone (no switch to
// 64 queries where the grid is small: every compiled instance is then the one the tests reach), O stays where the
// compiler puts it, and fp32 carries a third plane of K and V (above).
//
// Memory safety: every global index is built from a query below Nq, a key below Nk (so a row below nlat_in) and a
// channel below d.  LDS per workgroup: attention_s2_global_route in spectral.h.
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

constexpr int kNT = kAttnS2GThreads;
constexpr int kKC = kAttnS2GChunk;
constexpr float kLog2e = 1.4426950408889634f;

struct Args {
  const void* q;
  const void* k;
  const void* v;
  const float* logw;
  void* y;
  int d, nlon_in, nq, nk, qtiles;  // nq, nk: points of the output and the input grid
  float scale2;                    // scale * log2 e
};

// ---- the fragment helpers of attention_s2.hip
template <bool BF>
__device__ __forceinline__ float ld(const void* p, int64_t i) {
  if constexpr (BF) return __uint_as_float(static_cast<uint32_t>(reinterpret_cast<const uint16_t*>(p)[i]) << 16);
  else return reinterpret_cast<const float*>(p)[i];
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ bf16x8 frag(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return __builtin_bit_cast(bf16x8, uint4{a, b, c, d});
}
// eight values -> one fragment (BF: they are bf16 values already, the rounding is exact), or its (hi, lo) split
template <bool BF>
__device__ __forceinline__ void pack8(const float (&f)[8], uint4& hi, uint4& lo) {
  uint32_t h[4], l[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if constexpr (BF) h[e] = pk_bf16(f[2 * e], f[2 * e + 1]);
    else split_pk(f[2 * e], f[2 * e + 1], h[e], l[e]);
  }
  hi = uint4{h[0], h[1], h[2], h[3]};
  lo = uint4{l[0], l[1], l[2], l[3]};
}
// the staged operands K and V in fp32: (hi, lo, rest), rest = bf16(x - hi - lo), both differences exact in fp32
__device__ __forceinline__ void pack8x3(const float (&f)[8], uint4& hi, uint4& lo, uint4& rs) {
  uint32_t h[4], l[4], r[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float a = f[2 * e], b = f[2 * e + 1];
    split_pk(a, b, h[e], l[e]);
    r[e] = pk_bf16(a - __uint_as_float(h[e] << 16) - __uint_as_float(l[e] << 16),
                   b - __uint_as_float(h[e] & 0xffff0000u) - __uint_as_float(l[e] & 0xffff0000u));
  }
  hi = uint4{h[0], h[1], h[2], h[3]};
  lo = uint4{l[0], l[1], l[2], l[3]};
  rs = uint4{r[0], r[1], r[2], r[3]};
}
__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// A.B on one MFMA (bf16 operands) or four (fp32 operands: the bf16x3 split plus the rest of A, the staged operand)
template <bool BF>
__device__ __forceinline__ f32x4 mma(bf16x8 ah, bf16x8 al, bf16x8 ar, bf16x8 bh, bf16x8 bl, f32x4 c) {
  c = mfma(ah, bh, c);
  if constexpr (!BF) {
    c = mfma(al, bh, c);
    c = mfma(ah, bl, c);
    c = mfma(ar, bh, c);
  }
  return c;
}

template <bool BF, int DP, int NQ>
__global__ void __launch_bounds__(kNT) attention_s2_global_kernel(const Args a) {
  constexpr int NP = BF ? 1 : 3;       // LDS planes per operand: hi (, lo, rest)
  constexpr int NBUF = !BF && DP == 128 ? 1 : 2;  // LDS buffers (attention_s2_global_route)
  constexpr int KS = DP / 32;          // contraction steps of the score product
  constexpr int RT = DP / 16;          // output row tiles
  constexpr int SG = DP / 32;          // channel groups of eight a thread stages per chunk
  constexpr int KP = (DP + 8) * 2;     // K pitch in bytes: [key][channel]
  constexpr int VP = (kKC + 8) * 2;    // V pitch in bytes: [channel][key]
  constexpr int KPLANE = kKC * KP, VPLANE = DP * VP;
  constexpr int BIAS = NP * (KPLANE + VPLANE);  // the bias row of a buffer
  constexpr int BUF = BIAS + kKC * 4;
  constexpr int QW = 16 * NQ;
  constexpr float NEG = -__builtin_huge_valf();
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6), l15 = lane & 15, lq = lane >> 4;
  const int d = a.d;
  const int bh = blockIdx.x / a.qtiles, qt = blockIdx.x - bh * a.qtiles;
  const int64_t nq = a.nq, nk = a.nk;
  const int64_t in0 = static_cast<int64_t>(bh) * d * nk, out0 = static_cast<int64_t>(bh) * d * nq;
  const int64_t jw = static_cast<int64_t>(qt) * (4 * QW) + QW * wv;  // the wave's first query
  const bool wave_live = jw < nq;

  // ---- the query fragments: Q[query l15 of tile n][channel 32 ks + 8 lq + 0..7], zero past d and past Nq
  bf16x8 qh[NQ][KS], ql[NQ][KS];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    const int64_t jq = jw + 16 * n + l15;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = 32 * ks + 8 * lq + e;
        f[e] = jq < nq && c < d ? ld<BF>(a.q, out0 + c * nq + jq) : 0.f;
      }
      uint4 h, l;
      pack8<BF>(f, h, l);
      qh[n][ks] = __builtin_bit_cast(bf16x8, h);
      ql[n][ks] = __builtin_bit_cast(bf16x8, l);
    }
  }

  float m[NQ], lsum[NQ];  // running maximum of a query (its four lanes agree), this lane's part of its sum
  f32x4 o[RT][NQ];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    m[n] = NEG;
    lsum[n] = 0.f;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) o[rt][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // ---- staging: a lane owns key sp of the chunk and the channel groups sg, sg + 4, ...; wave 0 also the bias row
  // (wave-uniform, so a load's address is a scalar base plus the lane's key)
  const int sp = lane, sg = wv;
  float kf[SG][8], vf[SG][8], bias = NEG;
  auto stage_load = [&](int t) {
    const int64_t key0 = static_cast<int64_t>(t) * kKC, key = key0 + sp;
    const bool ok = key < nk;
#pragma unroll
    for (int g = 0; g < SG; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = 8 * (sg + 4 * g) + e;
        const bool in = ok && c < d;
        const int64_t at = in0 + c * nk + key0;  // uniform
        kf[g][e] = in ? ld<BF>(a.k, at + sp) : 0.f;
        vf[g][e] = in ? ld<BF>(a.v, at + sp) : 0.f;
      }
    if (sg == 0) bias = ok ? a.logw[static_cast<int>(key) / a.nlon_in] * kLog2e : NEG;  // key < Nk < 2^31
  };
  auto stage_write = [&](char* buf) {
    char* const Ks = buf;
    char* const Vs = buf + NP * KPLANE;
#pragma unroll
    for (int g = 0; g < SG; ++g) {
      const int gg = sg + 4 * g;
      uint4 h, l, r = uint4{0u, 0u, 0u, 0u};
      if constexpr (BF) pack8<BF>(kf[g], h, l);
      else pack8x3(kf[g], h, l, r);
      *reinterpret_cast<uint4*>(Ks + sp * KP + 16 * gg) = h;
      if constexpr (!BF) {
        *reinterpret_cast<uint4*>(Ks + KPLANE + sp * KP + 16 * gg) = l;
        *reinterpret_cast<uint4*>(Ks + 2 * KPLANE + sp * KP + 16 * gg) = r;
      }
      if constexpr (BF) pack8<BF>(vf[g], h, l);
      else pack8x3(vf[g], h, l, r);
      const uint32_t hv[4] = {h.x, h.y, h.z, h.w}, lv[4] = {l.x, l.y, l.z, l.w}, rv[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        char* dst = Vs + (8 * gg + 2 * e) * VP + 2 * sp;
        *reinterpret_cast<uint16_t*>(dst) = static_cast<uint16_t>(hv[e] & 0xffffu);
        *reinterpret_cast<uint16_t*>(dst + VP) = static_cast<uint16_t>(hv[e] >> 16);
        if constexpr (!BF) {
          *reinterpret_cast<uint16_t*>(dst + VPLANE) = static_cast<uint16_t>(lv[e] & 0xffffu);
          *reinterpret_cast<uint16_t*>(dst + VPLANE + VP) = static_cast<uint16_t>(lv[e] >> 16);
          *reinterpret_cast<uint16_t*>(dst + 2 * VPLANE) = static_cast<uint16_t>(rv[e] & 0xffffu);
          *reinterpret_cast<uint16_t*>(dst + 2 * VPLANE + VP) = static_cast<uint16_t>(rv[e] >> 16);
        }
      }
    }
    if (sg == 0) reinterpret_cast<float*>(buf + BIAS)[sp] = bias;
  };

  const int nch = static_cast<int>((nk + kKC - 1) / kKC);
  stage_load(0);
  stage_write(smem);
  __syncthreads();

  for (int t = 0; t < nch; ++t) {
    const char* const buf = smem + (t % NBUF) * BUF;
    const bool more = t + 1 < nch;  // workgroup-uniform
    if (more) stage_load(t + 1);    // in flight during the MFMA work below

    if (wave_live) {  // wave-uniform; the barrier is outside
      const char* const Ks = buf;
      const char* const Vs = buf + NP * KPLANE;
#pragma unroll
      for (int st = 0; st < kKC / 32; ++st) {
        // ---- S = K . Q: two 16-key tiles, every K fragment against the NQ query tiles
        f32x4 acc[2][NQ];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
#pragma unroll
          for (int n = 0; n < NQ; ++n) acc[t2][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const char* src = Ks + (32 * st + 16 * t2 + l15) * KP + (32 * ks + 8 * lq) * 2;
            const bf16x8 kh = *reinterpret_cast<const bf16x8*>(src);
            bf16x8 kl = kh, kr = kh;
            if constexpr (!BF) {
              kl = *reinterpret_cast<const bf16x8*>(src + KPLANE);
              kr = *reinterpret_cast<const bf16x8*>(src + 2 * KPLANE);
            }
#pragma unroll
            for (int n = 0; n < NQ; ++n) acc[t2][n] = mma<BF>(kh, kl, kr, qh[n][ks], ql[n][ks], acc[t2][n]);
          }
        }
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(buf + BIAS + (32 * st + 4 * lq) * 4);
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(buf + BIAS + (32 * st + 16 + 4 * lq) * 4);

        // ---- online softmax of every query column
        float alpha[NQ];
        bf16x8 ph[NQ], pl[NQ];
        bool moved = false;
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
          float sc[8], mstep = NEG;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sc[i] = acc[0][n][i] * a.scale2 + b0[i];
            sc[4 + i] = acc[1][n][i] * a.scale2 + b1[i];
            mstep = fmaxf(mstep, fmaxf(sc[i], sc[4 + i]));
          }
          mstep = fmaxf(mstep, __shfl_xor(mstep, 16));
          mstep = fmaxf(mstep, __shfl_xor(mstep, 32));
          const float mnew = fmaxf(m[n], mstep);
          const float msafe = mnew == NEG ? 0.f : mnew;  // no finite score so far: exponents against 0
          alpha[n] = __builtin_amdgcn_exp2f(m[n] - msafe);
          moved = moved || mnew != m[n];
          m[n] = mnew;
          float pr[8], psum = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            pr[i] = __builtin_amdgcn_exp2f(sc[i] - msafe);
            psum += pr[i];
          }
          lsum[n] = lsum[n] * alpha[n] + psum;
          uint4 ph4, pl4;
          pack8<BF>(pr, ph4, pl4);
          ph[n] = __builtin_bit_cast(bf16x8, ph4);
          pl[n] = __builtin_bit_cast(bf16x8, pl4);
        }
        if (__any(moved)) {  // wave-uniform; elsewhere every alpha is 1
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int n = 0; n < NQ; ++n)
#pragma unroll
              for (int i = 0; i < 4; ++i) o[rt][n][i] *= alpha[n];
        }

        // ---- O += V . P: contraction index 8 lq + 4 t2 + i is key 16 t2 + 4 lq + i of the step
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          if (16 * rt >= d) continue;
          const char* src = Vs + (16 * rt + l15) * VP + (32 * st + 4 * lq) * 2;
          const uint2 v0 = *reinterpret_cast<const uint2*>(src);
          const uint2 v1 = *reinterpret_cast<const uint2*>(src + 32);
          const bf16x8 vh = frag(v0.x, v0.y, v1.x, v1.y);
          bf16x8 vl = vh, vr = vh;
          if constexpr (!BF) {
            const uint2 w0 = *reinterpret_cast<const uint2*>(src + VPLANE);
            const uint2 w1 = *reinterpret_cast<const uint2*>(src + VPLANE + 32);
            vl = frag(w0.x, w0.y, w1.x, w1.y);
            const uint2 x0 = *reinterpret_cast<const uint2*>(src + 2 * VPLANE);
            const uint2 x1 = *reinterpret_cast<const uint2*>(src + 2 * VPLANE + 32);
            vr = frag(x0.x, x0.y, x1.x, x1.y);
          }
#pragma unroll
          for (int n = 0; n < NQ; ++n) o[rt][n] = mma<BF>(vh, vl, vr, ph[n], pl[n], o[rt][n]);
        }
      }
    }

    if constexpr (NBUF == 1) __syncthreads();  // one buffer: every wave is done with it first
    if (more) stage_write(smem + ((t + 1) % NBUF) * BUF);  // two: the buffer every wave left at the previous barrier
    __syncthreads();
  }

  // ---- epilogue: the sum across the four lanes of a query, one division, one rounding at the store
  if (!wave_live) return;
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    float s = lsum[n];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    const float inv = s > 0.f ? 1.f / s : 0.f;
    const int64_t jq = jw + 16 * n + l15;
    if (jq >= nq) continue;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = 16 * rt + 4 * lq + i;
        if (c >= d) continue;
        const float val = o[rt][n][i] * inv;
        const int64_t at = out0 + c * nq + jq;
        if constexpr (BF) reinterpret_cast<__bf16*>(a.y)[at] = static_cast<__bf16>(val);
        else reinterpret_cast<float*>(a.y)[at] = val;
      }
    }
  }
}

template <bool BF, int DP, int NQ>
void launch(const Args& a, const AttnS2GlobalRoute& r, hipStream_t st) {
  if (r.lds > 64 * 1024) {  // more than 64 KB of dynamic LDS has to be asked for
    const hipError_t attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_s2_global_kernel<BF, DP, NQ>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(r.lds));
    if (attr != hipSuccess)
      throw std::runtime_error(std::string("amd_dft: attention_s2_global: attr: ") + hipGetErrorString(attr));
  }
  hipLaunchKernelGGL((attention_s2_global_kernel<BF, DP, NQ>), dim3(static_cast<uint32_t>(r.wgs)), dim3(kNT),
                     static_cast<size_t>(r.lds), st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("amd_dft: attention_s2_global: launch: ") + hipGetErrorString(e));
}

}  // namespace

void launch_attention_s2_global(const AttnS2GlobalLaunch& p, void* stream) {
  constexpr int64_t k2p31 = int64_t(1) << 31;
  if (p.B <= 0 || p.heads <= 0 || p.nlat_out <= 0 || p.nlon_out <= 0) return;
  if (p.d < 1 || p.d > kAttnS2GMaxD)
    throw std::invalid_argument("amd_dft: attention_s2_global: the head dimension must be 1 .. " +
                                std::to_string(kAttnS2GMaxD) + " on the device, got " + std::to_string(p.d));
  const int64_t nq = static_cast<int64_t>(p.nlat_out) * p.nlon_out, nk = static_cast<int64_t>(p.nlat_in) * p.nlon_in;
  if (p.nlat_in < 1 || p.nlon_in < 1 || nq >= k2p31 || nk >= k2p31 || p.B * p.heads >= k2p31)
    throw std::invalid_argument("amd_dft: attention_s2_global: bad launch (sizes)");
  const AttnS2GlobalRoute r =
      attention_s2_global_route(p.B, p.heads, p.d, p.nlat_in, p.nlon_in, p.nlat_out, p.nlon_out, p.bf16 != 0);
  if (r.wgs >= k2p31 || r.lds > kAttnS2GLdsMax)
    throw std::invalid_argument("amd_dft: attention_s2_global: too many workgroups or too much LDS");
  Args a;
  a.q = p.q;
  a.k = p.k;
  a.v = p.v;
  a.logw = p.logw;
  a.y = p.y;
  a.d = static_cast<int>(p.d);
  a.nlon_in = p.nlon_in;
  a.nq = static_cast<int>(nq);
  a.nk = static_cast<int>(nk);
  a.qtiles = static_cast<int>(r.qtiles);
  a.scale2 = p.scale * kLog2e;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (p.bf16) {
    if (r.dp == 32) launch<true, 32, 2>(a, r, st);
    else if (r.dp == 64) launch<true, 64, 2>(a, r, st);
    else launch<true, 128, 2>(a, r, st);
  } else {
    if (r.dp == 32) launch<false, 32, 2>(a, r, st);
    else if (r.dp == 64) launch<false, 64, 2>(a, r, st);
    else launch<false, 128, 1>(a, r, st);
  }
}

}  // namespace amd_dft

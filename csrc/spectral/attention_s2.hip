// amd_dft-build-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
// Neighbourhood attention on the sphere on MFMA: sliding-window flash attention on a ring of longitudes.
//   score(k, j)       = scale * sum_c q[b, h, c, k', j'] k[b, h, c, k, j] + logw[k]
//   y[b, h, :, k', j'] = sum_{(k, j) in N(k', j')} softmax_N(score)(k, j) v[b, h, :, k, j]
// N(k', j'): the longitudes j of input row k with circular |j - s j'| <= hw[k', k], s = nlon_in / nlon_out; hw < 0:
// no neighbour in that row; 2 hw + 1 >= nlon_in: the whole row, each longitude once.  An empty N gives 0.
// q [B, heads * d, nlat_out, nlon_out], k and v [B, heads * d, nlat_in, nlon_in], all fp32 or all bf16 (NCHW); y as
// q.  1 <= d <= 64.
//
// Work split.  A workgroup of 256 threads owns one (b, head, k') and a tile of 64 output longitudes, 16 per wave.
// Workgroups are numbered from both poles inwards: polar output rows see whole input rows and start first.  Each
// lane loads its part of the wave's 16 x d query tile once, channel-minor and zero-padded to DP = 32 or 64 channels,
// and keeps it as the B fragments of the score product for the workgroup's lifetime.
//
// Key walk.  For every input row k with hw[k', k] >= 0 the workgroup walks the union interval of its queries,
// longitudes s j'0 - hw .. s (j'0 + nq - 1) + hw mod nlon_in (nq the tile's live queries), capped at nlon_in
// consecutive longitudes so that no key is visited twice, in chunks of 64 key longitudes staged through LDS from
// NCHW: a lane owns one key longitude and eight channels at a time, so each channel's row segment is one coalesced
// read.  K is written channel-minor [key][DP + 8] (transposed at the LDS write, one 16-byte write per eight
// channels), V key-minor [channel][64 + 8], the natural layout.  Keys past the interval and channels past d are
// WRITTEN as zeros (0 * stale NaN is NaN).
//
// MFMA steps (v_mfma_f32_16x16x32_bf16; A: lane = row l15, k = 8 lq + 0..7; B: lane = column l15, k = 8 lq + 0..7;
// C: acc[i] = row 4 lq + i, column l15), per 32 keys of a chunk:
//   S = K . Q      rows = 16 keys (two tiles), columns = the wave's 16 queries, contraction over channels: a lane's
//                  accumulators are 4 keys of ONE query, so the softmax state of a query lives in the four lanes
//                  l15, l15 + 16, l15 + 32, l15 + 48;
//   mask           circular distance of the key's longitude to s j' against hw (hw is clamped to nlon_in / 2, where
//                  the test is always true: the whole row needs no case of its own);
//   softmax        online, in base 2 (log2 e folded into scale and logw): the running maximum is reduced across the
//                  four lanes of a query with two cross-lane moves per step, the running sum is kept per lane and
//                  reduced once, in the epilogue.  While every key so far was masked the maximum is -inf and the
//                  exponent is taken against 0 instead: exp2(-inf - 0) = 0, never exp2(-inf + inf);
//   O += V . P     rows = channels (up to four 16-row tiles), columns = queries, contraction over the 32 keys.  P is
//                  the B operand straight from the score accumulators: the contraction index 8 lq + 4 t + i stands
//                  for key 16 t + 4 lq + i of the step, and the V fragment is read in that order (two 8-byte LDS
//                  reads per lane), so P never goes through LDS.
// A wave skips a 32-key step that lies wholly outside its own 16 queries' windows (not where the walk was capped).
// Epilogue: O / sum, one rounding at the store, plain vector stores: no atomics, bit-identical run to run.
//
// Precision.  bf16: the operands as they are, P rounded to bf16, the sum taken from the unrounded P, fp32
// accumulation.  fp32: the project's bf16x3 split, A.B = Ah.Bh + Al.Bh + Ah.Bl with fp32 accumulation: q, k and v
// are split as they are staged (two LDS planes), P is split in registers.
//
// Memory safety: hw is clamped to [-1, nlon_in / 2] here; every global index is built from a longitude reduced into
// [0, nlon_in), a row below nlat_in and a channel below d, so nothing outside q, k, v, hw, logw and y is touched
// whatever hw holds.  LDS per workgroup: attention_s2_route in spectral.h.
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

constexpr int kNT = kAttnS2Threads;
constexpr int kQT = kAttnS2QTile;
constexpr int kKC = kAttnS2Chunk;
constexpr float kLog2e = 1.4426950408889634f;

struct Args {
  const void* q;
  const void* k;
  const void* v;
  const int32_t* hw;
  const float* logw;
  void* y;
  int heads_b;  // B * heads
  int d, nlat_in, nlon_in, nlat_out, nlon_out, s, qtiles;
  float scale2;  // scale * log2 e
};

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
__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// A.B on one MFMA (bf16 operands) or three (the bf16x3 split of fp32 operands)
template <bool BF>
__device__ __forceinline__ f32x4 mma(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x4 c) {
  c = mfma(ah, bh, c);
  if constexpr (!BF) {
    c = mfma(al, bh, c);
    c = mfma(ah, bl, c);
  }
  return c;
}

template <bool BF, int DP>
__global__ void __launch_bounds__(kNT) attention_s2_kernel(const Args a) {
  constexpr int NP = BF ? 1 : 2;       // LDS planes per operand: hi (, lo)
  constexpr int KS = DP / 32;          // contraction steps of the score product
  constexpr int RT = DP / 16;          // output row tiles
  constexpr int KP = (DP + 8) * 2;     // K pitch in bytes: [key][channel]
  constexpr int VP = (kKC + 8) * 2;    // V pitch in bytes: [channel][key]
  constexpr int KPLANE = kKC * KP, VPLANE = DP * VP;
  constexpr float NEG = -__builtin_huge_valf();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Ks = smem;
  char* const Vs = smem + NP * KPLANE;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const int d = a.d, n = a.nlon_in, s = a.s;
  // workgroup -> (latitude from both poles inwards, (b, head), query tile)
  const int per_lat = a.heads_b * a.qtiles;
  const int r = blockIdx.x / per_lat, rem = blockIdx.x - r * per_lat;
  const int kp = (r & 1) ? a.nlat_out - 1 - (r >> 1) : (r >> 1);
  const int bh = rem / a.qtiles, qt = rem - bh * a.qtiles;
  const int j0 = qt * kQT;
  const int nq = a.nlon_out - j0 < kQT ? a.nlon_out - j0 : kQT;  // live queries of the tile, >= 1
  const int jq = j0 + 16 * wv + l15;                             // this lane's query
  const bool q_ok = jq < a.nlon_out;
  const bool wave_live = 16 * wv < nq;
  const int64_t plane_in = static_cast<int64_t>(a.nlat_in) * n;
  const int64_t plane_out = static_cast<int64_t>(a.nlat_out) * a.nlon_out;
  const int64_t in0 = static_cast<int64_t>(bh) * d * plane_in;
  const int64_t out0 = static_cast<int64_t>(bh) * d * plane_out + static_cast<int64_t>(kp) * a.nlon_out;

  // ---- the query fragments: Q[query l15][channel 32 ks + 8 lq + 0..7], zero past d and past the row
  bf16x8 qh[KS], ql[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = 32 * ks + 8 * lq + e;
      f[e] = q_ok && c < d ? ld<BF>(a.q, out0 + c * plane_out + jq) : 0.f;
    }
    uint4 h, l;
    pack8<BF>(f, h, l);
    qh[ks] = __builtin_bit_cast(bf16x8, h);
    ql[ks] = __builtin_bit_cast(bf16x8, l);
  }

  float m = NEG, lsum = 0.f;  // running maximum of the query (all four lanes agree), this lane's part of the sum
  f32x4 o[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) o[rt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int sp = tid & 63, sg = tid >> 6;  // staging: key longitude of the chunk, first channel group of eight

  for (int kr = 0; kr < a.nlat_in; ++kr) {
    const int hraw = uni(a.hw[static_cast<int64_t>(kp) * a.nlat_in + kr]);
    if (hraw < 0) continue;  // workgroup-uniform
    const int hwc = hraw < (n >> 1) ? hraw : (n >> 1);
    int L = s * (nq - 1) + 2 * hwc + 1;  // the union interval of the tile's queries
    const bool capped = L >= n;
    if (capped) L = n;
    int start = s * j0 - hwc;  // s j0 < nlon_in and hwc <= nlon_in / 2: one wrap at most
    if (start < 0) start += n;
    const float lw = a.logw[kr] * kLog2e;
    const int cq = s * (16 * wv + l15) + hwc;  // the walk position of this lane's query
    const int64_t row0 = in0 + static_cast<int64_t>(kr) * n;

    for (int p0 = 0; p0 < L; p0 += kKC) {
      __syncthreads();  // every wave is done with the previous chunk
      // ---- stage the chunk: lane = key longitude, eight channels at a time
      {
        const bool ok = p0 + sp < L;
        int j = start + p0 + sp;  // < 2 nlon_in
        if (j >= n) j -= n;
#pragma unroll
        for (int gg = sg; gg < DP / 8; gg += 4) {
          float kf[8], vf[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int c = 8 * gg + e;
            const bool in = ok && c < d;
            kf[e] = in ? ld<BF>(a.k, row0 + c * plane_in + j) : 0.f;
            vf[e] = in ? ld<BF>(a.v, row0 + c * plane_in + j) : 0.f;
          }
          uint4 h, l;
          pack8<BF>(kf, h, l);
          *reinterpret_cast<uint4*>(Ks + sp * KP + 16 * gg) = h;
          if constexpr (!BF) *reinterpret_cast<uint4*>(Ks + KPLANE + sp * KP + 16 * gg) = l;
          pack8<BF>(vf, h, l);
          const uint32_t hv[4] = {h.x, h.y, h.z, h.w}, lv[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            char* dst = Vs + (8 * gg + 2 * e) * VP + 2 * sp;
            *reinterpret_cast<uint16_t*>(dst) = static_cast<uint16_t>(hv[e] & 0xffffu);
            *reinterpret_cast<uint16_t*>(dst + VP) = static_cast<uint16_t>(hv[e] >> 16);
            if constexpr (!BF) {
              *reinterpret_cast<uint16_t*>(dst + VPLANE) = static_cast<uint16_t>(lv[e] & 0xffffu);
              *reinterpret_cast<uint16_t*>(dst + VPLANE + VP) = static_cast<uint16_t>(lv[e] >> 16);
            }
          }
        }
      }
      __syncthreads();
      if (!wave_live) continue;  // wave-uniform; the barriers above are outside

#pragma unroll
      for (int st = 0; st < kKC / 32; ++st) {
        const int ps = p0 + 32 * st;  // first walk position of the step
        if (ps >= L) continue;
        // the wave's queries sit at positions 16 wv s + hwc .. (16 wv + 15) s + hwc, each seeing +- hwc
        if (!capped && (ps > (16 * wv + 15) * s + 2 * hwc || ps + 31 < 16 * wv * s)) continue;

        // ---- S = K . Q: two 16-key tiles
        float sc[2][4];
        float mstep = NEG;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const char* src = Ks + (32 * st + 16 * t + l15) * KP + (32 * ks + 8 * lq) * 2;
            const bf16x8 kh = *reinterpret_cast<const bf16x8*>(src);
            bf16x8 kl = kh;
            if constexpr (!BF) kl = *reinterpret_cast<const bf16x8*>(src + KPLANE);
            acc = mma<BF>(kh, kl, qh[ks], ql[ks], acc);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int p = ps + 16 * t + 4 * lq + i;
            int dist = p - cq;  // in (-1.5 nlon_in, nlon_in)
            dist = dist < 0 ? -dist : dist;
            if (dist >= n) dist -= n;
            dist = dist < n - dist ? dist : n - dist;  // circular
            const bool in = q_ok && p < L && dist <= hwc;
            sc[t][i] = in ? acc[i] * a.scale2 + lw : NEG;
            mstep = fmaxf(mstep, sc[t][i]);
          }
        }
        // ---- online softmax of the query column: the maximum across the four lanes of a query
        mstep = fmaxf(mstep, __shfl_xor(mstep, 16));
        mstep = fmaxf(mstep, __shfl_xor(mstep, 32));
        const float mnew = fmaxf(m, mstep);
        const float msafe = mnew == NEG ? 0.f : mnew;  // every key so far masked: exponents against 0
        const float alpha = __builtin_amdgcn_exp2f(m - msafe);
        m = mnew;
        float pr[8], psum = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            pr[4 * t + i] = __builtin_amdgcn_exp2f(sc[t][i] - msafe);
            psum += pr[4 * t + i];
          }
        lsum = lsum * alpha + psum;
        uint4 ph4, pl4;
        pack8<BF>(pr, ph4, pl4);
        const bf16x8 ph = __builtin_bit_cast(bf16x8, ph4), pl = __builtin_bit_cast(bf16x8, pl4);

        // ---- O = alpha O + V . P: contraction index 8 lq + 4 t + i is key 16 t + 4 lq + i of the step
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          if (16 * rt >= d) continue;
          const char* src = Vs + (16 * rt + l15) * VP + (32 * st + 4 * lq) * 2;
          const uint2 v0 = *reinterpret_cast<const uint2*>(src);
          const uint2 v1 = *reinterpret_cast<const uint2*>(src + 32);
          const bf16x8 vh = frag(v0.x, v0.y, v1.x, v1.y);
          bf16x8 vl = vh;
          if constexpr (!BF) {
            const uint2 w0 = *reinterpret_cast<const uint2*>(src + VPLANE);
            const uint2 w1 = *reinterpret_cast<const uint2*>(src + VPLANE + 32);
            vl = frag(w0.x, w0.y, w1.x, w1.y);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) o[rt][i] *= alpha;
          o[rt] = mma<BF>(vh, vl, ph, pl, o[rt]);
        }
      }
    }
  }

  // ---- epilogue: the sum across the four lanes of a query, one division, one rounding at the store
  if (!wave_live) return;
  lsum += __shfl_xor(lsum, 16);
  lsum += __shfl_xor(lsum, 32);
  const float inv = lsum > 0.f ? 1.f / lsum : 0.f;  // an empty neighbourhood stores 0
  if (!q_ok) return;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 16 * rt + 4 * lq + i;
      if (c >= d) continue;
      const float val = o[rt][i] * inv;
      const int64_t at = out0 + c * plane_out + jq;
      if constexpr (BF) reinterpret_cast<__bf16*>(a.y)[at] = static_cast<__bf16>(val);
      else reinterpret_cast<float*>(a.y)[at] = val;
    }
  }
}

template <bool BF, int DP>
void launch(const Args& a, const AttnS2Route& r, hipStream_t st) {
  hipLaunchKernelGGL((attention_s2_kernel<BF, DP>), dim3(static_cast<uint32_t>(r.wgs)), dim3(kNT),
                     static_cast<size_t>(r.lds), st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: attention_s2: launch: ") + hipGetErrorString(e));
}

}  // namespace

void launch_attention_s2(const AttnS2Launch& p, void* stream) {
  constexpr int64_t k2p31 = int64_t(1) << 31;
  if (p.B <= 0 || p.heads <= 0 || p.nlat_out <= 0 || p.nlon_out <= 0) return;
  if (p.d < 1 || p.d > kAttnS2MaxD)
    throw std::invalid_argument("amd_dft: attention_s2: the head dimension must be 1 .. " +
                                std::to_string(kAttnS2MaxD) + " on the device, got " + std::to_string(p.d));
  if (p.nlat_in < 1 || p.nlon_in < 1 || p.nlon_in % p.nlon_out != 0 || p.nlon_in >= (1 << 24) ||
      p.B * p.heads >= k2p31)
    throw std::invalid_argument("amd_dft: attention_s2: bad launch (nlon_in % nlon_out, sizes)");
  const AttnS2Route r =
      attention_s2_route(p.B, p.heads, p.d, p.nlat_in, p.nlon_in, p.nlat_out, p.nlon_out, p.bf16 != 0);
  if (r.wgs >= k2p31) throw std::invalid_argument("amd_dft: attention_s2: too many workgroups");
  Args a;
  a.q = p.q;
  a.k = p.k;
  a.v = p.v;
  a.hw = p.hw;
  a.logw = p.logw;
  a.y = p.y;
  a.heads_b = static_cast<int>(p.B * p.heads);
  a.d = static_cast<int>(p.d);
  a.nlat_in = p.nlat_in;
  a.nlon_in = p.nlon_in;
  a.nlat_out = p.nlat_out;
  a.nlon_out = p.nlon_out;
  a.s = p.nlon_in / p.nlon_out;
  a.qtiles = static_cast<int>(r.qtiles);
  a.scale2 = p.scale * kLog2e;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (p.bf16) {
    if (r.dp == 32) launch<true, 32>(a, r, st);
    else launch<true, 64>(a, r, st);
  } else {
    if (r.dp == 32) launch<false, 32>(a, r, st);
    else launch<false, 64>(a, r, st);
  }
}

}  // namespace amd_dft

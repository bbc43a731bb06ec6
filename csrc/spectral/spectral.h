// Host interfaces of the fused spectral-layer kernels (no torch dependency).
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

#include "../ops/tuning.h"

namespace amd_dft {

// ---- AFNO: fused FFT_H -> block-diagonal complex MLP (MFMA) -> softshrink -> IFFT_H
struct AfnoLaunch {
  const void* x;        // [B, H, KM, C, 2] fp32/bf16 (W-direction half spectrum, KM kept modes)
  void* y;              // same shape (fp32/bf16)
  int bf16_in = 0, bf16_out = 0;
  int x3 = 0;           // fp32 bf16x3 variant: fp32 in/out, weights [NB][2*BS][hi 2*BS | lo 2*BS]
  const uint16_t* w1t;  // [NB][2*BS][2*BS] bf16, real-block weight transposed ([n][k])
  const uint16_t* w2t;
  const float* b1;      // [NB][2*BS] = [b_re | b_im]
  const float* b2;
  const void* tw;       // FFT plan twiddles for length H
  int r0 = 0, r1 = 0;   // the plan's radix order (must match the instance's two passes)
  int B, H, KM, C, NB;
  float lambda;
};
bool afno_spectral_supported(int H, int block_size);
std::vector<std::pair<int, int>> afno_spectral_shapes();  // instantiated (H, block size) pairs
int64_t afno_spectral_lds_bytes(int H, int block_size, bool x3);
void launch_afno_spectral(const AfnoLaunch& p, void* stream);

// ---- AFNO block-diagonal complex MLP on an already-transformed spectrum (afno_mlp.hip): no H limit,
// the block size is a runtime loop bound
struct AfnoMlpLaunch {
  const float* x;       // [T, C, 2] fp32, (c, re/im) interleaved rows
  float* y;             // same shape
  const uint16_t* w1t;  // [NB][2*BS][2*BS] bf16 ([n][k]), or x3: [NB][2*BS][2 * 2*BS] k32-interleaved hi|lo
  const uint16_t* w2t;
  const float* b1;      // [NB][2*BS] = [b_re | b_im]
  const float* b2;
  int64_t T;            // tokens (rows)
  int C, NB;
  int x3 = 0;           // 3-product bf16 split GEMMs (split weights)
  float lambda;
};
// Which kernel afno_mlp runs (host only; launch_afno_mlp and the afno_mlp_info op both answer from here).
// ok: 16 <= BS <= 256 and BS % 16 == 0 (the split layout's 32-column groups over K = 2 BS).  The token tile
// is the largest of 64 / 32 / 16 rows whose LDS image -- the [tok][2 BS + 8] bf16 operand and hidden
// tiles, hi (and lo) planes each -- stays within 80 KB (two workgroups per CU), halved further while it
// would be at least twice the token count.
constexpr int64_t kAfnoMlpLdsBudget = 80 * 1024;
struct AfnoMlpRoute {
  bool ok;
  const char* why;   // !ok: the reason
  int tok;           // token rows per workgroup
  int ksteps;        // 32-deep k-steps of each GEMM (BS / 16)
  int64_t lds;       // dynamic LDS bytes per workgroup
  int64_t tiles;     // token tiles (workgroups = tiles * NB)
};
inline int64_t afno_mlp_lds_bytes(int bs, bool split, int tok) {
  return 2LL * (split ? 2 : 1) * tok * (2 * bs + 8) * 2;
}
inline AfnoMlpRoute afno_mlp_route(int64_t bs, bool split, int64_t tokens) {
  AfnoMlpRoute r{};
  if (bs < 16 || bs > 256) {
    r.why = "block size outside 16..256";
    return r;
  }
  if (bs % 16 != 0) {
    r.why = "block size is not a multiple of 16";
    return r;
  }
  r.ok = true;
  r.tok = 64;
  while (r.tok > 16 && afno_mlp_lds_bytes(static_cast<int>(bs), split, r.tok) > kAfnoMlpLdsBudget) r.tok /= 2;
  while (r.tok > 16 && r.tok / 2 >= tokens) r.tok /= 2;
  r.ksteps = static_cast<int>(bs / 16);
  r.lds = afno_mlp_lds_bytes(static_cast<int>(bs), split, r.tok);
  r.tiles = tokens > 0 ? (tokens + r.tok - 1) / r.tok : 0;
  return r;
}
void launch_afno_mlp(const AfnoMlpLaunch& p, void* stream);

// ---- FNO: per-mode complex channel mixing out[b,o,m] = sum_i x[b,i,m] * w[i,o,m]
struct FnoMixLaunch {
  const void* x;    // [B, Cin, M, 2] fp32 (bf16 if bf16; M = kept modes, flattened)
  const void* w;    // [Cin, Cout, M, 2] fp32 (bf16 if bf16)
  void* y;          // [B, Cout, M, 2] fp32 (bf16 if bf16)
  int B, Cin, Cout, M;
  int mfma = 0;     // 1: the batched MFMA kernel even for B <= 8 (weights read once per mode tile)
  int bf16 = 0;     // 1: bf16 x, w and y; a (re, im) pair is one 4-byte word, fp32 accumulation, one rounding
};
// Which kernel a call takes (host only; launch_fno_mix and the fno_mix_info op both answer from here).
//   Stream: B <= 8 unless the caller asks for the MFMA kernel -- one lane per (o, m) output, the Cin sum split over
//     the 4 waves of a workgroup; the instance NB = 1 / 2 / 4 / 8 holds the batch in registers.  bf16 with an even M:
//     two modes per lane, so that a lane's loads are 8 bytes as in fp32.
//   Mfma: every other call whose LDS tile fits.  A workgroup owns mt consecutive modes.
//     fp32: mt = 8, tiles X [mt][Bp][Kp], W [mt][Kp][Np], Y [mt][Bp][Np] floats with Bp = ceil16(B), Kp = ceil4(2 Cin),
//       Np = ceil16(2 Cout), within the device's 160 KB.
//     bf16: K-major tiles X [mt][Bp][pitch], W [mt][Np][pitch] with pitch = 2 ceil32(2 Cin) + 16 bytes (the pad keeps
//       the 16-byte fragment reads of 16 consecutive rows off each other's banks) and the packed result
//       Y [mt][Bp][Np / 2] words (each mode's tiles 16 bytes / one word apart from the next).  mt is the largest of 16 / 8 / 4 whose tile stays within 80 KB (two workgroups per
//       CU), halved while the grid would leave CUs without a workgroup; where not even 4 modes fit 80 KB, 4 modes
//       within 160 KB.
//   StreamBatched: the MFMA tile does not fit -- the stream kernel, 8 samples per launch (a call with B <= 8 is then
//     plain Stream, whatever the caller asked for).
constexpr int64_t kFnoMixLdsMax = 160 * 1024;
constexpr int64_t kFnoMixLdsShared = 80 * 1024;
constexpr int64_t kFnoMixFillWgs = 256;
enum class FnoMixKind { Stream, Mfma, StreamBatched };
struct FnoMixRoute {
  FnoMixKind kind;
  int nb;          // stream: the instance (samples held per lane) of the first launch
  int vec;         // stream: modes per lane -- 2 (8-byte loads and stores) for bf16 with an even M and x, w, y on
                   // 8-byte boundaries (aligned), else 1
  int mt;          // mfma: modes per workgroup
  int pitch;       // mfma, bf16: bytes per K-major LDS row
  int64_t lds;     // LDS bytes per workgroup (stream: the static reduction buffer)
  int64_t wgs;     // workgroups per launch
  int launches;
};
inline int64_t fno_mix_lds_f32(int64_t B, int64_t Cin, int64_t Cout) {
  const int64_t K = 2 * Cin, N = 2 * Cout, Kp = (K + 3) & ~int64_t(3), Bp = (B + 15) & ~int64_t(15),
                Np = (N + 15) & ~int64_t(15);
  return 4 * 8 * (Bp * Kp + Kp * Np + Bp * Np);
}
inline int64_t fno_mix_pitch_bf16(int64_t Cin) { return 2 * ((2 * Cin + 31) / 32 * 32) + 16; }
inline int64_t fno_mix_lds_bf16(int64_t B, int64_t Cin, int64_t Cout, int mt) {
  const int64_t Bp = (B + 15) & ~int64_t(15), Np = (2 * Cout + 15) & ~int64_t(15);
  // each mode's x and w tiles are followed by 16 bytes, its result tile by one word (bank spreading over the modes)
  return mt * ((Bp + Np) * fno_mix_pitch_bf16(Cin) + 32 + Bp * Np * 2 + 4);
}
inline FnoMixRoute fno_mix_route(int64_t B, int64_t Cin, int64_t Cout, int64_t M, bool bf16, bool mfma,
                                 bool aligned = true) {
  FnoMixRoute r{};
  int mt = 0;
  int64_t lds = 0;
  if (!bf16) {
    lds = fno_mix_lds_f32(B, Cin, Cout);
    if (lds <= kFnoMixLdsMax) mt = 8;
  } else {
    for (int t = 16; t >= 4 && mt == 0; t /= 2)
      if (fno_mix_lds_bf16(B, Cin, Cout, t) <= kFnoMixLdsShared) mt = t;
    while (mt > 4 && (M + mt - 1) / mt < kFnoMixFillWgs) mt /= 2;
    if (mt == 0 && fno_mix_lds_bf16(B, Cin, Cout, 4) <= kFnoMixLdsMax) mt = 4;
    lds = fno_mix_lds_bf16(B, Cin, Cout, mt);
  }
  if (mt != 0 && (B > 8 || mfma)) {
    r.kind = FnoMixKind::Mfma;
    r.mt = mt;
    r.pitch = bf16 ? static_cast<int>(fno_mix_pitch_bf16(Cin)) : 0;
    r.lds = lds;
    r.wgs = (M + mt - 1) / mt;
    r.launches = 1;
    return r;
  }
  r.kind = B <= 8 ? FnoMixKind::Stream : FnoMixKind::StreamBatched;
  r.nb = B <= 1 ? 1 : B <= 2 ? 2 : B <= 4 ? 4 : 8;
  r.vec = bf16 && M % 2 == 0 && aligned ? 2 : 1;
  r.lds = 3LL * r.nb * 64 * 8 * r.vec;
  r.wgs = (Cout * (M / r.vec) + 63) / 64;
  r.launches = static_cast<int>((B + 7) / 8);
  return r;
}
void launch_fno_mix(const FnoMixLaunch& p, void* stream);

// ---- FNO pointwise epilogue: y[b,o,p] = act(spec[b,o,p] + sum_i w[o,i] x[b,i,p] + bias[o])
struct FnoPointwiseLaunch {
  const void* spec;    // [B, Cout, P] (same dtype as x) or nullptr
  const void* x;       // [B, Cin, P]
  const float* w;      // [Cout, Cin] fp32
  const float* bias;   // [Cout] fp32 or nullptr
  void* y;             // [B, Cout, P]
  int B, Cin, Cout, P;
  int bf16 = 0, gelu = 1;
};
// the register-resident instances of fno_pointwise.hip
inline bool fno_pointwise_fixed(int cin) {
  return cin == 4 || cin == 8 || cin == 16 || cin == 20 || cin == 32 || cin == 64 || cin == 128;
}
void launch_fno_pointwise(const FnoPointwiseLaunch& p, void* stream);
// the MFMA kernel (fno_pointwise_mfma.hip): any Cin, Cout, P; vec = 4-pixel vector I/O
void launch_fno_pointwise_mfma(const FnoPointwiseLaunch& p, bool vec, void* stream);

// Which pointwise kernel a call takes (host only; launch_fno_pointwise and the fno_pointwise_info op
// both answer from here).  The seven register-resident instances keep their channel counts; every
// other Cin >= 1 runs on the MFMA kernel.  aligned: x, y and spec start on a 4-element boundary.
constexpr int kPwSlab = 32;        // input channels per K slab of the MFMA kernel
constexpr int kPwGroupTiles = 4;   // 16-channel output tiles per accumulator group (64 channels)
struct FnoPointwiseRoute {
  bool mfma;    // false: fixed instance of Cin
  int vp;       // pixels per lane-load: 4 (vector I/O) or 1
  int slabs;    // mfma: ceil(Cin / 32) K slabs
  int otiles;   // mfma: ceil(Cout / 16) output tiles
  int groups;   // mfma: ceil(otiles / 4) passes over the x slabs
  bool x3;      // mfma: fp32 I/O, 3-product bf16 split
};
inline FnoPointwiseRoute fno_pointwise_route(int cin, int cout, bool bf16, int64_t P, bool aligned) {
  FnoPointwiseRoute r{};
  // tuning builds: MI_DFT_PW_MFMA=1 sends the fixed channel counts to the MFMA kernel too (A/B runs)
  const char* e = tuning_env("MI_DFT_PW_MFMA");
  r.mfma = !fno_pointwise_fixed(cin) || (e && e[0] == '1');
  const bool vec = P % 4 == 0 && aligned;
  r.vp = vec && (r.mfma || cin <= 32) ? 4 : 1;  // the fixed instances above 32 channels load per element
  if (r.mfma) {
    r.slabs = (cin + kPwSlab - 1) / kPwSlab;
    r.otiles = (cout + 15) / 16;
    r.groups = (r.otiles + kPwGroupTiles - 1) / kPwGroupTiles;
    r.x3 = !bf16;
  }
  return r;
}

// ---- Legendre transform (the latitude half of a spherical harmonic transform, legendre.hip):
//   y[n, r, m, :] = sum_q T[m, r, q] * x[n, q, m, :]      (x complex as trailing re/im, T real, per mode m)
// forward: Q = nlat, R = lmax, T = w_k P_l^m(cos theta_k); inverse: Q = lmax, R = nlat, T = P transposed.
// Its vector form (the latitude half of a vector spherical harmonic transform), over pairs of planes of x:
//   y[n, 0, r, m] = sum_q A[m, r, q] x[n, 0, q, m] - i B[m, r, q] x[n, 1, q, m]
//   y[n, 1, r, m] = sum_q A[m, r, q] x[n, 1, q, m] + i B[m, r, q] x[n, 0, q, m]
struct LegendreLaunch {
  const void* x;       // [N, Q, M, 2] fp32 (bf16 if bf16); vec: [N / 2, 2, Q, M, 2]
  const uint16_t* th;  // [M, Rp, Qp] bf16, hi plane of T (vec: A) zero-padded to Rp = ceil16(R), Qp = ceil32(Q)
  const uint16_t* tl;  // the lo plane, bf16(T - hi); not read if bf16
  const uint16_t* bh = nullptr;  // vec: the same two planes of B
  const uint16_t* bl = nullptr;
  void* y;             // [N, R, M, 2] fp32 (bf16 if bf16); vec: [N / 2, 2, R, M, 2]
  int64_t N;           // [Q, M, 2] planes of x (vec: 2 x fields)
  int Q, R, M;
  int tri = 0;         // 0: dense; 1: rows r < m (of both tables) are zero; 2: columns q < m are zero
  int bf16 = 0;        // 1: bf16 x and y, one plane per table (th = bf16(T)), one MFMA per fragment pair
  int vec = 0;         // 1: the vector form, for launch_legendre_vec
};
// Which tiling a call takes (host only; the launchers and the legendre_info / legendre_vec_info ops answer from here).
// A workgroup (4 waves) owns mt consecutive modes (a wave mt / 4 of them), 8 ct fields n (ct 16-column
// MFMA tiles of the 2 N real columns) and one group of up to 64 rows r; it walks Q in 32-deep slabs.
// The tile starts at 8 modes x 16 fields and shrinks -- first to 4 modes, then to 8 fields -- while the grid
// would leave most of the 256 CUs without a workgroup (or the shape has nothing to fill the larger tile).
// vec: the kernel runs over the component planes -- a 16-column tile is 4 fields x 2 components x (re | im),
// cols = 4 x fields -- so the tiles, the LDS image and the shrink rule are the same: 8 modes x 8 fields, then 4
// modes, then 4 fields.  fp32 vec starts at 4 modes: with two tables in two planes an 8-mode fp32 kernel leaves
// one wave per SIMD (legendre.hip).
constexpr int kLegSlab = 32;        // q per K slab
constexpr int kLegRowTiles = 4;     // 16-row tiles per row group (64 x 16 ct accumulators per mode)
constexpr int kLegXPitch = 80;      // bytes per LDS column of a slab: 32 bf16 + 16 B (conflict-free 16-byte reads)
constexpr int64_t kLegFillWgs = 256;
struct LegendreRoute {
  int mt;          // modes per workgroup: 8 or 4
  int ct;          // 16-column tiles per workgroup: 2 or 1
  int slabs;       // ceil(Q / 32)
  int rtiles;      // ceil(R / 16)
  int rgroups;     // ceil(rtiles / 4) (grid z)
  int mgroups;     // ceil(M / mt)     (grid x)
  int ctiles;      // ceil(cols / (16 ct)) (grid y)
  int64_t lds;     // dynamic LDS bytes per workgroup
  int64_t wgs;     // workgroups
};
inline int64_t legendre_lds_bytes(int mt, int ct, bool bf16 = false) {
  // slab image: 2 planes (bf16: 1) x mt modes x (16 ct columns x 80 B + a pad that spreads the modes over the banks);
  // output image (one 16-row tile, modes innermost): 16 x (8 ct x (2 mt + 2) + 4) floats -- they share the space
  const int64_t xs = (bf16 ? 1LL : 2LL) * mt * (16 * ct * kLegXPitch + 256 / mt);
  const int64_t ys = 16LL * (8 * ct * (2 * mt + 2) + 4) * 4;
  return xs > ys ? xs : ys;
}
inline LegendreRoute legendre_route(int64_t Q, int64_t R, int64_t M, int64_t cols, int /*tri*/, bool bf16 = false,
                                    bool vec = false) {
  LegendreRoute r{};
  r.slabs = static_cast<int>((Q + kLegSlab - 1) / kLegSlab);
  r.rtiles = static_cast<int>((R + 15) / 16);
  r.rgroups = (r.rtiles + kLegRowTiles - 1) / kLegRowTiles;
  auto count = [&](int mt, int ct) { return ((M + mt - 1) / mt) * ((cols + 16 * ct - 1) / (16 * ct)) * r.rgroups; };
  r.mt = vec && !bf16 ? 4 : 8;
  r.ct = 2;
  if (M <= 4 || count(r.mt, r.ct) < kLegFillWgs) r.mt = 4;
  if (cols <= 16 || count(r.mt, r.ct) < kLegFillWgs) r.ct = 1;
  r.mgroups = static_cast<int>((M + r.mt - 1) / r.mt);
  r.ctiles = static_cast<int>((cols + 16 * r.ct - 1) / (16 * r.ct));
  r.lds = legendre_lds_bytes(r.mt, r.ct, bf16);
  r.wgs = count(r.mt, r.ct);
  return r;
}
void launch_legendre(const LegendreLaunch& p, void* stream);
void launch_legendre_vec(const LegendreLaunch& p, void* stream);

// ---- SFNO per-degree channel mixing (sfno_mix.hip):
//   y[b, o, l, m] = sum_i c[b, i, l, m] * w[i, o, l]       (complex; one weight per degree l, shared by all orders m)
struct SfnoMixLaunch {
  const void* c;       // [B, Cin, L, M, 2] fp32 (bf16 if bf16)
  const uint16_t* wh;  // [L, Op, Kp] bf16, hi plane of the real form of w: row o, k = 2 i -> Wr[i, o, l],
                       // k = 2 i + 1 -> Wi[i, o, l], zero-padded to Op = ceil16(Cout), Kp = ceil32(2 Cin)
  const uint16_t* wl;  // the lo plane, bf16(W - hi); not read if bf16
  void* y;             // [B, Cout, L, M, 2] fp32 (bf16 if bf16)
  int B, Cin, Cout, L, M;
  int tri = 0;         // 0: dense; 1: c is zero where l < m -- orders m > l are not read, y is 0.0 there
  int bf16 = 0;        // 1: bf16 c and y, one weight plane (wh = bf16(W)), one MFMA per fragment pair
};
// The tiling of a call (host only; launch_sfno_mix and the sfno_mix_info op both answer from here).  A workgroup
// (4 waves) owns one degree, one group of up to 64 output channels and one tile of 64 complex (128 real) columns;
// the columns of a degree are its live orders flattened over the batch, (b, m) -> b Ml + m with Ml = M, or
// min(M, l + 1) under tri = 1.  One tiling, no fill rule: a degree with fewer columns leaves waves of its last
// tile idle, which skip their loads and MFMAs.  The grid is (column tiles of the fullest degree, groups, L);
// workgroups past a degree's last tile only help store the zeros of l < m.
constexpr int kSfnoSlab = 32;       // k per K slab (16 input channels)
constexpr int kSfnoRowTiles = 4;    // 16-row tiles per output-channel group
constexpr int kSfnoColTile = 64;    // complex columns per workgroup (8 16-column MFMA tiles of real columns)
constexpr int kSfnoXPitch = 80;     // bytes per LDS column of a slab: 32 bf16 + 16 B (conflict-free 16-byte reads)
struct SfnoMixRoute {
  int slabs;       // ceil(2 Cin / 32)
  int otiles;      // ceil(Cout / 16)
  int ogroups;     // ceil(otiles / 4) (grid y)
  int coltile;     // complex columns per workgroup
  int64_t ctiles;  // column tiles of the fullest degree (grid x)
  int64_t lds;     // dynamic LDS bytes per workgroup
  int64_t wgs;     // workgroups with a non-empty column tile (the ones that load and multiply)
  int64_t grid;    // workgroups launched
};
inline int64_t sfno_mix_lds_bytes(bool bf16 = false) { return (bf16 ? 1LL : 2LL) * 2 * kSfnoColTile * kSfnoXPitch; }
inline SfnoMixRoute sfno_mix_route(int64_t B, int64_t Cin, int64_t Cout, int64_t L, int64_t M, int tri,
                                   bool bf16 = false) {
  SfnoMixRoute r{};
  r.slabs = static_cast<int>((2 * Cin + kSfnoSlab - 1) / kSfnoSlab);
  r.otiles = static_cast<int>((Cout + 15) / 16);
  r.ogroups = (r.otiles + kSfnoRowTiles - 1) / kSfnoRowTiles;
  r.coltile = kSfnoColTile;
  auto tiles = [&](int64_t ml) { return (B * ml + kSfnoColTile - 1) / kSfnoColTile; };
  const int64_t full = tri == 1 && L < M ? L : M;  // live orders of the fullest degree
  r.ctiles = tiles(full);
  int64_t live = 0;
  for (int64_t l = 0; l < L; ++l) live += tiles(tri == 1 && l + 1 < M ? l + 1 : M);
  r.lds = sfno_mix_lds_bytes(bf16);
  r.wgs = live * r.ogroups;
  r.grid = r.ctiles * r.ogroups * L;
  return r;
}
void launch_sfno_mix(const SfnoMixLaunch& p, void* stream);

// ---- test support (lds_poison.hip): NaN-fill every CU's LDS, and measure what a following kernel finds there
constexpr uint32_t kLdsPoisonWord = 0x7fc07fc0u;  // a quiet NaN as fp32 and as two bf16
constexpr int kLdsPoisonRounds = 4;                // workgroups per CU
struct LdsPoisonGeo {
  int64_t wgs;      // workgroups launched (CUs x kLdsPoisonRounds)
  int threads;      // threads per workgroup
  int64_t words;    // 32-bit LDS words per workgroup: the largest dynamic LDS the device allows
};
LdsPoisonGeo lds_poison_geometry();                  // of the current device
void launch_lds_poison(void* stream);                // writes no global memory
void launch_lds_probe(int32_t* hits, void* stream);  // hits [wgs * threads]: matching words seen by each thread

// ---- LayerNorm over the last dim (bf16/fp32 I/O, fp32 statistics)
struct LayerNormLaunch {
  const void* x;
  void* y;
  const void* gamma;
  const void* beta;
  const void* residual;  // optional: y = LN(x) ; x_out = x + residual written to resid_out
  void* resid_out;
  int64_t rows;
  int cols;
  float eps;
  int bf16;  // 1: bf16 tensors, 0: fp32 (gamma/beta fp32)
  int split_out = 0;           // fp32 only: y = [rows, 2 cols] bf16 pair rows [hi | lo]
  const float* pre = nullptr;  // fp32 only: per-channel addend applied before the statistics
};
void launch_layernorm(const LayerNormLaunch& p, void* stream);

// The kernel of layernorm.hip a launch runs for a row width (host only; the launchers and the ln_info op both ask
// here).  nch = the instance's 16-byte chunks per lane (Stats768, SplitLds: 3 by construction).  None: no kernel
// takes the width (bf16 rows need cols % 8 == 0, fp32 rows cols % 4 == 0, split rows cols % 32 == 0, all <= 2048;
// a residual needs bf16) and the launchers throw.
enum class LnOp { LayerNorm, LayerNormRes, LnStats, LayerNormSplit };
enum class LnKernel { None, Bf16, Bf16Res, Stats, Stats768, F32, F32Stats, F32Split, SplitLds };
struct LnRoute {
  LnKernel kernel = LnKernel::None;
  int nch = 0;
};
LnRoute ln_route(LnOp op, int64_t cols, bool bf16);
const char* ln_kernel_name(LnKernel k);

// ---- Instance normalisation over the spatial plane of each (batch, channel) of an NCHW tensor (instance_norm.hip):
//   y[p, :] = (x[p, :] - mean_p) * rsqrt(var_p + eps) * w[p % C] + b[p % C],  biased variance over the P elements
struct InstanceNormLaunch {
  const void* x = nullptr;     // [planes, P] fp32 (bf16 if bf16), starting on a 16-byte boundary
  void* y = nullptr;           // same shape and alignment; nullptr: statistics only
  const float* w = nullptr;    // [C] fp32 or nullptr (1)
  const float* b = nullptr;    // [C] fp32 or nullptr (0)
  float* stats = nullptr;      // statistics only: [planes, 2] (mean, rstd)
  float* part = nullptr;       // split route: [planes, S, 4] workspace (count, mean - x[p, 0], M2, unused)
  int64_t planes = 0, P = 0;
  int C = 1;
  float eps = 1e-5f;
  int bf16 = 0;
};
// The route of a call (host only; launch_instance_norm and the instance_norm_info op both answer from here).
// resident: P <= kInMaxLen, the plane fits the LDS image of one workgroup (64 KB with its scratch, so two
// workgroups share a CU) -- one workgroup per plane.  split: every larger plane, in S = ceil(P / chunk) chunks; the
// chunk starts at kInMaxLen elements and halves, down to kInMinChunk, while planes * S would leave fewer than
// kInFillWgs workgroups (four per CU).  Both dtypes share the rule: the LDS image is fp32.
constexpr int kInThreads = 512;
constexpr int kInScratchBytes = 256;                // reduction scratch in front of the LDS image
constexpr int64_t kInMaxLen = 16256;                // elements: 256 + (16256 + 4) * 4 = 65296 bytes <= 64 KB
constexpr int64_t kInMinChunk = kInMaxLen / 8;      // 2032
constexpr int64_t kInFillWgs = 1024;
struct InstanceNormRoute {
  bool resident;
  int64_t S;       // chunks per plane (resident: 1)
  int64_t chunk;   // elements per chunk, the last one of a plane may be shorter (resident: P)
  int vec;         // elements per 16-byte access
  int64_t lds;     // dynamic LDS bytes per workgroup of the kernel that holds the data
  int64_t wgs;     // workgroups per launch: planes * S
};
inline int64_t instance_norm_lds_bytes(int64_t len) { return kInScratchBytes + (len + 4) * 4; }
inline InstanceNormRoute instance_norm_route(int64_t planes, int64_t P, bool bf16) {
  InstanceNormRoute r{};
  r.vec = bf16 ? 8 : 4;
  r.resident = P <= kInMaxLen;
  if (r.resident) {
    r.S = 1;
    r.chunk = P;
  } else {
    r.chunk = kInMaxLen;
    while (r.chunk > kInMinChunk && planes * ((P + r.chunk - 1) / r.chunk) < kInFillWgs) r.chunk /= 2;
    r.S = (P + r.chunk - 1) / r.chunk;
  }
  r.lds = instance_norm_lds_bytes(r.chunk);
  r.wgs = planes * r.S;
  return r;
}
void launch_instance_norm(const InstanceNormLaunch& p, void* stream);

// ---- Discrete-continuous (DISCO) convolution on the sphere, the gather half (disco.hip):
//   y[n, p, k', j'] = sum_e val[e] * x[n, k_e, (d_e + s j') mod nlon_in],  e over CSR row p * nlat_out + k',
//   idx[e] = k_e * nlon_in + d_e sorted within a row, s = nlon_in / nlon_out
struct DiscoLaunch {
  const void* x = nullptr;         // [planes, nlat_in, nlon_in] fp32 (bf16 if bf16), element-aligned
  const int32_t* row_ptr = nullptr;  // [K * nlat_out + 1]
  const int32_t* idx = nullptr;    // [nnz]
  const float* val = nullptr;      // [nnz]
  void* y = nullptr;               // [planes, K, nlat_out, nlon_out], x's dtype
  int64_t planes = 0;
  int nlat_in = 0, nlon_in = 0, K = 0, nlat_out = 0, nlon_out = 0;
  int64_t nnz = 0;
  int bf16 = 0;
};
// The route of a call (host only; launch_disco and the disco_info op both answer from here).  A workgroup of
// kDiscoThreads owns one output latitude and PT planes and holds `rows` input rows of each as fp32 in LDS.  PT = 4
// where four planes of at least kDiscoMinRows rows fit kDiscoLdsBytes and there are four planes, else 1.  The band of
// an output latitude is read from the table by the kernel; where it is taller than `rows` it is walked in chunks.
constexpr int kDiscoThreads = 256;
constexpr int kDiscoItems = 3;                  // outputs per lane and pass
constexpr int64_t kDiscoLdsBytes = 64 * 1024;   // two workgroups per CU
constexpr int kDiscoMinRows = 8;
struct DiscoRoute {
  int pt;          // planes per workgroup: 1 or 4
  int rows;        // input rows per plane in LDS (the chunk)
  int64_t lds;     // dynamic LDS bytes per workgroup
  int64_t ptiles;  // plane tiles
  int64_t wgs;     // nlat_out * ptiles
  int passes;      // ceil(pt * nlon_out / (kDiscoThreads * kDiscoItems))
};
inline DiscoRoute disco_route(int64_t planes, int64_t nlat_in, int64_t nlon_in, int64_t /*K*/, int64_t nlat_out,
                              int64_t nlon_out, int64_t /*nnz_max*/, bool /*bf16*/) {
  DiscoRoute r{};
  const int64_t row = nlon_in * 4;
  r.pt = (planes >= 4 && 4 * kDiscoMinRows * row <= kDiscoLdsBytes) ? 4 : 1;
  int64_t rows = kDiscoLdsBytes / (r.pt * row);
  if (rows < 1) rows = 1;
  if (rows > nlat_in) rows = nlat_in;
  r.rows = static_cast<int>(rows);
  r.lds = r.pt * rows * row;
  r.ptiles = (planes + r.pt - 1) / r.pt;
  r.wgs = nlat_out * r.ptiles;
  r.passes = static_cast<int>((r.pt * nlon_out + kDiscoThreads * kDiscoItems - 1) / (kDiscoThreads * kDiscoItems));
  return r;
}
void launch_disco(const DiscoLaunch& p, void* stream);

// ---- DISCO convolution on the sphere, the transposed (upsampling) half (disco_t.hip): a gather CSR over rows
// r = k * s + rho (output latitude k, longitude phase rho, s = nlon_out / nlon_in),
//   y[n, k, s t + rho] = sum_e val[e] * z[n, p_e, k'_e, (d_e + t) mod nlon_in] (+ bias[n mod C]),  0 <= t < nlon_in,
//   idx[e] = (k'_e * K + p_e) * nlon_in + d_e sorted within a row
struct DiscoTLaunch {
  const void* z = nullptr;           // [planes, K, nlat_in, nlon_in] fp32 (bf16 if bf16), element-aligned
  const int32_t* row_ptr = nullptr;  // [nlat_out * s + 1]
  const int32_t* idx = nullptr;      // [nnz]
  const float* val = nullptr;        // [nnz]
  const float* bias = nullptr;       // [C] or nullptr; plane n takes bias[n mod C]
  void* y = nullptr;                 // [planes, nlat_out, nlon_out], z's dtype
  int64_t planes = 0, C = 1;
  int nlat_in = 0, nlon_in = 0, K = 0, nlat_out = 0, nlon_out = 0;
  int64_t nnz = 0;
  int bf16 = 0;
};
// The route (host only; launch_disco_t and the disco_t_info op both answer from here): disco_route's rule with an
// LDS row of all K basis planes of one input latitude, K * nlon_in * 4 bytes.  A workgroup owns one output latitude,
// all s phases and PT planes; lanes are (plane, t), so a pass covers kDiscoThreads * kDiscoItems of PT * nlon_in.
struct DiscoTRoute {
  int pt;          // planes per workgroup: 1 or 4
  int rows;        // input latitudes per plane in LDS (the chunk), K basis planes each
  int64_t lds;     // dynamic LDS bytes per workgroup
  int64_t ptiles;  // plane tiles
  int64_t wgs;     // nlat_out * ptiles
  int passes;      // ceil(pt * nlon_in / (kDiscoThreads * kDiscoItems)), per phase
  int phases;      // s
};
inline DiscoTRoute disco_t_route(int64_t planes, int64_t nlat_in, int64_t nlon_in, int64_t K, int64_t nlat_out,
                                 int64_t nlon_out, int64_t /*nnz_max*/, bool /*bf16*/) {
  DiscoTRoute r{};
  const int64_t row = K * nlon_in * 4;
  r.pt = (planes >= 4 && 4 * kDiscoMinRows * row <= kDiscoLdsBytes) ? 4 : 1;
  int64_t rows = kDiscoLdsBytes / (r.pt * row);
  if (rows < 1) rows = 1;
  if (rows > nlat_in) rows = nlat_in;
  r.rows = static_cast<int>(rows);
  r.lds = r.pt * rows * row;
  r.ptiles = (planes + r.pt - 1) / r.pt;
  r.wgs = nlat_out * r.ptiles;
  r.passes = static_cast<int>((r.pt * nlon_in + kDiscoThreads * kDiscoItems - 1) / (kDiscoThreads * kDiscoItems));
  r.phases = static_cast<int>(nlon_out / nlon_in);
  return r;
}
void launch_disco_t(const DiscoTLaunch& p, void* stream);

// ---- AFNO W-direction transforms with LayerNorm fused into the IO (afno_wfft.hip)
struct AfnoWLaunch {
  const void* x = nullptr;        // [O, L, C] bf16 (fp32 if f32) stored residual stream
  const float* stats = nullptr;   // [O, L, 2] (mean, rstd) of x + pre
  const float* gamma = nullptr;   // [C] fp32
  const float* beta = nullptr;    // [C] fp32
  const float* pre = nullptr;     // [C] fp32 or nullptr
  const void* spec = nullptr;     // C2R input [O, KM, C, 2] bf16
  void* out = nullptr;            // R2C: [O, KM, C, 2] bf16; C2R: [O, L, C] bf16
  int O = 0, L = 0, C = 0, KM = 0;
  float scale = 1.f;
  int f32 = 0;                    // fp32 residual stream, spectrum and output
  // C2R, fp32 only: also the output's bf16x3 split-pair rows [O*L, 2C] (k32-interleaved, the
  // next GEMM's operand) and its per-64-channel LayerNorm partials [O*L, C/64] (mean, M2)
  uint16_t* pairs = nullptr;
  float* part = nullptr;
  // C2R SPLIT, optional: [O*L, C] bf16 third term of the split, bf16(out - m - (hi + lo)): with the pairs it
  // carries out to ~2^-27 of |out - m| (below fp32 rounding), so the fp32 copy (out) can be skipped
  uint16_t* lo2 = nullptr;
};
bool afno_w_supported(int L, int C, int KM);
// The kernel instance a launch runs, from the flags the launchers dispatch on (host only; the launchers and the
// afno_w_info op both answer from here).  Throws for a combination no instance covers.
enum class AfnoWInstance { R2cBf16, R2cF32, C2rBf16, C2rF32, C2rF32Split, C2rBf16Part };
AfnoWInstance afno_w_instance(bool c2r, bool f32, bool pairs, bool part);
const char* afno_w_instance_name(AfnoWInstance i);
void launch_afno_w_r2c_ln(const AfnoWLaunch& p, void* stream);
void launch_afno_w_c2r_ln(const AfnoWLaunch& p, void* stream);

// ---- LayerNorm statistics only: stats[r] = (mean, rstd) of x[r, :] + pre (bf16 rows)
struct LnStatsLaunch {
  const void* x;       // [rows, cols] bf16
  const float* pre;    // [cols] fp32 or nullptr
  float* stats;        // [rows, 2] fp32
  int64_t rows;
  int cols;
  float eps;
  int f32 = 0;         // x is fp32
};
void launch_ln_stats(const LnStatsLaunch& p, void* stream);
// [rows, nc, 2] per-chunk (mean, M2) partials of chunk width `width` -> [rows, 2] (mean, rstd)
void launch_ln_stats_merge(const float* part, float* stats, int64_t rows, int nc, int width, float eps, void* stream,
                           const float* shift = nullptr);

// ---- fp32 -> bf16 (hi, lo) split pairs for the bf16x3 GEMM: rows -> [rows, 2 cols] [hi | lo],
// else planes [2, n]
void launch_split_bf16(const float* x, uint16_t* y, int64_t n, int cols, bool rows, void* stream);

}  // namespace amd_dft

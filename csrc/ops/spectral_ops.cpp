// Torch op layer for the fused spectral-layer kernels (FourCastNet AFNO, FNO) and the
// fused LayerNorm.  CPU implementations are plain ATen math (reference semantics); the
// CUDA (HIP) implementations launch the hand-written gfx950 kernels.
#include <ATen/ATen.h>
#include <ATen/Parallel.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <ATen/core/dispatch/Dispatcher.h>
#include <torch/library.h>

#include "trace.h"
#include "../spectral/dft_gemm.h"
#include "../spectral/spectral.h"
#include "checks.h"
#include "op_family.h"
#include "plan_cache.h"

namespace amd_dft {
namespace {

// The families with an `_out` op (afno_mlp, fno_mix, fno_pointwise, fno_c2r_pw, legendre, legendre_vec, disco,
// sfno_mix, instance_norm) are described once each, in a struct after their check, reference and launch path;
// op_family.h makes the six backend forms of the description.

// ------------------------------------------------------------------ AFNO spectral filter
// xw [B, H, KM, C, 2] fp32 (W-direction half spectrum), w1t/w2t [NB, 2BS, 2BS] bf16 ([n][k]),
// b1/b2 [NB, 2BS] fp32.  Returns [B, H, KM, C, 2] fp32:
//   IFFT_H( softshrink( ReLU(FFT_H(x) W1' + b1') W2' + b2' ) )   (FFTs unnormalised)
void check_afno(const at::Tensor& xw, const at::Tensor& w1t, const at::Tensor& w2t, const at::Tensor& b1,
                const at::Tensor& b2) {
  TORCH_CHECK(xw.dim() == 5 && xw.size(4) == 2 &&
                  (xw.scalar_type() == at::kFloat || xw.scalar_type() == at::kBFloat16),
              "afno_spectral: x must be [B, H, KM, C, 2] float32 or bfloat16");
  TORCH_CHECK(w1t.dim() == 3, "afno_spectral: bad weight shapes");
  const int64_t NB = w1t.size(0), K = w1t.size(1);
  TORCH_CHECK((w1t.size(2) == K || w1t.size(2) == 2 * K) && w2t.sizes() == w1t.sizes(),
              "afno_spectral: weights must be [NB, 2BS, 2BS] (bf16) or split [NB, 2BS, 2*2BS] (bf16x3, fp32 path)");
  TORCH_CHECK(NB * K == 2 * xw.size(3), "afno_spectral: NB * 2 * block_size must equal 2 * C");
  TORCH_CHECK(b1.sizes() == at::IntArrayRef({NB, K}) && b2.sizes() == b1.sizes(), "afno_spectral: bad bias shapes");
}

at::Tensor afno_spectral_cpu(const at::Tensor& xw, const at::Tensor& w1t, const at::Tensor& w2t, const at::Tensor& b1,
                             const at::Tensor& b2, double lam) {
  check_afno(xw, w1t, w2t, b1, b2);
  const int64_t B = xw.size(0), H = xw.size(1), KM = xw.size(2), C = xw.size(3);
  const int64_t NB = w1t.size(0), BS = C / NB;
  at::Tensor X = at::fft_fft(at::view_as_complex(xw.to(at::kFloat).contiguous()), std::nullopt, 1, "backward");
  at::Tensor Xr = at::view_as_real(X).reshape({B, H, KM, NB, BS, 2});
  at::Tensor A = at::cat({Xr.select(-1, 0), Xr.select(-1, 1)}, -1);  // [..., NB, 2BS]
  at::Tensor W1 = unsplit_k32(w1t, "afno_spectral").transpose(1, 2);  // [NB, k, n]
  at::Tensor W2 = unsplit_k32(w2t, "afno_spectral").transpose(1, 2);
  at::Tensor H1 = at::relu(at::einsum("...bk,bkn->...bn", {A, W1}) + b1);
  at::Tensor O = at::einsum("...bk,bkn->...bn", {H1, W2}) + b2;
  O = at::softshrink(O, lam);
  at::Tensor Oc = at::complex(O.narrow(-1, 0, BS), O.narrow(-1, BS, BS)).reshape({B, H, KM, C});
  at::Tensor Y = at::fft_ifft(Oc, std::nullopt, 1, "forward");
  return at::view_as_real(Y).to(xw.scalar_type()).contiguous();
}

at::Tensor afno_spectral_cuda(const at::Tensor& xw_, const at::Tensor& w1t_, const at::Tensor& w2t_, const at::Tensor& b1_,
                              const at::Tensor& b2_, double lam) {
  check_afno(xw_, w1t_, w2t_, b1_, b2_);
  const c10::DeviceGuard guard(xw_.device());
  at::Tensor xw = xw_.contiguous();
  at::Tensor w1t = w1t_.to(at::kBFloat16).contiguous(), w2t = w2t_.to(at::kBFloat16).contiguous();
  at::Tensor b1 = b1_.to(at::kFloat).contiguous(), b2 = b2_.to(at::kFloat).contiguous();
  const int64_t B = xw.size(0), H = xw.size(1), KM = xw.size(2), C = xw.size(3), NB = w1t.size(0);
  TORCH_CHECK(afno_spectral_supported(static_cast<int>(H), static_cast<int>(C / NB)),
              "afno_spectral: no fused instance for H = ", H, ", block size ", C / NB,
              " (afno_spectral_shapes() lists them; use the generic path)");
  const bool x3 = w1t.size(2) == 2 * w1t.size(1);
  TORCH_CHECK(!x3 || xw.scalar_type() == at::kFloat, "afno_spectral: split (bf16x3) weights go with a float32 spectrum");
  at::Tensor y = at::empty_like(xw);
  if (xw.numel() == 0) return y;
  auto dp = get_plan(H, xw.device());
  AfnoLaunch p;
  p.x3 = x3 ? 1 : 0;
  p.x = xw.data_ptr();
  p.y = y.data_ptr();
  p.bf16_in = p.bf16_out = xw.scalar_type() == at::kBFloat16;
  p.w1t = reinterpret_cast<const uint16_t*>(w1t.data_ptr());
  p.w2t = reinterpret_cast<const uint16_t*>(w2t.data_ptr());
  p.b1 = b1.data_ptr<float>();
  p.b2 = b2.data_ptr<float>();
  p.tw = dp->tw.data_ptr();
  TORCH_CHECK(dp->plan.radices.size() == 2, "afno_spectral: H = ", H, " is not a two-pass plan");
  p.r0 = dp->plan.radices[0];
  p.r1 = dp->plan.radices[1];
  p.B = static_cast<int>(B);
  p.H = static_cast<int>(H);
  p.KM = static_cast<int>(KM);
  p.C = static_cast<int>(C);
  p.NB = static_cast<int>(NB);
  p.lambda = static_cast<float>(lam);
  launch_afno_spectral(p, current_stream(xw));
  return checked(y, "afno_spectral");
}

std::vector<int64_t> afno_spectral_shape_list() {  // flattened (H, block size) pairs
  std::vector<int64_t> v;
  for (const auto& hb : afno_spectral_shapes()) {
    v.push_back(hb.first);
    v.push_back(hb.second);
  }
  return v;
}

bool afno_spectral_ok(int64_t H, int64_t block_size) {
  return afno_spectral_supported(static_cast<int>(H), static_cast<int>(block_size));
}

// ------------------------------------------------------------------ AFNO block MLP on a transformed spectrum
// x [..., C, 2] fp32 (any leading dims: the kept modes), weights / biases as afno_spectral.  Returns the same
// shape:  softshrink( ReLU([xr|xi] W1' + b1') W2' + b2' )  per token and channel block, stored interleaved.
// afno_mlp_out writes into a given contiguous fp32 tensor of x's shape.
void check_afno_mlp(const at::Tensor& x, const at::Tensor& w1t, const at::Tensor& w2t, const at::Tensor& b1,
                    const at::Tensor& b2) {
  TORCH_CHECK(x.dim() >= 2 && x.size(-1) == 2 && x.scalar_type() == at::kFloat,
              "afno_mlp: x must be [..., C, 2] float32");
  TORCH_CHECK(w1t.dim() == 3, "afno_mlp: bad weight shapes");
  const int64_t NB = w1t.size(0), K = w1t.size(1);
  TORCH_CHECK((w1t.size(2) == K || w1t.size(2) == 2 * K) && w2t.sizes() == w1t.sizes(),
              "afno_mlp: weights must be [NB, 2BS, 2BS] (bf16) or split [NB, 2BS, 2*2BS] (bf16x3)");
  TORCH_CHECK(NB >= 1 && K >= 2 && K % 2 == 0 && NB * K == 2 * x.size(-2),
              "afno_mlp: NB * 2 * block_size must equal 2 * C");
  TORCH_CHECK(b1.sizes() == at::IntArrayRef({NB, K}) && b2.sizes() == b1.sizes(), "afno_mlp: bad bias shapes");
}

at::Tensor afno_mlp_ref(const at::Tensor& x, const at::Tensor& w1t, const at::Tensor& w2t, const at::Tensor& b1,
                        const at::Tensor& b2, double lam) {
  const int64_t C = x.size(-2), NB = w1t.size(0), BS = C / NB;
  at::Tensor Xr = x.contiguous().reshape({-1, NB, BS, 2});
  at::Tensor A = at::cat({Xr.select(-1, 0), Xr.select(-1, 1)}, -1);  // [T, NB, 2BS]
  at::Tensor W1 = unsplit_k32(w1t, "afno_mlp").transpose(1, 2), W2 = unsplit_k32(w2t, "afno_mlp").transpose(1, 2);
  at::Tensor H1 = at::relu(at::einsum("tbk,bkn->tbn", {A, W1}) + b1.to(at::kFloat));  // W1, W2 [NB, k, n]
  at::Tensor O = at::softshrink(at::einsum("tbk,bkn->tbn", {H1, W2}) + b2.to(at::kFloat), lam);
  return at::stack({O.narrow(-1, 0, BS), O.narrow(-1, BS, BS)}, -1).reshape(x.sizes()).contiguous();
}

// the launch path of afno_mlp and afno_mlp_out: y is the contiguous fp32 result, 16-byte aligned
void afno_mlp_run(const at::Tensor& x_, const at::Tensor& w1t_, const at::Tensor& w2t_, const at::Tensor& b1_,
                  const at::Tensor& b2_, double lam, const at::Tensor& y) {
  // 16-byte loads of two channels' (re, im): a view at an odd offset gets its own copy
  at::Tensor x = aligned_to(x_.contiguous(), 16);
  at::Tensor w1t = w1t_.to(at::kBFloat16).contiguous(), w2t = w2t_.to(at::kBFloat16).contiguous();
  at::Tensor b1 = b1_.to(at::kFloat).contiguous(), b2 = b2_.to(at::kFloat).contiguous();
  const int64_t C = x.size(-2), NB = w1t.size(0), BS = C / NB;
  const bool x3 = w1t.size(2) == 2 * w1t.size(1);
  const int64_t T = x.numel() / (2 * C);
  const AfnoMlpRoute r = afno_mlp_route(BS, x3, T);
  TORCH_CHECK(r.ok, "afno_mlp: no kernel for block size ", BS, " (", r.why ? r.why : "", "); use the generic path");
  TORCH_CHECK(C < (1 << 28), "afno_mlp: channel count too large");
  if (T == 0) return;
  AfnoMlpLaunch p;
  p.x = x.data_ptr<float>();
  p.y = y.data_ptr<float>();
  p.w1t = reinterpret_cast<const uint16_t*>(w1t.data_ptr());
  p.w2t = reinterpret_cast<const uint16_t*>(w2t.data_ptr());
  p.b1 = b1.data_ptr<float>();
  p.b2 = b2.data_ptr<float>();
  p.T = T;
  p.C = static_cast<int>(C);
  p.NB = static_cast<int>(NB);
  p.x3 = x3 ? 1 : 0;
  p.lambda = static_cast<float>(lam);
  launch_afno_mlp(p, current_stream(x));
}

struct AfnoMlp : OpFamily {
  using Sig = at::Tensor(const at::Tensor&, const at::Tensor&, const at::Tensor&, const at::Tensor&, const at::Tensor&,
                         double);
  static constexpr const char *name = "afno_mlp", *out_name = "afno_mlp_out";
  static void check(const char*, const at::Tensor& x, const at::Tensor& w1t, const at::Tensor& w2t,
                    const at::Tensor& b1, const at::Tensor& b2, double) {
    check_afno_mlp(x, w1t, w2t, b1, b2);
  }
  template <class... A>
  static OpResult result(const at::Tensor& x, const A&...) {
    return {x.sizes(), x.options()};
  }
  template <class... A>
  static uintptr_t out_align(const A&...) {
    return 16;
  }
  static constexpr auto& reference = afno_mlp_ref;
  static constexpr auto& run = afno_mlp_run;
};
AMD_DFT_OP_FAMILY(afno_mlp, AfnoMlp)

// Which kernel afno_mlp runs for (block size, packing, tokens) -- host only, no device (the companion of
// fno_pointwise_info): "mfma TOK=32 ksteps=6 x3=1 lds=51200 tiles=512" or "none <reason>"
std::string afno_mlp_info(int64_t block_size, bool split, int64_t tokens) {
  TORCH_CHECK(tokens >= 0, "amd_dft.afno_mlp_info: tokens must be >= 0");
  const AfnoMlpRoute r = afno_mlp_route(block_size, split, tokens);
  if (!r.ok) return std::string("none ") + r.why;
  return "mfma TOK=" + std::to_string(r.tok) + " ksteps=" + std::to_string(r.ksteps) + " x3=" +
         std::to_string(split ? 1 : 0) + " lds=" + std::to_string(r.lds) + " tiles=" + std::to_string(r.tiles);
}

// ------------------------------------------------------------------ FNO mode mixing
// x [B, Cin, M, 2], w [Cin, Cout, M, 2] -> y [B, Cout, M, 2]:   y[b, o, m] = sum_i x[b, i, m] w[i, o, m]   (complex)
// dtype rule: x and w both bfloat16 -> the bf16 kernels and a bf16 result (bf16 operands as they are, fp32
// accumulation, one rounding); every other combination is upcast to fp32, runs the fp32 kernels and returns fp32.
void check_fno_mix(const at::Tensor& x, const at::Tensor& w) {
  TORCH_CHECK(x.dim() == 4 && x.size(3) == 2 && w.dim() == 4 && w.size(3) == 2 && w.size(0) == x.size(1) &&
                  w.size(2) == x.size(2),
              "fno_mix: x [B, Cin, M, 2], w [Cin, Cout, M, 2]");
}
bool fno_mix_bf16(const at::Tensor& x, const at::Tensor& w) {
  return x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16;
}

at::Tensor fno_mix_ref(const at::Tensor& x, const at::Tensor& w, int64_t /*path*/) {
  at::Tensor xc = at::view_as_complex(x.to(at::kFloat).contiguous());
  at::Tensor wc = at::view_as_complex(w.to(at::kFloat).contiguous());
  at::Tensor y = at::view_as_real(at::einsum("bim,iom->bom", {xc, wc})).contiguous();
  return fno_mix_bf16(x, w) ? y.to(at::kBFloat16) : y;  // the product of the upcast operands, rounded once
}

// the launch path of fno_mix and fno_mix_out: y is the contiguous result, aligned to one (re, im) pair (8 bytes fp32,
// 4 bytes bf16: the kernels' stores).  path: 0 = auto (the split-K stream kernel for B <= 8, the MFMA kernel above),
// 2 = the MFMA kernel at any B; fno_mix_route (spectral.h) decides.
void fno_mix_run(const at::Tensor& x_, const at::Tensor& w_, int64_t path, const at::Tensor& y) {
  const bool bf16 = fno_mix_bf16(x_, w_);
  const int64_t B = x_.size(0), Cin = x_.size(1), M = x_.size(2), Cout = w_.size(1);
  TORCH_CHECK(B < (1 << 30) && Cin < (1 << 28) && Cout < (1 << 28) && M < (int64_t(1) << 31) &&
                  Cout * M < (int64_t(1) << 37),
              "fno_mix: tensor too large");
  const at::ScalarType dt = bf16 ? at::kBFloat16 : at::kFloat;
  // one load per (re, im) pair: a view at an odd element offset gets its own copy
  const uintptr_t al = bf16 ? 4 : 8;
  at::Tensor x = aligned_to(x_.to(dt).contiguous(), al), w = aligned_to(w_.to(dt).contiguous(), al);
  if (y.numel() == 0) return;
  FnoMixLaunch p;
  p.x = x.data_ptr();
  p.w = w.data_ptr();
  p.y = y.data_ptr();
  p.B = static_cast<int>(B);
  p.Cin = static_cast<int>(Cin);
  p.Cout = static_cast<int>(Cout);
  p.M = static_cast<int>(M);
  p.mfma = path == 2 ? 1 : 0;
  p.bf16 = bf16 ? 1 : 0;
  launch_fno_mix(p, current_stream(x));
}

struct FnoMix : OpFamily {
  using Sig = at::Tensor(const at::Tensor&, const at::Tensor&, int64_t);
  static constexpr const char *name = "fno_mix", *out_name = "fno_mix_out";
  static void check(const char*, const at::Tensor& x, const at::Tensor& w, int64_t) { check_fno_mix(x, w); }
  static void check_device(const char* op, const at::Tensor& x, const at::Tensor& w, int64_t) {
    TORCH_CHECK(w.device() == x.device(), op, ": w must be on the device of x");
  }
  static OpResult result(const at::Tensor& x, const at::Tensor& w, int64_t) {  // dtype by the rule above, on x's device
    return {{x.size(0), w.size(1), x.size(2), 2}, x.options().dtype(fno_mix_bf16(x, w) ? at::kBFloat16 : at::kFloat)};
  }
  static uintptr_t out_align(const at::Tensor& x, const at::Tensor& w, int64_t) { return fno_mix_bf16(x, w) ? 4 : 8; }
  static constexpr auto& reference = fno_mix_ref;
  static constexpr auto& run = fno_mix_run;
};
AMD_DFT_OP_FAMILY(fno_mix, FnoMix)

// Which kernel fno_mix runs for (B, Cin, Cout, M, dtype, path) -- host only, no device (the companion of
// sfno_mix_info): "stream NB=4 vec=1 lds=6144 wgs=640 launches=1", "mfma MT=8 lds=151552 wgs=256 launches=1" or
// "stream-batched NB=8 vec=1 lds=12288 wgs=8 launches=2"; bf16: the bf16 instances' route (vec=2: two modes per lane,
// what an even M runs when x, w and the result start on 8-byte boundaries) with a trailing " bf16=1"
std::string fno_mix_info(int64_t B, int64_t Cin, int64_t Cout, int64_t M, bool bf16, int64_t path) {
  TORCH_CHECK(B >= 1 && Cin >= 1 && Cout >= 1 && M >= 1 && B < (1 << 30) && Cin < (1 << 28) && Cout < (1 << 28) &&
                  M < (int64_t(1) << 31) && Cout * M < (int64_t(1) << 37),
              "amd_dft.fno_mix_info: B, Cin, Cout, M must be >= 1 (and the tensor within the op's limits)");
  const FnoMixRoute r = fno_mix_route(B, Cin, Cout, M, bf16, path == 2);
  std::string s = r.kind == FnoMixKind::Mfma ? "mfma MT=" + std::to_string(r.mt)
                                             : std::string(r.kind == FnoMixKind::Stream ? "stream" : "stream-batched") +
                                                   " NB=" + std::to_string(r.nb) + " vec=" + std::to_string(r.vec);
  return s + " lds=" + std::to_string(r.lds) + " wgs=" + std::to_string(r.wgs) +
         " launches=" + std::to_string(r.launches) + (bf16 ? " bf16=1" : "");
}

// ------------------------------------------------------------------ FNO pointwise epilogue
// y = act(spec + conv1x1(x, w) + bias); x [B, Cin, *S], spec [B, Cout, *S] (or None), w [Cout, Cin(,1,1)]
at::Tensor fno_pointwise_ref(const c10::optional<at::Tensor>& spec, const at::Tensor& x, const at::Tensor& w,
                             const c10::optional<at::Tensor>& bias, bool gelu) {
  TORCH_CHECK(x.dim() >= 2, "fno_pointwise: x [B, Cin, ...]");
  const int64_t B = x.size(0), Cin = x.size(1);
  at::Tensor w2 = w.reshape({w.size(0), -1}).to(at::kFloat);
  TORCH_CHECK(w2.size(1) == Cin, "fno_pointwise: weight must be [Cout, Cin]");
  at::Tensor xf = x.to(at::kFloat).reshape({B, Cin, -1});
  at::Tensor y = at::einsum("oi,bip->bop", {w2, xf});
  if (present(bias)) y = y + bias->to(at::kFloat).reshape({1, -1, 1});
  if (present(spec)) y = y + spec->to(at::kFloat).reshape({B, w2.size(0), -1});
  if (gelu) y = at::gelu(y);
  std::vector<int64_t> shape = x.sizes().vec();
  shape[1] = w2.size(0);
  return y.reshape(shape).to(x.scalar_type());
}

// the launch path of fno_pointwise and fno_pointwise_out: y is the contiguous [B, Cout, ...] result in x's dtype
void fno_pointwise_run(const c10::optional<at::Tensor>& spec_, const at::Tensor& x_, const at::Tensor& w,
                       const c10::optional<at::Tensor>& bias, bool gelu, const at::Tensor& y) {
  TORCH_CHECK(x_.dim() >= 2, "fno_pointwise: x [B, Cin, ...]");
  TORCH_CHECK(x_.scalar_type() == at::kFloat || x_.scalar_type() == at::kBFloat16,
              "fno_pointwise: x must be float32 or bfloat16");
  const int64_t B = x_.size(0), Cin = x_.size(1);
  const int64_t P = x_.numel() / std::max<int64_t>(B * Cin, 1);
  at::Tensor w2 = w.reshape({w.size(0), -1}).to(at::kFloat).contiguous();
  TORCH_CHECK(w2.size(1) == Cin, "fno_pointwise: weight must be [Cout, Cin]");
  const int64_t Cout = w2.size(0);
  // any channel counts: fno_pointwise_route picks the register-resident instance or the MFMA kernel
  TORCH_CHECK(Cin >= 1 && Cin < (1 << 20) && Cout < (1 << 20), "fno_pointwise: bad channel count ", Cin, " -> ", Cout);
  TORCH_CHECK(P < (int64_t(1) << 31) / 4 && B <= 65535, "fno_pointwise: tensor too large");
  at::Tensor x = x_.contiguous();
  at::Tensor spec;
  if (present(spec_)) {
    TORCH_CHECK(spec_->numel() == B * Cout * P, "fno_pointwise: spec must be [B, Cout, ...] like the output");
    spec = spec_->to(x.scalar_type()).contiguous();
  }
  at::Tensor bf = f32_or_undef(bias);
  FnoPointwiseLaunch p;
  p.spec = spec.defined() ? spec.data_ptr() : nullptr;
  p.x = x.data_ptr();
  p.w = w2.data_ptr<float>();
  p.bias = bf.defined() ? bf.data_ptr<float>() : nullptr;
  p.y = y.data_ptr();
  p.B = static_cast<int>(B);
  p.Cin = static_cast<int>(Cin);
  p.Cout = static_cast<int>(Cout);
  p.P = static_cast<int>(P);
  p.bf16 = x.scalar_type() == at::kBFloat16;
  p.gelu = gelu;
  launch_fno_pointwise(p, current_stream(x));
}

// no check beyond result's (the reference and the launch path make their own) and no out_align: out starts at any
// element -- the kernels fall to per-element I/O off the 4-element boundary
struct FnoPointwise : OpFamily {
  using Sig = at::Tensor(const c10::optional<at::Tensor>&, const at::Tensor&, const at::Tensor&,
                         const c10::optional<at::Tensor>&, bool);
  static constexpr const char *name = "fno_pointwise", *out_name = "fno_pointwise_out";
  template <class... A>
  static OpResult result(const c10::optional<at::Tensor>&, const at::Tensor& x, const at::Tensor& w, const A&...) {
    TORCH_CHECK(x.dim() >= 2 && w.dim() >= 1, "fno_pointwise: x [B, Cin, ...], w [Cout, Cin]");
    OpResult r(x.sizes(), x.options());
    r.shape[1] = w.size(0);
    return r;
  }
  static constexpr auto& reference = fno_pointwise_ref;
  static constexpr auto& run = fno_pointwise_run;
};
AMD_DFT_OP_FAMILY(fno_pointwise, FnoPointwise)

// Which kernel fno_pointwise runs for (Cin, Cout, dtype, P) on aligned tensors -- host only, no device
// (the companion of fft_pass_info): "fixed cin=20 vp=4" or "mfma slabs=2 otiles=3 groups=1 x3=1 vp=4"
std::string fno_pointwise_info(int64_t cin, int64_t cout, bool bf16, int64_t P) {
  TORCH_CHECK(cin >= 1 && cin < (1 << 20) && cout >= 1 && cout < (1 << 20) && P >= 1,
              "amd_dft.fno_pointwise_info: cin, cout, P must be >= 1");
  const FnoPointwiseRoute r = fno_pointwise_route(static_cast<int>(cin), static_cast<int>(cout), bf16, P, true);
  if (!r.mfma) return "fixed cin=" + std::to_string(cin) + " vp=" + std::to_string(r.vp);
  return "mfma slabs=" + std::to_string(r.slabs) + " otiles=" + std::to_string(r.otiles) +
         " groups=" + std::to_string(r.groups) + " x3=" + std::to_string(r.x3 ? 1 : 0) + " vp=" + std::to_string(r.vp);
}

// ------------------------------------------------------------------ FNO layer tail (C2R-W + pointwise)
// yw [B, Cout, H, m, 2] fp32 (inverse-H-transformed kept modes, carrying the 1/(H W) scale),
// x [B, Cin, H, W] -> y [B, Cout, H, W] = act(irfft_W(yw) + conv1x1(x, wc) + bias), dtype of x.
void check_fno_c2r(const at::Tensor& yw, const at::Tensor& x, const at::Tensor& wc) {
  TORCH_CHECK(x.dim() == 4 && yw.dim() == 5 && yw.size(4) == 2, "fno_c2r_pw: yw [B, Cout, H, m, 2], x [B, Cin, H, W]");
  TORCH_CHECK(yw.size(0) == x.size(0) && yw.size(2) == x.size(2), "fno_c2r_pw: batch / H mismatch");
  TORCH_CHECK(wc.numel() == yw.size(1) * x.size(1), "fno_c2r_pw: wc must be [Cout, Cin]");
  TORCH_CHECK(2 * (yw.size(3) - 1) <= x.size(3), "fno_c2r_pw: more modes than the half spectrum");
}

at::Tensor fno_c2r_pw_ref(const at::Tensor& yw, const at::Tensor& x, const at::Tensor& wc,
                          const c10::optional<at::Tensor>& bias, bool gelu) {
  const int64_t W = x.size(3), m = yw.size(3);
  at::Tensor full = at::zeros({yw.size(0), yw.size(1), yw.size(2), W / 2 + 1}, yw.options().dtype(at::kComplexDouble));
  full.narrow(3, 0, m).copy_(at::view_as_complex(yw.to(at::kDouble).contiguous()));
  at::Tensor spec = at::fft_irfft(full, W, 3, "forward").to(at::kFloat);
  return fno_pointwise_ref(spec, x, wc.reshape({yw.size(1), x.size(1)}), bias, gelu);
}

// shapes outside both fused kernels (m > 64, W % 8 != 0, a rotation table beyond LDS): C2R on the FFT kernels
at::Tensor fno_tail_c2r(const at::Tensor& yw, int64_t W, at::ScalarType dt) {
  static auto c2r = c10::Dispatcher::singleton()
                        .findSchemaOrThrow("amd_dft::c2r", "")
                        .typed<at::Tensor(const at::Tensor&, at::IntArrayRef, at::IntArrayRef, double, at::IntArrayRef,
                                          std::optional<at::ScalarType>)>();
  const std::vector<int64_t> dim{3}, out_size{W};
  return c2r.call(yw.to(at::kFloat).contiguous(), dim, out_size, 1.0, {}, dt);
}

// the one launch of the fused tail kernels, narrow or wide (Cin or Cout > 32: fno_c2r_pw_wide.hip, 64-pixel chunks):
// y = act(irfft_W(yw) + conv1x1(x, wc) + bias) in y's dtype; x and wc null: the spectral part alone (fno_c2r, Cin = 0)
void fno_tail_launch(bool wide, const at::Tensor& yw_, const at::Tensor* x_, const at::Tensor* wc_,
                     const c10::optional<at::Tensor>& bias, bool gelu, const at::Tensor& y) {
  const int64_t Cin = x_ ? x_->size(1) : 0, Cout = y.size(1), W = y.size(3), m = yw_.size(3);
  const bool bf16 = y.scalar_type() == at::kBFloat16;
  // the tail kernel reads 4 modes per 16-byte load: a view at an odd float2 offset gets its own copy
  at::Tensor yw = aligned_to(yw_.to(at::kFloat).contiguous(), 16);
  at::Tensor x, wc, bf = f32_or_undef(bias);
  if (x_) {
    x = x_->contiguous();
    wc = wc_->to(at::kFloat).reshape({Cout, Cin}).contiguous();
  }
  auto tabs = get_dft_gemm_tables(bf16 && !wide ? DftTable::C2R_BF16 : DftTable::C2R_F32, static_cast<int>(W),
                                  static_cast<int>(m), y.device());
  FnoC2RPwLaunch p;
  p.yw = yw.data_ptr();
  p.x = x_ ? x.data_ptr() : nullptr;
  p.wc = x_ ? wc.data_ptr<float>() : nullptr;
  p.bias = bf.defined() ? bf.data_ptr<float>() : nullptr;
  p.y = y.data_ptr();
  p.g0 = tabs.first.data_ptr();
  p.rot = tabs.second.data_ptr();
  p.B = static_cast<int>(y.size(0));
  p.Cin = static_cast<int>(Cin);
  p.Cout = static_cast<int>(Cout);
  p.H = static_cast<int>(y.size(2));
  p.W = static_cast<int>(W);
  p.m = static_cast<int>(m);
  p.bf16 = bf16;
  p.gelu = gelu;
  if (wide) launch_fno_c2r_pw_wide(p, current_stream(y));
  else launch_fno_c2r_pw(p, current_stream(y));
}

// the launch path of fno_c2r_pw and fno_c2r_pw_out: y is the contiguous [B, Cout, H, W] result in x's dtype
void fno_c2r_pw_run(const at::Tensor& yw, const at::Tensor& x, const at::Tensor& wc,
                    const c10::optional<at::Tensor>& bias, bool gelu, const at::Tensor& y) {
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16,
              "fno_c2r_pw: x must be float32 or bfloat16");
  const int64_t Cin = x.size(1), W = x.size(3), Cout = yw.size(1), m = yw.size(3);
  const FnoTailRoute route = fno_c2r_pw_route(static_cast<int>(Cin), static_cast<int>(Cout), static_cast<int>(m),
                                              static_cast<int>(W), x.scalar_type() == at::kBFloat16);
  if (route.kind == FnoTailKind::Split)  // + the pointwise kernel, which takes any channel counts (fno_pointwise_route)
    return fno_pointwise_run(fno_tail_c2r(yw, W, x.scalar_type()), x, wc.reshape({Cout, Cin}), bias, gelu, y);
  TORCH_CHECK(x.numel() < (int64_t(1) << 31) && y.numel() < (int64_t(1) << 31), "fno_c2r_pw: tensor too large");
  fno_tail_launch(route.kind == FnoTailKind::Wide, yw, &x, &wc, bias, gelu, y);
}

struct FnoC2rPw : OpFamily {
  using Sig = at::Tensor(const at::Tensor&, const at::Tensor&, const at::Tensor&, const c10::optional<at::Tensor>&,
                         bool);
  static constexpr const char *name = "fno_c2r_pw", *out_name = "fno_c2r_pw_out";
  template <class... A>
  static void check(const char*, const at::Tensor& yw, const at::Tensor& x, const at::Tensor& wc, const A&...) {
    check_fno_c2r(yw, x, wc);
  }
  template <class... A>
  static OpResult result(const at::Tensor& yw, const at::Tensor& x, const A&...) {
    return {{x.size(0), yw.size(1), x.size(2), x.size(3)}, x.options()};
  }
  template <class... A>
  static uintptr_t out_align(const A&...) {  // the store width of both fused kernels in either dtype
    return 16;
  }
  static constexpr auto& reference = fno_c2r_pw_ref;
  static constexpr auto& run = fno_c2r_pw_run;
};
AMD_DFT_OP_FAMILY(fno_c2r_pw, FnoC2rPw)

// Which route fno_c2r_pw (cin >= 1) or fno_c2r (cin = 0) takes for a shape -- host only, no device (the
// companion of fno_pointwise_info): "fused ks=2 co=2 chunk=128", "wide slabs=2 otiles=4 groups=1 ks=2 chunk=64
// x3=0 wl=1" (wl: the 1x1 weights staged in LDS, the kernel's WL instances) or "split"
std::string fno_c2r_pw_info(int64_t cin, int64_t cout, int64_t m, int64_t W, bool bf16) {
  TORCH_CHECK(cin >= 0 && cin < (1 << 20) && cout >= 1 && cout < (1 << 20) && m >= 1 && W >= 1 &&
                  W < (int64_t(1) << 31) && m < (int64_t(1) << 31),
              "amd_dft.fno_c2r_pw_info: cin must be >= 0 and cout, m, W >= 1");
  const FnoTailRoute r = fno_c2r_pw_route(static_cast<int>(cin), static_cast<int>(cout), static_cast<int>(m),
                                          static_cast<int>(W), bf16);
  if (r.kind == FnoTailKind::Fused)
    return "fused ks=" + std::to_string(r.ks) + " co=" + std::to_string(r.co) + " chunk=" + std::to_string(r.chunk);
  if (r.kind == FnoTailKind::Wide)
    return "wide slabs=" + std::to_string(r.slabs) + " otiles=" + std::to_string(r.otiles) +
           " groups=" + std::to_string(r.groups) + " ks=" + std::to_string(r.ks) + " chunk=" + std::to_string(r.chunk) +
           " x3=" + std::to_string(r.x3 ? 1 : 0) + " wl=" + std::to_string(r.wl ? 1 : 0);
  return "split";
}

// ------------------------------------------------------------------ SpectralConv2d tail (C2R-W only)
// yw [B, Cout, H, m, 2] fp32 (inverse-H-transformed kept modes, carrying the 1/(H W) scale) ->
// y [B, Cout, H, W] = irfft_W(yw) in out_dtype (float32 default, or bfloat16): the fno_c2r_pw kernel
// without its pointwise branch (no x read, no 1x1 conv, no activation) -- the classic FNO
// SpectralConv2d ends here (BASELINE config 3: rfft2 -> complex mul -> irfft2).
at::ScalarType fno_c2r_dtype(const at::Tensor& yw, int64_t W, const std::optional<at::ScalarType>& out_dtype) {
  TORCH_CHECK(yw.dim() == 5 && yw.size(4) == 2, "fno_c2r: yw must be [B, Cout, H, m, 2]");
  TORCH_CHECK(W >= 1 && 2 * (yw.size(3) - 1) <= W, "fno_c2r: more modes than the half spectrum of W");
  const at::ScalarType dt = out_dtype.has_value() ? *out_dtype : at::kFloat;
  TORCH_CHECK(dt == at::kFloat || dt == at::kBFloat16, "fno_c2r: out_dtype must be float32 or bfloat16");
  return dt;
}

at::Tensor fno_c2r_cpu(const at::Tensor& yw, int64_t W, std::optional<at::ScalarType> out_dtype) {
  const at::ScalarType dt = fno_c2r_dtype(yw, W, out_dtype);
  const int64_t m = yw.size(3);
  at::Tensor full = at::zeros({yw.size(0), yw.size(1), yw.size(2), W / 2 + 1}, yw.options().dtype(at::kComplexDouble));
  full.narrow(3, 0, m).copy_(at::view_as_complex(yw.to(at::kDouble).contiguous()));
  return at::fft_irfft(full, W, 3, "forward").to(dt);
}

at::Tensor fno_c2r_cuda(const at::Tensor& yw_, int64_t W, std::optional<at::ScalarType> out_dtype) {
  const c10::DeviceGuard guard(yw_.device());
  const at::ScalarType dt = fno_c2r_dtype(yw_, W, out_dtype);
  const int64_t B = yw_.size(0), Cout = yw_.size(1), H = yw_.size(2), m = yw_.size(3);
  const FnoTailRoute route =
      fno_c2r_pw_route(0, static_cast<int>(Cout), static_cast<int>(m), static_cast<int>(W), dt == at::kBFloat16);
  if (route.kind == FnoTailKind::Split || B * Cout * H * W >= (int64_t(1) << 31)) return fno_tail_c2r(yw_, W, dt);
  at::Tensor y = at::empty({B, Cout, H, W}, yw_.options().dtype(dt));
  fno_tail_launch(route.kind == FnoTailKind::Wide, yw_, nullptr, nullptr, c10::nullopt, false, y);
  return checked(y, "fno_c2r");
}

at::Tensor fno_c2r_meta(const at::Tensor& yw, int64_t W, std::optional<at::ScalarType> out_dtype) {
  return at::empty({yw.size(0), yw.size(1), yw.size(2), W}, yw.options().dtype(out_dtype.has_value() ? *out_dtype : at::kFloat));
}

// the checks legendre (vec = false) and legendre_vec share once the dtypes and ranks are known to fit: the extents
// of x against the table's (both tables of legendre_vec have one shape), tri, and the split forms that were given
void check_legendre_common(bool vec, const at::Tensor& x, const at::Tensor& table,
                           std::initializer_list<const c10::optional<at::Tensor>*> splits, int64_t tri) {
  const char* op = vec ? "legendre_vec" : "legendre";
  const char* tbl = vec ? "the tables " : "the table ";
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  TORCH_CHECK(x.size(-3) == table.size(2), op, ": x has ", x.size(-3), " points along the transformed dim, ", tbl,
              table.size(2));
  TORCH_CHECK(x.size(-2) == table.size(0), op, ": mode counts differ: x has ", x.size(-2), ", ", tbl, table.size(0));
  TORCH_CHECK(tri >= 0 && tri <= 2, op, ": tri must be 0, 1 or 2");
  TORCH_CHECK(table.size(0) < (1 << 30) && table.size(1) < (1 << 30) && table.size(2) >= 1 && table.size(2) < (1 << 30),
              op, ": bad table size");
  const int64_t Rp = ceil16(table.size(1)), Qp = ceil32(table.size(2));
  for (const c10::optional<at::Tensor>* ts : splits) {
    if (!present(*ts)) continue;
    TORCH_CHECK((*ts)->scalar_type() == at::kBFloat16 &&
                    (*ts)->sizes() == at::IntArrayRef({bf16 ? 1 : 2, table.size(0), Rp, Qp}) &&
                    (*ts)->device() == x.device(),
                op, vec ? ": ta_split and tb_split" : ": table_split", " must be bfloat16 [", bf16 ? 1 : 2,
                ", M, ceil16(R), ceil32(Q)] on the device of x (two planes for ",
                vec ? "float32 tables" : "a float32 table", ", one for bfloat16)");
  }
}

// ------------------------------------------------------------------ Legendre transform (latitude half of an SHT)
// x [..., Q, M, 2] fp32 (complex as trailing re/im), table [M, R, Q] fp32 -> y [..., R, M, 2] fp32:
//   y[n, r, m, :] = sum_q table[m, r, q] x[n, q, m, :]
// or all three bfloat16: bf16 operands as they are on one MFMA per fragment pair, fp32 accumulation, one rounding at
// the store (fp32 runs the bf16x3 split).  x and table of different dtypes raise.
// tri declares the structurally zero part of the table (1: rows r < m, 2: columns q < m), which every
// implementation treats as zero: tri = 1 returns exact zeros in y[.., r < m, m, :], and under tri = 2 every
// implementation ignores x where q < m -- a NaN or Inf there does not reach the result.  The table itself must be
// finite everywhere (the kernel multiplies partial tiles of it against staged zeros).
// table_split: the table as the kernel reads it, split_bf16(rows=False) of the
// table zero-padded to [M, ceil16(R), ceil32(Q)] -> bf16 [2, M, Rp, Qp]; built per call when absent.  For a bf16
// table it is the padded table itself, [1, M, Rp, Qp].
// legendre_out writes into a given contiguous tensor of the result's shape and dtype.
void check_legendre(const char*, const at::Tensor& x, const at::Tensor& table, const c10::optional<at::Tensor>& ts,
                    int64_t tri) {
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  TORCH_CHECK((x.scalar_type() == at::kFloat || bf16) && table.scalar_type() == x.scalar_type(),
              "legendre: x and table must both be float32 or both be bfloat16, got ", x.scalar_type(), " and ",
              table.scalar_type());
  TORCH_CHECK(x.dim() >= 3 && x.size(-1) == 2 && table.dim() == 3, "legendre: x [..., Q, M, 2], table [M, R, Q]");
  check_legendre_common(false, x, table, {&ts}, tri);
}

std::vector<int64_t> legendre_out_shape(const at::Tensor& x, const at::Tensor& table) {
  std::vector<int64_t> shape = x.sizes().vec();
  shape[shape.size() - 3] = table.size(1);
  return shape;
}

at::Tensor legendre_ref(const at::Tensor& x, const at::Tensor& table, const c10::optional<at::Tensor>& ts, int64_t tri) {
  const int64_t M = table.size(0), R = table.size(1), Q = table.size(2);
  if (x.scalar_type() == at::kBFloat16)  // the bf16 operands as they are, the product in fp32, rounded once
    return legendre_ref(x.to(at::kFloat), table.to(at::kFloat), c10::nullopt, tri).to(at::kBFloat16);
  at::Tensor t = table, xs = x.reshape({-1, Q, M, 2});
  if (tri != 0) {
    at::Tensor m = at::arange(M, table.options().dtype(at::kLong)).unsqueeze(1);
    at::Tensor k = at::arange(tri == 1 ? R : Q, table.options().dtype(at::kLong)).unsqueeze(0);
    at::Tensor keep = k.ge(m);  // [M, R] or [M, Q]
    t = at::where(tri == 1 ? keep.unsqueeze(2) : keep.unsqueeze(1), table, at::zeros({}, table.options()));
    // tri = 2: x[n, q < m, m, :] is not read (a masked table alone would turn a NaN or Inf there into NaN)
    if (tri == 2) xs = at::where(keep.t().unsqueeze(0).unsqueeze(-1), xs, at::zeros({}, x.options()));
  }
  at::Tensor y = at::einsum("mrq,nqmc->nrmc", {t, xs});
  return y.reshape(legendre_out_shape(x, table)).contiguous();
}

// a table as the kernel reads it: its split form where the caller gave one, else the table zero-padded to
// [M, Rp, Qp] and split into bf16 planes [2, M, Rp, Qp] (a bf16 table: the padded table itself, [1, M, Rp, Qp])
at::Tensor legendre_table_planes(bool vec, const at::Tensor& table, const c10::optional<at::Tensor>& ts,
                                 const at::Tensor& x, hipStream_t stream) {
  if (present(ts)) return ts->contiguous();
  TORCH_CHECK(table.device() == x.device(),
              vec ? "legendre_vec: ta and tb must be on the device of x" : "legendre: table must be on the device of x");
  const int64_t M = table.size(0), R = table.size(1), Q = table.size(2);
  const int64_t Rp = ceil16(R), Qp = ceil32(Q);
  at::Tensor tp = at::constant_pad_nd(table, {0, Qp - Q, 0, Rp - R}).contiguous();
  if (x.scalar_type() == at::kBFloat16) return tp.unsqueeze(0);
  at::Tensor planes = at::empty({2, M, Rp, Qp}, tp.options().dtype(at::kBFloat16));
  if (tp.numel() > 0)
    launch_split_bf16(tp.data_ptr<float>(), reinterpret_cast<uint16_t*>(planes.data_ptr()), tp.numel(),
                      static_cast<int>(Qp), false, stream);
  return planes;
}

// the launch path of legendre, legendre_vec (tb given: two tables) and their _out forms: y is the contiguous result,
// aligned to one (re, im) pair (8 bytes fp32, 4 bytes bf16: the kernel's stores)
void legendre_run(const at::Tensor& x_, const at::Tensor& ta, const c10::optional<at::Tensor>& tas,
                  const at::Tensor* tb, const c10::optional<at::Tensor>& tbs, int64_t tri, const at::Tensor& y) {
  const bool vec = tb != nullptr;
  const int64_t M = ta.size(0), R = ta.size(1), Q = ta.size(2);
  const int64_t plane = M * ceil16(R) * ceil32(Q);
  auto stream = current_stream(x_);
  const bool bf16 = x_.scalar_type() == at::kBFloat16;
  // one load per mode's (re, im), 8 bytes (bf16: 4): a view at an odd element offset gets its own copy
  at::Tensor x = aligned_to(x_.contiguous(), bf16 ? 4 : 8);
  at::Tensor ap = legendre_table_planes(vec, ta, tas, x, stream), bp;
  if (vec) bp = legendre_table_planes(vec, *tb, tbs, x, stream);
  if (y.numel() == 0) return;
  LegendreLaunch p;
  p.N = x.numel() / (Q * M * 2);  // the [Q, M, 2] planes of x: fields, or vec: 2 x fields
  TORCH_CHECK(p.N < (int64_t(1) << 31) / 16, vec ? "legendre_vec" : "legendre", ": too many fields");
  p.x = x.data_ptr();
  p.th = reinterpret_cast<const uint16_t*>(ap.data_ptr());
  p.tl = bf16 ? nullptr : p.th + plane;
  if (vec) {
    p.bh = reinterpret_cast<const uint16_t*>(bp.data_ptr());
    p.bl = bf16 ? nullptr : p.bh + plane;
  }
  p.y = y.data_ptr();
  p.bf16 = bf16 ? 1 : 0;
  p.vec = vec ? 1 : 0;
  p.Q = static_cast<int>(Q);
  p.R = static_cast<int>(R);
  p.M = static_cast<int>(M);
  p.tri = static_cast<int>(tri);
  if (vec) launch_legendre_vec(p, stream);
  else launch_legendre(p, stream);
}

struct Legendre : OpFamily {
  using Sig = at::Tensor(const at::Tensor&, const at::Tensor&, const c10::optional<at::Tensor>&, int64_t);
  static constexpr const char *name = "legendre", *out_name = "legendre_out";
  static constexpr auto& check = check_legendre;
  template <class... A>
  static OpResult result(const at::Tensor& x, const at::Tensor& table, const A&...) {
    return {legendre_out_shape(x, table), x.options()};
  }
  template <class... A>
  static uintptr_t out_align(const at::Tensor& x, const A&...) {  // one (re, im) pair
    return 2 * x.element_size();
  }
  static constexpr auto& reference = legendre_ref;
  static void run(const at::Tensor& x, const at::Tensor& table, const c10::optional<at::Tensor>& ts, int64_t tri,
                  const at::Tensor& y) {
    legendre_run(x, table, ts, nullptr, c10::nullopt, tri, y);
  }
};
AMD_DFT_OP_FAMILY(legendre, Legendre)

// Which tiling legendre runs for (Q, R, M, real columns = 2 x fields, tri) -- host only, no device (the companion
// of fno_pointwise_info): "mfma MT=8 CT=2 slabs=23 rtiles=4 rgroups=1 mgroups=8 ctiles=3 lds=41472 wgs=24 tri=1";
// bf16: the same tiling with the bf16 instances' LDS bytes and a trailing " bf16=1".  legendre_vec_info: the same
// fields for legendre_vec, real columns = 4 x fields (fp32 has no MT=8 instance)
std::string legendre_info_of(bool vec, int64_t Q, int64_t R, int64_t M, int64_t cols, int64_t tri, bool bf16) {
  const char* op = vec ? "amd_dft.legendre_vec_info" : "amd_dft.legendre_info";
  const int64_t unit = vec ? 4 : 2;
  TORCH_CHECK(Q >= 1 && R >= 1 && M >= 1 && cols >= unit && cols % unit == 0 && Q < (1 << 30) && R < (1 << 30) &&
                  M < (1 << 30) && cols < (int64_t(1) << 31) / 8,
              op, ": Q, R, M must be >= 1 and cols a positive ", vec ? "multiple of 4" : "even count");
  TORCH_CHECK(tri >= 0 && tri <= 2, op, ": tri must be 0, 1 or 2");
  const LegendreRoute r = legendre_route(Q, R, M, cols, static_cast<int>(tri), bf16, vec);
  return "mfma MT=" + std::to_string(r.mt) + " CT=" + std::to_string(r.ct) + " slabs=" + std::to_string(r.slabs) +
         " rtiles=" + std::to_string(r.rtiles) + " rgroups=" + std::to_string(r.rgroups) +
         " mgroups=" + std::to_string(r.mgroups) + " ctiles=" + std::to_string(r.ctiles) +
         " lds=" + std::to_string(r.lds) + " wgs=" + std::to_string(r.wgs) + " tri=" + std::to_string(tri) +
         (bf16 ? " bf16=1" : "");
}
std::string legendre_info(int64_t Q, int64_t R, int64_t M, int64_t cols, int64_t tri, bool bf16) {
  return legendre_info_of(false, Q, R, M, cols, tri, bf16);
}
std::string legendre_vec_info(int64_t Q, int64_t R, int64_t M, int64_t cols, int64_t tri, bool bf16) {
  return legendre_info_of(true, Q, R, M, cols, tri, bf16);
}

// ------------------------------------------------------------------ vector Legendre transform (vector SHT)
// x [..., 2, Q, M, 2] (a tangential vector field's two components, complex as trailing re/im), ta and tb [M, R, Q]
// -> y [..., 2, R, M, 2]:
//   y[n, 0, r, m] = sum_q ta[m, r, q] x[n, 0, q, m] - i tb[m, r, q] x[n, 1, q, m]
//   y[n, 1, r, m] = sum_q ta[m, r, q] x[n, 1, q, m] + i tb[m, r, q] x[n, 0, q, m]
// All float32 (bf16x3) or all bfloat16, as legendre; tri, the split forms and the _out variant are legendre's too,
// with tri declaring the same zero part of both tables.
void check_legendre_vec(const char*, const at::Tensor& x, const at::Tensor& ta, const at::Tensor& tb,
                        const c10::optional<at::Tensor>& tas, const c10::optional<at::Tensor>& tbs, int64_t tri) {
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  TORCH_CHECK((x.scalar_type() == at::kFloat || bf16) && ta.scalar_type() == x.scalar_type() &&
                  tb.scalar_type() == x.scalar_type(),
              "legendre_vec: x, ta and tb must all be float32 or all be bfloat16, got ", x.scalar_type(), ", ",
              ta.scalar_type(), " and ", tb.scalar_type());
  TORCH_CHECK(x.dim() >= 4 && x.size(-1) == 2 && x.size(-4) == 2 && ta.dim() == 3,
              "legendre_vec: x [..., 2, Q, M, 2], ta and tb [M, R, Q]");
  TORCH_CHECK(tb.sizes() == ta.sizes(), "legendre_vec: ta and tb must have the same shape, got ", ta.sizes(), " and ",
              tb.sizes());
  TORCH_CHECK(tb.device() == ta.device(), "legendre_vec: ta and tb must be on the same device");
  check_legendre_common(true, x, ta, {&tas, &tbs}, tri);
}

at::Tensor legendre_vec_ref(const at::Tensor& x, const at::Tensor& ta, const at::Tensor& tb,
                            const c10::optional<at::Tensor>& tas, const c10::optional<at::Tensor>& tbs, int64_t tri) {
  // the definition: four plain transforms and the two rotations; y0 = A x0 - i B x1, y1 = A x1 + i B x0
  if (x.scalar_type() == at::kBFloat16)  // the bf16 operands as they are, everything in fp32, rounded once
    return legendre_vec_ref(x.to(at::kFloat), ta.to(at::kFloat), tb.to(at::kFloat), c10::nullopt, c10::nullopt, tri)
        .to(at::kBFloat16);
  at::Tensor a = legendre_ref(x, ta, c10::nullopt, tri);  // [..., 2, R, M, 2]: (A x0, A x1)
  at::Tensor b = legendre_ref(x, tb, c10::nullopt, tri);  //                    (B x0, B x1)
  at::Tensor b0 = b.select(-4, 0), b1 = b.select(-4, 1);
  // -i (re, im) = (im, -re);  +i (re, im) = (-im, re)
  at::Tensor r0 = at::stack({b1.select(-1, 1), b1.select(-1, 0).neg()}, -1);
  at::Tensor r1 = at::stack({b0.select(-1, 1).neg(), b0.select(-1, 0)}, -1);
  return (a + at::stack({r0, r1}, -4)).contiguous();
}

struct LegendreVec : Legendre {  // result and out_align are legendre's, from x and the first table
  using Sig = at::Tensor(const at::Tensor&, const at::Tensor&, const at::Tensor&, const c10::optional<at::Tensor>&,
                         const c10::optional<at::Tensor>&, int64_t);
  static constexpr const char *name = "legendre_vec", *out_name = "legendre_vec_out";
  static constexpr auto& check = check_legendre_vec;
  static constexpr auto& reference = legendre_vec_ref;
  static void run(const at::Tensor& x, const at::Tensor& ta, const at::Tensor& tb, const c10::optional<at::Tensor>& tas,
                  const c10::optional<at::Tensor>& tbs, int64_t tri, const at::Tensor& y) {
    legendre_run(x, ta, tas, &tb, tbs, tri, y);
  }
};
AMD_DFT_OP_FAMILY(legendre_vec, LegendreVec)

// ------------------------------------------------------------------ DISCO convolution on the sphere (gather half)
// x [..., nlat_in, nlon_in], a longitude-invariant filter tensor in CSR over rows p * nlat_out + k' (row_ptr int32
// [K * nlat_out + 1], idx int32 [nnz] = k * nlon_in + d sorted within a row, val [nnz]) -> y [..., K, nlat_out, nlon_out]:
//   y[n, p, k', j'] = sum_e val[e] * x[n, k_e, (d_e + s j') mod nlon_in],  s = nlon_in / nlon_out
// x float32 or bfloat16 with float32 val, fp32 accumulation, one rounding to x's dtype.  CPU tensors only: float64 x
// with float64 val, the unrounded definition (what the fp64 oracle tests compare).  The table is trusted to be what
// ops.disco.disco_tables builds (the holder checks it on the host); the kernel reads nothing outside x whatever it
// holds, and the CPU kernel checks every entry.
void check_disco(const char* op, const at::Tensor& x, const at::Tensor& row_ptr, const at::Tensor& idx,
                 const at::Tensor& val, int64_t K, int64_t nlat_out, int64_t nlon_out) {
  const auto xt = x.scalar_type();
  TORCH_CHECK(xt == at::kFloat || xt == at::kBFloat16 || (xt == at::kDouble && x.device().is_cpu()), op,
              ": x must be float32 or bfloat16 (float64 on CPU tensors), got ", xt);
  TORCH_CHECK(val.scalar_type() == (xt == at::kDouble ? at::kDouble : at::kFloat), op, ": val must be ",
              xt == at::kDouble ? "float64 for a float64 x" : "float32", ", got ", val.scalar_type());
  TORCH_CHECK(row_ptr.scalar_type() == at::kInt && idx.scalar_type() == at::kInt, op,
              ": row_ptr and idx must be int32, got ", row_ptr.scalar_type(), " and ", idx.scalar_type());
  TORCH_CHECK(x.dim() >= 2, op, ": x must be [..., nlat_in, nlon_in], got ", x.sizes());
  TORCH_CHECK(K >= 1 && nlat_out >= 1 && nlon_out >= 1 && K * nlat_out < (int64_t(1) << 31) - 1, op,
              ": K, nlat_out and nlon_out must be >= 1");
  const int64_t nlat_in = x.size(-2), nlon_in = x.size(-1);
  TORCH_CHECK(nlat_in >= 1 && nlon_in >= 1 && nlat_in * nlon_in < (int64_t(1) << 31), op,
              ": the input grid must be non-empty and hold fewer than 2^31 points, got ", nlat_in, " x ", nlon_in);
  TORCH_CHECK(nlon_in % nlon_out == 0, op, ": nlon_in (", nlon_in, ") must be a multiple of nlon_out (", nlon_out, ")");
  TORCH_CHECK(row_ptr.dim() == 1 && row_ptr.size(0) == K * nlat_out + 1, op, ": row_ptr must be [K * nlat_out + 1] = [",
              K * nlat_out + 1, "], got ", row_ptr.sizes());
  TORCH_CHECK(idx.dim() == 1 && val.dim() == 1 && idx.size(0) == val.size(0) && idx.size(0) < (int64_t(1) << 31), op,
              ": idx and val must be [nnz] with nnz < 2^31, got ", idx.sizes(), " and ", val.sizes());
  TORCH_CHECK(row_ptr.device() == x.device() && idx.device() == x.device() && val.device() == x.device(), op,
              ": row_ptr, idx and val must be on the device of x");
}

std::vector<int64_t> disco_out_shape(const at::Tensor& x, int64_t K, int64_t nlat_out, int64_t nlon_out) {
  TORCH_CHECK(x.dim() >= 2, "disco: x must be [..., nlat_in, nlon_in]");
  std::vector<int64_t> s(x.sizes().begin(), x.sizes().end() - 2);
  s.insert(s.end(), {K, nlat_out, nlon_out});
  return s;
}

at::Tensor disco_ref(const at::Tensor& x, const at::Tensor& row_ptr, const at::Tensor& idx, const at::Tensor& val,
                     int64_t K, int64_t nlat_out, int64_t nlon_out) {
  const int64_t nlat_in = x.size(-2), nlon_in = x.size(-1), s = nlon_in / nlon_out, rows = K * nlat_out;
  const int64_t nnz = idx.size(0), pin = nlat_in * nlon_in;
  const at::Tensor rp = row_ptr.contiguous(), ix = idx.contiguous(), vd = val.to(at::kDouble).contiguous();
  const int32_t* rpp = rp.data_ptr<int32_t>();
  const int32_t* ixp = ix.data_ptr<int32_t>();
  const double* vp = vd.data_ptr<double>();
  TORCH_CHECK(rpp[0] >= 0 && rpp[rows] <= nnz, "disco: row_ptr must run from >= 0 to <= nnz");
  for (int64_t r = 0; r < rows; ++r)
    TORCH_CHECK(rpp[r] <= rpp[r + 1], "disco: row_ptr must not decrease (row ", r, ")");
  for (int64_t e = rpp[0]; e < rpp[rows]; ++e)
    TORCH_CHECK(ixp[e] >= 0 && ixp[e] < pin, "disco: idx[", e, "] = ", ixp[e], " is outside the input grid");
  // the fp32 / bf16 values as they are, every sum in fp64 in table order, one rounding to x's dtype
  const at::Tensor xd = x.to(at::kDouble).contiguous();
  const int64_t planes = pin > 0 ? xd.numel() / pin : 0;
  at::Tensor y = at::zeros(disco_out_shape(x, K, nlat_out, nlon_out), xd.options());
  const double* xp = xd.data_ptr<double>();
  double* yp = y.data_ptr<double>();
  at::parallel_for(0, planes * rows, 1, [&](int64_t b, int64_t e_) {
    for (int64_t t = b; t < e_; ++t) {
      const int64_t n = t / rows, r = t % rows;
      const double* xn = xp + n * pin;
      double* yr = yp + t * nlon_out;
      for (int64_t e = rpp[r]; e < rpp[r + 1]; ++e) {
        const int64_t k0 = ixp[e] / nlon_in * nlon_in, d = ixp[e] - k0;
        const double v = vp[e];
        for (int64_t j = 0; j < nlon_out; ++j) {
          int64_t c = d + s * j;
          if (c >= nlon_in) c -= nlon_in;
          yr[j] += v * xn[k0 + c];
        }
      }
    }
  });
  return y.to(x.scalar_type());
}

// the launch path of disco and disco_out (y contiguous, x's dtype)
void disco_run(const at::Tensor& x_, const at::Tensor& row_ptr, const at::Tensor& idx, const at::Tensor& val, int64_t K,
               int64_t nlat_out, int64_t nlon_out, const at::Tensor& y) {
  if (y.numel() == 0) return;
  at::Tensor x = x_.contiguous();  // element loads: a view at any element offset is read where it is
  at::Tensor rp = row_ptr.contiguous(), ix = idx.contiguous(), vl = val.contiguous();
  DiscoLaunch p;
  p.x = x.data_ptr();
  p.row_ptr = rp.data_ptr<int32_t>();
  p.idx = ix.data_ptr<int32_t>();
  p.val = vl.data_ptr<float>();
  p.y = y.data_ptr();
  p.nlat_in = static_cast<int>(x.size(-2));
  p.nlon_in = static_cast<int>(x.size(-1));
  p.planes = x.numel() / (x.size(-2) * x.size(-1));
  p.K = static_cast<int>(K);
  p.nlat_out = static_cast<int>(nlat_out);
  p.nlon_out = static_cast<int>(nlon_out);
  p.nnz = idx.size(0);
  p.bf16 = x.scalar_type() == at::kBFloat16 ? 1 : 0;
  launch_disco(p, current_stream(x));
}

void check_disco_device(const char* op, const at::Tensor& x, const at::Tensor&, const at::Tensor&, const at::Tensor&,
                        int64_t, int64_t nlat_out, int64_t nlon_out) {
  TORCH_CHECK(x.size(-1) * 4 <= kDiscoLdsBytes, op, ": nlon_in must be at most ", kDiscoLdsBytes / 4,
              " on the device (one input row per LDS chunk), got ", x.size(-1));
  TORCH_CHECK(nlon_out < (int64_t(1) << 28) && nlat_out < (int64_t(1) << 30), op, ": output grid too large");
}

struct Disco : OpFamily {
  using Sig = at::Tensor(const at::Tensor&, const at::Tensor&, const at::Tensor&, const at::Tensor&, int64_t, int64_t,
                         int64_t);
  static constexpr const char *name = "disco", *out_name = "disco_out";
  static constexpr auto& check = check_disco;
  static constexpr auto& check_device = check_disco_device;
  static OpResult result(const at::Tensor& x, const at::Tensor&, const at::Tensor&, const at::Tensor&, int64_t K,
                         int64_t nlat_out, int64_t nlon_out) {
    return {disco_out_shape(x, K, nlat_out, nlon_out), x.options()};
  }
  template <class... A>
  static uintptr_t out_align(const at::Tensor& x, const A&...) {  // element stores
    return x.element_size();
  }
  static constexpr auto& reference = disco_ref;
  static constexpr auto& run = disco_run;
};
AMD_DFT_OP_FAMILY(disco, Disco)

// Which instance and grid disco runs -- host only, no device; from disco_route, which launch_disco dispatches on:
// "PT=4 rows=11 lds=63360 ptiles=16 wgs=2880 passes=2 items=3 threads=256".  nnz_max: the entry count the launch is
// given (idx.numel(); only its range is checked).  The band of an output latitude is in the table, not in the
// arguments, so whether a latitude is walked in chunks (band > rows) is not part of the answer.
std::string disco_info(int64_t planes, int64_t nlat_in, int64_t nlon_in, int64_t K, int64_t nlat_out, int64_t nlon_out,
                       int64_t nnz_max, bool bf16) {
  TORCH_CHECK(planes >= 1 && nlat_in >= 1 && nlon_in >= 1 && K >= 1 && nlat_out >= 1 && nlon_out >= 1 &&
                  nlat_in * nlon_in < (int64_t(1) << 31) && nnz_max >= 0 && nnz_max < (int64_t(1) << 31),
              "amd_dft.disco_info: sizes must be >= 1 and the input grid and nnz_max below 2^31");
  TORCH_CHECK(nlon_in % nlon_out == 0, "amd_dft.disco_info: nlon_in must be a multiple of nlon_out");
  TORCH_CHECK(nlon_in * 4 <= kDiscoLdsBytes, "amd_dft.disco_info: nlon_in must be at most ", kDiscoLdsBytes / 4);
  const DiscoRoute r = disco_route(planes, nlat_in, nlon_in, K, nlat_out, nlon_out, nnz_max, bf16);
  return "PT=" + std::to_string(r.pt) + " rows=" + std::to_string(r.rows) + " lds=" + std::to_string(r.lds) +
         " ptiles=" + std::to_string(r.ptiles) + " wgs=" + std::to_string(r.wgs) +
         " passes=" + std::to_string(r.passes) + " items=" + std::to_string(kDiscoItems) +
         " threads=" + std::to_string(kDiscoThreads) + (bf16 ? " bf16=1" : "");
}

// ------------------------------------------------------------------ DISCO convolution on the sphere (transposed half)
// z [..., C, K, nlat_in, nlon_in], a gather CSR over rows k * s + rho, s = nlon_out / nlon_in (row_ptr int32
// [nlat_out * s + 1], idx int32 [nnz] = (k' * K + p) * nlon_in + d sorted within a row, val [nnz]), bias [C] fp32 or
// none -> y [..., C, nlat_out, nlon_out]:
//   y[n, k, s t + rho] = sum_e val[e] * z[n, p_e, k'_e, (d_e + t) mod nlon_in] (+ bias[c]),  0 <= t < nlon_in
// z float32 or bfloat16 with float32 val, fp32 accumulation, the bias added in fp32, one rounding to z's dtype.  CPU
// tensors only: float64 z with float64 val.  The table is trusted to be what ops.disco.disco_transpose_tables builds
// (the holder checks it on the host); the kernel reads nothing outside z whatever it holds, and the CPU kernel checks
// every entry.
void check_disco_t(const char* op, const at::Tensor& z, const at::Tensor& row_ptr, const at::Tensor& idx,
                   const at::Tensor& val, int64_t nlat_out, int64_t nlon_out, const c10::optional<at::Tensor>& bias) {
  const auto zt = z.scalar_type();
  TORCH_CHECK(zt == at::kFloat || zt == at::kBFloat16 || (zt == at::kDouble && z.device().is_cpu()), op,
              ": z must be float32 or bfloat16 (float64 on CPU tensors), got ", zt);
  TORCH_CHECK(val.scalar_type() == (zt == at::kDouble ? at::kDouble : at::kFloat), op, ": val must be ",
              zt == at::kDouble ? "float64 for a float64 z" : "float32", ", got ", val.scalar_type());
  TORCH_CHECK(row_ptr.scalar_type() == at::kInt && idx.scalar_type() == at::kInt, op,
              ": row_ptr and idx must be int32, got ", row_ptr.scalar_type(), " and ", idx.scalar_type());
  TORCH_CHECK(z.dim() >= 4, op, ": z must be [..., C, K, nlat_in, nlon_in], got ", z.sizes());
  const int64_t C = z.size(-4), K = z.size(-3), nlat_in = z.size(-2), nlon_in = z.size(-1);
  TORCH_CHECK(K >= 1 && nlat_in >= 1 && nlon_in >= 1 && K * nlat_in * nlon_in < (int64_t(1) << 31), op,
              ": K and the input grid must be non-empty and K * nlat_in * nlon_in below 2^31, got ", K, " x ", nlat_in,
              " x ", nlon_in);
  TORCH_CHECK(nlat_out >= 1 && nlon_out >= 1, op, ": nlat_out and nlon_out must be >= 1");
  TORCH_CHECK(nlon_out % nlon_in == 0, op, ": nlon_out (", nlon_out, ") must be a multiple of nlon_in (", nlon_in, ")");
  const int64_t s = nlon_out / nlon_in;
  TORCH_CHECK(nlat_out * s < (int64_t(1) << 31) - 1, op, ": too many table rows");
  TORCH_CHECK(row_ptr.dim() == 1 && row_ptr.size(0) == nlat_out * s + 1, op, ": row_ptr must be [nlat_out * s + 1] = [",
              nlat_out * s + 1, "], got ", row_ptr.sizes());
  TORCH_CHECK(idx.dim() == 1 && val.dim() == 1 && idx.size(0) == val.size(0) && idx.size(0) < (int64_t(1) << 31), op,
              ": idx and val must be [nnz] with nnz < 2^31, got ", idx.sizes(), " and ", val.sizes());
  TORCH_CHECK(row_ptr.device() == z.device() && idx.device() == z.device() && val.device() == z.device(), op,
              ": row_ptr, idx and val must be on the device of z");
  if (present(bias)) {
    TORCH_CHECK(bias->scalar_type() == (zt == at::kDouble ? at::kDouble : at::kFloat), op, ": bias must be ",
                zt == at::kDouble ? "float64 for a float64 z" : "float32", ", got ", bias->scalar_type());
    TORCH_CHECK(bias->dim() == 1 && bias->size(0) == C, op, ": bias must be [C] = [", C, "], got ", bias->sizes());
    TORCH_CHECK(bias->device() == z.device(), op, ": bias must be on the device of z");
  }
}

std::vector<int64_t> disco_t_out_shape(const at::Tensor& z, int64_t nlat_out, int64_t nlon_out) {
  TORCH_CHECK(z.dim() >= 4, "disco_t: z must be [..., C, K, nlat_in, nlon_in]");
  std::vector<int64_t> s(z.sizes().begin(), z.sizes().end() - 3);
  s.insert(s.end(), {nlat_out, nlon_out});
  return s;
}

at::Tensor disco_t_ref(const at::Tensor& z, const at::Tensor& row_ptr, const at::Tensor& idx, const at::Tensor& val,
                       int64_t nlat_out, int64_t nlon_out, const c10::optional<at::Tensor>& bias) {
  const int64_t C = z.size(-4), K = z.size(-3), nlat_in = z.size(-2), nlon_in = z.size(-1);
  const int64_t s = nlon_out / nlon_in, rows = nlat_out * s, nnz = idx.size(0), pin = nlat_in * nlon_in;
  const at::Tensor rp = row_ptr.contiguous(), ix = idx.contiguous(), vd = val.to(at::kDouble).contiguous();
  const int32_t* rpp = rp.data_ptr<int32_t>();
  const int32_t* ixp = ix.data_ptr<int32_t>();
  const double* vp = vd.data_ptr<double>();
  TORCH_CHECK(rpp[0] >= 0 && rpp[rows] <= nnz, "disco_t: row_ptr must run from >= 0 to <= nnz");
  for (int64_t r = 0; r < rows; ++r)
    TORCH_CHECK(rpp[r] <= rpp[r + 1], "disco_t: row_ptr must not decrease (row ", r, ")");
  for (int64_t e = rpp[0]; e < rpp[rows]; ++e)
    TORCH_CHECK(ixp[e] >= 0 && ixp[e] < K * pin, "disco_t: idx[", e, "] = ", ixp[e], " is outside the input grid");
  // the fp32 / bf16 values as they are, every sum in fp64 in table order, the bias last, one rounding to z's dtype
  const at::Tensor zd = z.to(at::kDouble).contiguous();
  const int64_t planes = zd.numel() / (K * pin);
  at::Tensor bd;
  if (present(bias)) bd = bias->to(at::kDouble).contiguous();
  const double* bp = bd.defined() ? bd.data_ptr<double>() : nullptr;
  at::Tensor y = at::zeros(disco_t_out_shape(z, nlat_out, nlon_out), zd.options());
  const double* zp = zd.data_ptr<double>();
  double* yp = y.data_ptr<double>();
  at::parallel_for(0, planes * nlat_out, 1, [&](int64_t b, int64_t e_) {
    for (int64_t u = b; u < e_; ++u) {
      const int64_t n = u / nlat_out, k = u % nlat_out;
      const double* zn = zp + n * K * pin;
      double* yr = yp + u * nlon_out;
      for (int64_t rho = 0; rho < s; ++rho) {
        const int64_t r = k * s + rho;
        for (int64_t e = rpp[r]; e < rpp[r + 1]; ++e) {
          const int64_t q = ixp[e] / nlon_in, d = ixp[e] - q * nlon_in, kin = q / K, p = q - kin * K;
          const double* zr = zn + p * pin + kin * nlon_in;
          const double v = vp[e];
          for (int64_t t = 0; t < nlon_in; ++t) {
            int64_t c = d + t;
            if (c >= nlon_in) c -= nlon_in;
            yr[s * t + rho] += v * zr[c];
          }
        }
      }
      if (bp)
        for (int64_t j = 0; j < nlon_out; ++j) yr[j] += bp[n % C];
    }
  });
  return y.to(z.scalar_type());
}

// the launch path of disco_t and disco_t_out (y contiguous, z's dtype)
void disco_t_run(const at::Tensor& z_, const at::Tensor& row_ptr, const at::Tensor& idx, const at::Tensor& val,
                 int64_t nlat_out, int64_t nlon_out, const c10::optional<at::Tensor>& bias, const at::Tensor& y) {
  if (y.numel() == 0) return;
  at::Tensor z = z_.contiguous();  // element loads: a view at any element offset is read where it is
  at::Tensor rp = row_ptr.contiguous(), ix = idx.contiguous(), vl = val.contiguous();
  at::Tensor bf = f32_or_undef(bias);
  DiscoTLaunch p;
  p.z = z.data_ptr();
  p.row_ptr = rp.data_ptr<int32_t>();
  p.idx = ix.data_ptr<int32_t>();
  p.val = vl.data_ptr<float>();
  p.bias = bf.defined() ? bf.data_ptr<float>() : nullptr;
  p.y = y.data_ptr();
  p.C = z.size(-4);
  p.K = static_cast<int>(z.size(-3));
  p.nlat_in = static_cast<int>(z.size(-2));
  p.nlon_in = static_cast<int>(z.size(-1));
  p.planes = z.numel() / (z.size(-3) * z.size(-2) * z.size(-1));
  p.nlat_out = static_cast<int>(nlat_out);
  p.nlon_out = static_cast<int>(nlon_out);
  p.nnz = idx.size(0);
  p.bf16 = z.scalar_type() == at::kBFloat16 ? 1 : 0;
  launch_disco_t(p, current_stream(z));
}

void check_disco_t_device(const char* op, const at::Tensor& z, const at::Tensor&, const at::Tensor&, const at::Tensor&,
                          int64_t nlat_out, int64_t nlon_out, const c10::optional<at::Tensor>&) {
  TORCH_CHECK(z.size(-3) * z.size(-1) * 4 <= kDiscoLdsBytes, op, ": K * nlon_in must be at most ", kDiscoLdsBytes / 4,
              " on the device (the K basis planes of one input latitude per LDS chunk), got ", z.size(-3), " * ",
              z.size(-1));
  TORCH_CHECK(nlon_out < (int64_t(1) << 28) && nlat_out < (int64_t(1) << 30), op, ": output grid too large");
}

struct DiscoT : OpFamily {
  using Sig = at::Tensor(const at::Tensor&, const at::Tensor&, const at::Tensor&, const at::Tensor&, int64_t, int64_t,
                         const c10::optional<at::Tensor>&);
  static constexpr const char *name = "disco_t", *out_name = "disco_t_out";
  static constexpr auto& check = check_disco_t;
  static constexpr auto& check_device = check_disco_t_device;
  static OpResult result(const at::Tensor& z, const at::Tensor&, const at::Tensor&, const at::Tensor&, int64_t nlat_out,
                         int64_t nlon_out, const c10::optional<at::Tensor>&) {
    return {disco_t_out_shape(z, nlat_out, nlon_out), z.options()};
  }
  template <class... A>
  static uintptr_t out_align(const at::Tensor& z, const A&...) {  // element stores
    return z.element_size();
  }
  static constexpr auto& reference = disco_t_ref;
  static constexpr auto& run = disco_t_run;
};
AMD_DFT_OP_FAMILY(disco_t, DiscoT)

// Which instance and grid disco_t runs -- host only, no device; from disco_t_route, which launch_disco_t dispatches
// on: "PT=1 rows=7 lds=60480 ptiles=20 wgs=14400 passes=1 phases=2 items=3 threads=256".  As with disco_info the band
// of an output latitude is in the table, so whether it is walked in chunks is not part of the answer.
std::string disco_t_info(int64_t planes, int64_t nlat_in, int64_t nlon_in, int64_t K, int64_t nlat_out,
                         int64_t nlon_out, int64_t nnz_max, bool bf16) {
  TORCH_CHECK(planes >= 1 && nlat_in >= 1 && nlon_in >= 1 && K >= 1 && nlat_out >= 1 && nlon_out >= 1 &&
                  K < (int64_t(1) << 31) && nlat_in * nlon_in < (int64_t(1) << 31) &&
                  K * nlat_in * nlon_in < (int64_t(1) << 31) && nnz_max >= 0 && nnz_max < (int64_t(1) << 31),
              "amd_dft.disco_t_info: sizes must be >= 1 and K * nlat_in * nlon_in and nnz_max below 2^31");
  TORCH_CHECK(nlon_out % nlon_in == 0, "amd_dft.disco_t_info: nlon_out must be a multiple of nlon_in");
  TORCH_CHECK(K * nlon_in * 4 <= kDiscoLdsBytes, "amd_dft.disco_t_info: K * nlon_in must be at most ",
              kDiscoLdsBytes / 4);
  const DiscoTRoute r = disco_t_route(planes, nlat_in, nlon_in, K, nlat_out, nlon_out, nnz_max, bf16);
  return "PT=" + std::to_string(r.pt) + " rows=" + std::to_string(r.rows) + " lds=" + std::to_string(r.lds) +
         " ptiles=" + std::to_string(r.ptiles) + " wgs=" + std::to_string(r.wgs) +
         " passes=" + std::to_string(r.passes) + " phases=" + std::to_string(r.phases) +
         " items=" + std::to_string(kDiscoItems) + " threads=" + std::to_string(kDiscoThreads) + (bf16 ? " bf16=1" : "");
}

// ------------------------------------------------------------------ SFNO per-degree channel mixing
// c [B, Cin, L, M, 2] fp32 (spherical harmonic coefficients, complex as trailing re/im), w [Cin, Cout, L, 2] fp32
// -> y [B, Cout, L, M, 2] fp32:   y[b, o, l, m] = sum_i c[b, i, l, m] w[i, o, l]   (complex)
// tri = 1 declares c zero where l < m (the spectrum of a real field): every implementation ignores c there and
// returns exact zeros.  w_split: the weights as the kernel reads them (sfno_mix_split); built per call when absent.
// All three bfloat16 instead: bf16 operands as they are on one MFMA per fragment pair, fp32 accumulation, one rounding
// at the store.  c and w of different dtypes raise.
void check_sfno_mix(const char*, const at::Tensor& c, const at::Tensor& w, const c10::optional<at::Tensor>& ws,
                    int64_t tri) {
  const bool bf16 = c.scalar_type() == at::kBFloat16;
  TORCH_CHECK((c.scalar_type() == at::kFloat || bf16) && w.scalar_type() == c.scalar_type(),
              "sfno_mix: c and w must both be float32 or both be bfloat16, got ", c.scalar_type(), " and ",
              w.scalar_type());
  TORCH_CHECK(c.dim() == 5 && c.size(4) == 2 && w.dim() == 4 && w.size(3) == 2,
              "sfno_mix: c [B, Cin, L, M, 2], w [Cin, Cout, L, 2]");
  TORCH_CHECK(c.size(1) == w.size(0) && w.size(0) >= 1, "sfno_mix: c has ", c.size(1), " input channels, w ", w.size(0));
  TORCH_CHECK(c.size(2) == w.size(2), "sfno_mix: degree counts differ: c has ", c.size(2), ", w ", w.size(2));
  TORCH_CHECK(tri == 0 || tri == 1, "sfno_mix: tri must be 0 or 1");
  TORCH_CHECK(w.size(0) < (1 << 28) && w.size(1) < (1 << 21) && c.size(2) <= 65535 &&
                  c.size(0) * c.size(3) < (int64_t(1) << 30),
              "sfno_mix: tensor too large");
  if (present(ws)) {
    const int64_t Op = ceil16(w.size(1)), Kp = ceil32(2 * w.size(0));
    TORCH_CHECK(ws->scalar_type() == at::kBFloat16 &&
                    ws->sizes() == at::IntArrayRef({bf16 ? 1 : 2, w.size(2), Op, Kp}) && ws->device() == c.device(),
                "sfno_mix: w_split must be bfloat16 [", bf16 ? 1 : 2,
                ", L, ceil16(Cout), ceil32(2 Cin)] on the device of c (two planes for float32 weights, one for bfloat16)");
  } else {
    TORCH_CHECK(w.device() == c.device(), "sfno_mix: w must be on the device of c");
  }
}

// w [Cin, Cout, L, 2] fp32 -> bf16 [2, L, ceil16(Cout), ceil32(2 Cin)]: the (hi, lo) planes of the degree-major real
// form W[l][o][2 i] = Wr[i, o, l], W[l][o][2 i + 1] = Wi[i, o, l], zero-padded.  Any device.  bf16 weights: the one
// plane of the same form, [1, L, Op, Kp].
at::Tensor sfno_mix_split(const at::Tensor& w) {
  TORCH_CHECK(w.scalar_type() == at::kFloat || w.scalar_type() == at::kBFloat16,
              "sfno_mix_split: w must be float32 or bfloat16, got ", w.scalar_type());
  TORCH_CHECK(w.dim() == 4 && w.size(3) == 2 && w.size(0) >= 1, "sfno_mix_split: w [Cin, Cout, L, 2]");
  const int64_t Cin = w.size(0), Cout = w.size(1), L = w.size(2);
  const int64_t Op = ceil16(Cout), Kp = ceil32(2 * Cin);
  at::Tensor wp = at::constant_pad_nd(w.detach().permute({2, 1, 0, 3}).reshape({L, Cout, 2 * Cin}),
                                      {0, Kp - 2 * Cin, 0, Op - Cout})
                      .contiguous();
  if (w.scalar_type() == at::kBFloat16) return wp.unsqueeze(0);
  if (wp.is_cuda()) {
    const c10::DeviceGuard guard(wp.device());
    at::Tensor ts = at::empty({2, L, Op, Kp}, wp.options().dtype(at::kBFloat16));
    if (wp.numel() > 0)
      launch_split_bf16(wp.data_ptr<float>(), reinterpret_cast<uint16_t*>(ts.data_ptr()), wp.numel(),
                        static_cast<int>(Kp), false, current_stream(wp));
    return ts;
  }
  at::Tensor hi = wp.to(at::kBFloat16);
  at::Tensor lo = (wp - hi.to(at::kFloat)).to(at::kBFloat16);
  return at::stack({hi, lo}, 0).contiguous();
}

at::Tensor sfno_mix_ref(const at::Tensor& c, const at::Tensor& w, const c10::optional<at::Tensor>& ws, int64_t tri) {
  if (c.scalar_type() == at::kBFloat16)  // the bf16 operands as they are, the product in fp32, rounded once
    return sfno_mix_ref(c.to(at::kFloat), w.to(at::kFloat), c10::nullopt, tri).to(at::kBFloat16);
  at::Tensor y = at::view_as_real(at::einsum("bilm,iol->bolm", {at::view_as_complex(c.contiguous()),
                                                               at::view_as_complex(w.contiguous())}))
                     .contiguous();
  if (tri == 1) {
    at::Tensor l = at::arange(c.size(2), c.options().dtype(at::kLong)).unsqueeze(1);
    at::Tensor m = at::arange(c.size(3), c.options().dtype(at::kLong)).unsqueeze(0);
    y.masked_fill_(l.lt(m).unsqueeze(-1), 0.0);
  }
  return y;
}

// the launch path of sfno_mix and sfno_mix_out: y is the contiguous result, aligned to one (re, im) pair (8 bytes
// fp32, 4 bytes bf16: the kernel's stores)
void sfno_mix_run(const at::Tensor& c_, const at::Tensor& w_, const c10::optional<at::Tensor>& ws_, int64_t tri,
                  const at::Tensor& y) {
  const int64_t B = c_.size(0), Cin = c_.size(1), L = c_.size(2), M = c_.size(3), Cout = w_.size(1);
  const bool bf16 = c_.scalar_type() == at::kBFloat16;
  // one load per order's (re, im), 8 bytes (bf16: 4): a view at an odd element offset gets its own copy
  at::Tensor c = aligned_to(c_.contiguous(), bf16 ? 4 : 8);
  at::Tensor ws = present(ws_) ? ws_->contiguous() : sfno_mix_split(w_);
  if (y.numel() == 0) return;
  SfnoMixLaunch p;
  p.c = c.data_ptr();
  p.wh = reinterpret_cast<const uint16_t*>(ws.data_ptr());
  p.wl = bf16 ? nullptr : p.wh + ws.numel() / 2;  // fp32: the lo plane follows the hi plane
  p.y = y.data_ptr();
  p.bf16 = bf16 ? 1 : 0;
  p.B = static_cast<int>(B);
  p.Cin = static_cast<int>(Cin);
  p.Cout = static_cast<int>(Cout);
  p.L = static_cast<int>(L);
  p.M = static_cast<int>(M);
  p.tri = static_cast<int>(tri);
  launch_sfno_mix(p, current_stream(c));
}

struct SfnoMix : OpFamily {
  using Sig = at::Tensor(const at::Tensor&, const at::Tensor&, const c10::optional<at::Tensor>&, int64_t);
  static constexpr const char *name = "sfno_mix", *out_name = "sfno_mix_out";
  static constexpr auto& check = check_sfno_mix;
  template <class... A>
  static OpResult result(const at::Tensor& c, const at::Tensor& w, const A&...) {
    return {{c.size(0), w.size(1), c.size(2), c.size(3), 2}, c.options()};
  }
  template <class... A>
  static uintptr_t out_align(const at::Tensor& c, const A&...) {  // one (re, im) pair
    return 2 * c.element_size();
  }
  static constexpr auto& reference = sfno_mix_ref;
  static constexpr auto& run = sfno_mix_run;
};
AMD_DFT_OP_FAMILY(sfno_mix, SfnoMix)

// The tiling sfno_mix runs for (B, Cin, Cout, L, M, tri) -- host only, no device (the companion of legendre_info):
// "mfma coltile=64 slabs=4 otiles=4 ogroups=1 ctiles=3 lds=20480 wgs=363 grid=540 tri=1"; bf16: the same tiling with
// the bf16 instance's LDS bytes and a trailing " bf16=1"
std::string sfno_mix_info(int64_t B, int64_t Cin, int64_t Cout, int64_t L, int64_t M, int64_t tri, bool bf16) {
  TORCH_CHECK(B >= 1 && Cin >= 1 && Cout >= 1 && L >= 1 && M >= 1 && Cin < (1 << 28) && Cout < (1 << 21) &&
                  L <= 65535 && B * M < (int64_t(1) << 30),
              "amd_dft.sfno_mix_info: B, Cin, Cout, L, M must be >= 1 (L <= 65535, B * M < 2^30)");
  TORCH_CHECK(tri == 0 || tri == 1, "amd_dft.sfno_mix_info: tri must be 0 or 1");
  const SfnoMixRoute r = sfno_mix_route(B, Cin, Cout, L, M, static_cast<int>(tri), bf16);
  return "mfma coltile=" + std::to_string(r.coltile) + " slabs=" + std::to_string(r.slabs) +
         " otiles=" + std::to_string(r.otiles) + " ogroups=" + std::to_string(r.ogroups) +
         " ctiles=" + std::to_string(r.ctiles) + " lds=" + std::to_string(r.lds) + " wgs=" + std::to_string(r.wgs) +
         " grid=" + std::to_string(r.grid) + " tri=" + std::to_string(tri) + (bf16 ? " bf16=1" : "");
}

// ------------------------------------------------------------------ instance normalisation (NCHW planes)
// x [B, C, *spatial] fp32 / bf16, weight / bias [C] (fp32 or x's dtype, either may be absent):
//   y = (x - mean) * rsqrt(var + eps) * weight[c] + bias[c], biased variance over the P = prod(spatial) elements of
// each (b, c) plane -- nn.InstanceNorm2d without running statistics.  The result has x's dtype.
struct InDims {
  int64_t B, C, P;
};
InDims instance_norm_dims(const at::Tensor& x) {
  InDims d{x.size(0), x.size(1), 1};
  for (int64_t i = 2; i < x.dim(); ++i) d.P *= x.size(i);
  return d;
}
InDims check_instance_norm(const char* op, const at::Tensor& x, const c10::optional<at::Tensor>& w,
                           const c10::optional<at::Tensor>& b) {
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, op,
              ": x must be float32 or bfloat16, got ", x.scalar_type());
  TORCH_CHECK(x.dim() >= 3, op, ": x must be [B, C, *spatial] with at least one spatial dimension, got ", x.sizes());
  const InDims d = instance_norm_dims(x);
  TORCH_CHECK(d.C >= 1, op, ": x has no channels");
  TORCH_CHECK(d.P >= 2, op, ": expected more than 1 spatial element per channel, got input of size ", x.sizes());
  TORCH_CHECK(d.P < (int64_t(1) << 31) && d.C < (int64_t(1) << 31), op, ": tensor too large");
  auto per_channel = [&](const c10::optional<at::Tensor>& t, const char* name) {
    if (!present(t)) return;
    TORCH_CHECK(t->dim() == 1 && t->size(0) == d.C, op, ": ", name, " must be [C] = [", d.C, "], got ", t->sizes());
    TORCH_CHECK(t->scalar_type() == at::kFloat || t->scalar_type() == x.scalar_type(), op, ": ", name,
                " must be float32 or ", x.scalar_type(), ", got ", t->scalar_type());
    TORCH_CHECK(t->device() == x.device(), op, ": ", name, " must be on the device of x");
  };
  per_channel(w, "weight");
  per_channel(b, "bias");
  return d;
}

// CPU: fp64 ATen math on the fp32 / bf16 values, one rounding to x's dtype
std::tuple<at::Tensor, at::Tensor, at::Tensor> instance_norm_moments_cpu(const at::Tensor& x, const InDims& d,
                                                                         double eps) {
  at::Tensor xd = x.to(at::kDouble).reshape({d.B, d.C, d.P});
  at::Tensor mean = xd.mean({-1}, /*keepdim=*/true);
  at::Tensor xc = xd - mean;
  at::Tensor rstd = at::rsqrt((xc * xc).mean({-1}, /*keepdim=*/true) + eps);
  return {xc, mean, rstd};
}

at::Tensor instance_norm_ref(const at::Tensor& x, const c10::optional<at::Tensor>& w,
                             const c10::optional<at::Tensor>& b, double eps) {
  const InDims d = instance_norm_dims(x);
  if (x.numel() == 0) return at::empty_like(x, at::MemoryFormat::Contiguous);
  auto [xc, mean, rstd] = instance_norm_moments_cpu(x, d, eps);
  at::Tensor y = xc * rstd;
  if (present(w)) y = y * w->to(at::kDouble).reshape({1, d.C, 1});
  if (present(b)) y = y + b->to(at::kDouble).reshape({1, d.C, 1});
  return y.reshape(x.sizes()).to(x.scalar_type());
}

at::Tensor instance_norm_stats_cpu(const at::Tensor& x, double eps) {
  const InDims d = check_instance_norm("instance_norm_stats", x, c10::nullopt, c10::nullopt);
  if (x.numel() == 0) return at::empty({d.B, d.C, 2}, x.options().dtype(at::kFloat));
  auto [xc, mean, rstd] = instance_norm_moments_cpu(x, d, eps);
  return at::cat({mean, rstd}, -1).to(at::kFloat);
}

// the launch path of the three device ops: y (contiguous, 16-byte aligned, x's dtype) or stats ([B, C, 2] fp32)
void instance_norm_run(const InDims& d, const at::Tensor& x_, const c10::optional<at::Tensor>& w,
                       const c10::optional<at::Tensor>& b, double eps, const at::Tensor& y, const at::Tensor& stats) {
  if (x_.numel() == 0) return;
  // 16-byte vectors between the peeled ends of every plane: a view at an odd element offset gets its own copy
  at::Tensor x = vec_aligned(x_.contiguous());
  at::Tensor wf = f32_or_undef(w), bf = f32_or_undef(b);
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  const InstanceNormRoute r = instance_norm_route(d.B * d.C, d.P, bf16);
  at::Tensor part;
  if (!r.resident) part = at::empty({d.B * d.C, r.S, 4}, x.options().dtype(at::kFloat));
  InstanceNormLaunch p;
  p.x = x.data_ptr();
  p.y = y.defined() ? y.data_ptr() : nullptr;
  p.w = wf.defined() ? wf.data_ptr<float>() : nullptr;
  p.b = bf.defined() ? bf.data_ptr<float>() : nullptr;
  p.stats = stats.defined() ? stats.data_ptr<float>() : nullptr;
  p.part = part.defined() ? part.data_ptr<float>() : nullptr;
  p.planes = d.B * d.C;
  p.P = d.P;
  p.C = static_cast<int>(d.C);
  p.eps = static_cast<float>(eps);
  p.bf16 = bf16 ? 1 : 0;
  launch_instance_norm(p, current_stream(x));
}

struct InstanceNorm : OpFamily {
  using Sig = at::Tensor(const at::Tensor&, const c10::optional<at::Tensor>&, const c10::optional<at::Tensor>&, double);
  static constexpr const char *name = "instance_norm", *out_name = "instance_norm_out";
  static void check(const char* op, const at::Tensor& x, const c10::optional<at::Tensor>& w,
                    const c10::optional<at::Tensor>& b, double) {
    check_instance_norm(op, x, w, b);
  }
  template <class... A>
  static OpResult result(const at::Tensor& x, const A&...) {
    return {x.sizes(), x.options()};
  }
  template <class... A>
  static uintptr_t out_align(const A&...) {
    return 16;
  }
  static constexpr auto& reference = instance_norm_ref;
  static void run(const at::Tensor& x, const c10::optional<at::Tensor>& w, const c10::optional<at::Tensor>& b,
                  double eps, const at::Tensor& y) {
    instance_norm_run(instance_norm_dims(x), x, w, b, eps, y, at::Tensor());
  }
};
AMD_DFT_OP_FAMILY(instance_norm, InstanceNorm)

at::Tensor instance_norm_stats_cuda(const at::Tensor& x, double eps) {
  const InDims d = check_instance_norm("instance_norm_stats", x, c10::nullopt, c10::nullopt);
  const c10::DeviceGuard guard(x.device());
  at::Tensor st = at::empty({d.B, d.C, 2}, x.options().dtype(at::kFloat));
  instance_norm_run(d, x, c10::nullopt, c10::nullopt, eps, at::Tensor(), st);
  return checked(st, "instance_norm_stats");
}

at::Tensor instance_norm_stats_meta(const at::Tensor& x, double) {
  TORCH_CHECK(x.dim() >= 3, "instance_norm_stats: x must be [B, C, *spatial]");
  return at::empty({x.size(0), x.size(1), 2}, x.options().dtype(at::kFloat));
}

// The route instance_norm runs for planes = B C planes of P elements -- host only, no device (the companion of
// ln_info): "route=resident S=1 chunk=4050 vec=4 lds=16472 wgs=20" or "route=split S=64 chunk=16256 vec=4 lds=65296
// wgs=1280".  chunk: elements per workgroup (the last chunk of a plane may be shorter); lds: dynamic LDS bytes of
// the kernel that holds the data (the split route's normalising kernel takes 16).
std::string instance_norm_info(int64_t planes, int64_t P, bool bf16) {
  TORCH_CHECK(planes >= 1 && P >= 2 && P < (int64_t(1) << 31) && planes < (int64_t(1) << 31),
              "amd_dft.instance_norm_info: planes must be >= 1 and 2 <= P < 2^31");
  const InstanceNormRoute r = instance_norm_route(planes, P, bf16);
  return std::string("route=") + (r.resident ? "resident" : "split") + " S=" + std::to_string(r.S) +
         " chunk=" + std::to_string(r.chunk) + " vec=" + std::to_string(r.vec) + " lds=" + std::to_string(r.lds) +
         " wgs=" + std::to_string(r.wgs);
}

// ------------------------------------------------------------------ LayerNorm (+ residual)
std::tuple<at::Tensor, at::Tensor> layer_norm_cpu(const at::Tensor& x, const at::Tensor& w, const at::Tensor& b,
                                                  double eps, const std::optional<at::Tensor>& residual) {
  // like the kernel: the fp32 sum is normalised, x_out is its rounding (LN of the rounded x_out would carry a
  // 2^-9 |x + residual| error per element into y, far above one output rounding where |mean| >> std)
  at::Tensor xf = present(residual) ? x.to(at::kFloat) + residual->to(at::kFloat) : x.to(at::kFloat);
  at::Tensor y = at::layer_norm(xf, {x.size(-1)}, w.to(at::kFloat), b.to(at::kFloat), eps);
  return {y.to(x.scalar_type()), present(residual) ? xf.to(x.scalar_type()) : x};
}

// The LayerNorm ops' per-channel arguments hold exactly C entries (the kernels read C of them with 16-byte loads)
void check_channels(const char* op, int64_t C, const at::Tensor& w, const at::Tensor& b,
                    const c10::optional<at::Tensor>& pre) {
  TORCH_CHECK(w.numel() == C && b.numel() == C && (!present(pre) || pre->numel() == C), "amd_dft.", op,
              ": weight/bias/pre must have C = ", C, " entries");
}

std::tuple<at::Tensor, at::Tensor> layer_norm_cuda(const at::Tensor& x_, const at::Tensor& w_, const at::Tensor& b_,
                                                   double eps, const std::optional<at::Tensor>& residual) {
  const c10::DeviceGuard guard(x_.device());
  const bool res = present(residual);
  const int64_t C = x_.size(-1);
  check_channels("layer_norm", C, w_, b_, c10::nullopt);
  TORCH_CHECK(!res || residual->sizes() == x_.sizes(), "amd_dft.layer_norm: residual shape mismatch");
  const bool f32 = x_.scalar_type() == at::kFloat, bf16 = x_.scalar_type() == at::kBFloat16;
  if (!(f32 || bf16) || ln_route(res ? LnOp::LayerNormRes : LnOp::LayerNorm, C, bf16).kernel == LnKernel::None) {
    fallback_note("layer_norm", "dtype/shape outside the LayerNorm kernels");
    return layer_norm_cpu(x_, w_, b_, eps, residual);  // ATen ops on the device tensors
  }
  const at::ScalarType dt = x_.scalar_type();
  at::Tensor x = vec_aligned(x_.contiguous());
  at::Tensor w = vec_aligned(w_.to(dt).contiguous()), b = vec_aligned(b_.to(dt).contiguous());
  at::Tensor y = at::empty_like(x);
  at::Tensor xs = x;
  LayerNormLaunch p;
  p.x = x.data_ptr();
  p.y = y.data_ptr();
  p.gamma = w.data_ptr();
  p.beta = b.data_ptr();
  p.residual = nullptr;
  p.resid_out = nullptr;
  at::Tensor r;
  if (res) {
    r = vec_aligned(residual->to(at::kBFloat16).contiguous());
    xs = at::empty_like(x);
    p.residual = r.data_ptr();
    p.resid_out = xs.data_ptr();
  }
  p.cols = static_cast<int>(C);
  p.rows = x.numel() / p.cols;
  p.eps = static_cast<float>(eps);
  p.bf16 = bf16 ? 1 : 0;
  if (p.rows > 0) launch_layernorm(p, current_stream(x));
  return {y, xs};
}

std::tuple<at::Tensor, at::Tensor> layer_norm_meta(const at::Tensor& x, const at::Tensor&, const at::Tensor&, double,
                                                   const std::optional<at::Tensor>&) {
  return {at::empty_like(x), at::empty_like(x)};
}

// ------------------------------------------------------------------ fp32 LayerNorm -> bf16 split pairs
// y = [..., 2C] = [hi | lo] of LN(x + pre): the A operand of the bf16x3 fc1 GEMM (fp32 path)
at::Tensor layer_norm_split_cpu(const at::Tensor& x, const at::Tensor& w, const at::Tensor& b, double eps,
                                const std::optional<at::Tensor>& pre) {
  at::Tensor xf = x.to(at::kFloat);
  if (present(pre)) xf = xf + pre->to(at::kFloat);
  at::Tensor y = at::layer_norm(xf, {x.size(-1)}, w.to(at::kFloat), b.to(at::kFloat), eps);
  at::Tensor hi = y.to(at::kBFloat16);
  at::Tensor lo = (y - hi.to(at::kFloat)).to(at::kBFloat16);
  const int64_t C = x.size(-1);
  TORCH_CHECK(C % 32 == 0, "amd_dft.layer_norm_split: C must be a multiple of 32");
  std::vector<int64_t> v(x.sizes().begin(), x.sizes().end() - 1), o = v;
  v.insert(v.end(), {C / 32, 32});
  o.push_back(2 * C);
  return at::cat({hi.reshape(v), lo.reshape(v)}, -1).reshape(o).contiguous();  // k32-interleaved
}

at::Tensor layer_norm_split_cuda(const at::Tensor& x_, const at::Tensor& w_, const at::Tensor& b_, double eps,
                                 const std::optional<at::Tensor>& pre_) {
  const c10::DeviceGuard guard(x_.device());
  const int64_t C = x_.size(-1);
  TORCH_CHECK(x_.scalar_type() == at::kFloat && ln_route(LnOp::LayerNormSplit, C, false).kernel != LnKernel::None,
              "amd_dft.layer_norm_split: x must be float32 with C % 32 == 0 and C <= 2048");
  check_channels("layer_norm_split", C, w_, b_, pre_);
  at::Tensor x = vec_aligned(x_.contiguous());
  at::Tensor w = vec_aligned(w_.to(at::kFloat).contiguous()), b = vec_aligned(b_.to(at::kFloat).contiguous());
  at::Tensor pre = vec_aligned(f32_or_undef(pre_));
  std::vector<int64_t> os(x.sizes().begin(), x.sizes().end());
  os.back() = 2 * C;
  at::Tensor y = at::empty(os, x.options().dtype(at::kBFloat16));
  LayerNormLaunch p;
  p.x = x.data_ptr();
  p.y = y.data_ptr();
  p.gamma = w.data_ptr();
  p.beta = b.data_ptr();
  p.residual = nullptr;
  p.resid_out = nullptr;
  p.cols = static_cast<int>(C);
  p.rows = x.numel() / C;
  p.eps = static_cast<float>(eps);
  p.bf16 = 0;
  p.split_out = 1;
  p.pre = pre.defined() ? pre.data_ptr<float>() : nullptr;
  if (p.rows > 0) launch_layernorm(p, current_stream(x));
  return y;
}

at::Tensor layer_norm_split_meta(const at::Tensor& x, const at::Tensor&, const at::Tensor&, double,
                                 const std::optional<at::Tensor>&) {
  std::vector<int64_t> os(x.sizes().begin(), x.sizes().end());
  os.back() = 2 * os.back();
  return at::empty(os, x.options().dtype(at::kBFloat16));
}

// ------------------------------------------------------------------ LayerNorm statistics only
// (mean, rstd) per row of x' = x + pre: the AFNO W-transforms apply LN(x') on load.
at::Tensor ln_stats_cpu(const at::Tensor& x, const std::optional<at::Tensor>& pre, double eps) {
  at::Tensor xp = x.to(at::kFloat);
  if (present(pre)) xp = xp + pre->to(at::kFloat);
  xp = xp.reshape({-1, x.size(-1)});
  // two passes like the kernels (mean, then the centred sum of squares): an error of the mean cancels in the
  // variance to first order.  at::var_mean on the device came out 2.3x over the kernels' error model at 6 channels
  // (tests/test_layernorm.py, rows with |mean| / std up to 100).
  at::Tensor mean = xp.mean({1}, /*keepdim=*/true);
  at::Tensor d = xp - mean;
  at::Tensor var = (d * d).mean({1});
  return at::stack({mean.squeeze(1), at::rsqrt(var + eps)}, 1).contiguous();
}

at::Tensor ln_stats_cuda(const at::Tensor& x_, const std::optional<at::Tensor>& pre_, double eps) {
  const c10::DeviceGuard guard(x_.device());
  const int64_t C = x_.size(-1);
  TORCH_CHECK(!present(pre_) || pre_->numel() == C, "amd_dft.ln_stats: pre must have one entry per channel");
  const bool f32 = x_.scalar_type() == at::kFloat && ln_route(LnOp::LnStats, C, false).kernel != LnKernel::None;
  if (!f32 && (x_.scalar_type() != at::kBFloat16 || ln_route(LnOp::LnStats, C, true).kernel == LnKernel::None)) {
    fallback_note("ln_stats", "dtype/shape outside the LayerNorm kernels");
    return ln_stats_cpu(x_, pre_, eps);
  }
  at::Tensor x = vec_aligned(x_.contiguous());
  at::Tensor pre = vec_aligned(f32_or_undef(pre_));
  const int64_t rows = x.numel() / C;
  at::Tensor st = at::empty({rows, 2}, x.options().dtype(at::kFloat));
  LnStatsLaunch p;
  p.x = x.data_ptr();
  p.pre = pre.defined() ? pre.data_ptr<float>() : nullptr;
  p.stats = st.data_ptr<float>();
  p.rows = rows;
  p.cols = static_cast<int>(C);
  p.eps = static_cast<float>(eps);
  p.f32 = f32 ? 1 : 0;
  if (rows > 0) launch_ln_stats(p, current_stream(x));
  return checked(st, "ln_stats");
}

at::Tensor ln_stats_meta(const at::Tensor& x, const std::optional<at::Tensor>&, double) {
  return at::empty({x.numel() / std::max<int64_t>(x.size(-1), 1), 2}, x.options().dtype(at::kFloat));
}

// (mean, rstd) per row from [rows, nc, 2] per-64-chunk (mean, M2) partials (linear3_stats);
// shift [rows, 2] (optional): its column 0 is subtracted from the mean (statistics of an operand
// centred on that offset, e.g. c2r_ln_add_split's pairs)
static void check_merge_shift(const at::Tensor& part, const std::optional<at::Tensor>& shift) {
  TORCH_CHECK(part.dim() == 3 && part.size(2) == 2, "amd_dft.ln_stats_merge: part must be [rows, chunks, 2]");
  if (present(shift)) {
    TORCH_CHECK(shift->numel() == part.size(0) * 2 && shift->size(-1) == 2 && shift->device() == part.device(),
                "amd_dft.ln_stats_merge: shift must hold [rows, 2] on the device of part");
  }
}

at::Tensor ln_stats_merge_cpu(const at::Tensor& part, double eps, const std::optional<at::Tensor>& shift) {
  check_merge_shift(part, shift);
  at::Tensor p = part.to(at::kFloat);
  at::Tensor m = p.select(2, 0), q = p.select(2, 1);
  at::Tensor mean = m.mean(1);
  at::Tensor m2 = q.sum(1) + 64.0 * (m - mean.unsqueeze(1)).pow(2).sum(1);
  if (present(shift)) mean = mean - shift->reshape({-1, 2}).select(1, 0).to(at::kFloat);
  return at::stack({mean, at::rsqrt(m2 / (64.0 * p.size(1)) + eps)}, 1).contiguous();
}

at::Tensor ln_stats_merge_cuda(const at::Tensor& part_, double eps, const std::optional<at::Tensor>& shift_) {
  const c10::DeviceGuard guard(part_.device());
  check_merge_shift(part_, shift_);
  TORCH_CHECK(part_.scalar_type() == at::kFloat, "amd_dft.ln_stats_merge: part must be fp32 [rows, chunks, 2]");
  at::Tensor part = vec_aligned(part_.contiguous());
  at::Tensor shift = vec_aligned(f32_or_undef(shift_));  // read as float2: 8 bytes would do, the one helper serves
  at::Tensor st = at::empty({part.size(0), 2}, part.options());
  launch_ln_stats_merge(part.data_ptr<float>(), st.data_ptr<float>(), part.size(0), static_cast<int>(part.size(1)), 64,
                        static_cast<float>(eps), current_stream(part),
                        shift.defined() ? shift.data_ptr<float>() : nullptr);
  return checked(st, "ln_stats_merge");
}

at::Tensor ln_stats_merge_meta(const at::Tensor& part, double, const std::optional<at::Tensor>&) {
  return at::empty({part.size(0), 2}, part.options());
}

// The kernel of layernorm.hip a 16-byte-aligned device call of a LayerNorm op takes at channel count C -- host
// only, no device (the companion of afno_w_info).  op: layer_norm, layer_norm_res (layer_norm with a residual),
// ln_stats or layer_norm_split; bf16: the dtype of x (else fp32).  "ln_bf16<4>", "ln_bf16_res<1>", "ln_stats<2>",
// "ln_stats_768", "ln_f32<8>", "ln_f32_stats<3>", "ln_f32_split<2>", "ln_split_lds<3>": kernel<16-byte chunks per
// lane>; "fallback" where the op routes to ATen, "error" where it raises.  Answers from ln_route(), which the
// wrappers above and the launchers dispatch on.  The shipped route only: the duplicated-load split kernel
// (ln_split_kernel, MI_DFT_LN_SPLIT=dup) exists in AMD_DFT_TUNING builds alone, its switch is latched on first use
// in the process, and it is neither reported here nor covered by tests/test_layernorm.py.
std::string ln_info(std::string op, int64_t C, bool bf16) {
  const bool split = op == "layer_norm_split";
  TORCH_CHECK(op == "layer_norm" || op == "layer_norm_res" || op == "ln_stats" || split,
              "amd_dft.ln_info: op must be layer_norm, layer_norm_res, ln_stats or layer_norm_split");
  TORCH_CHECK(C >= 1, "amd_dft.ln_info: C must be >= 1");
  const LnOp o = split ? LnOp::LayerNormSplit : op == "ln_stats" ? LnOp::LnStats
                 : op == "layer_norm_res" ? LnOp::LayerNormRes : LnOp::LayerNorm;
  const LnRoute r = ln_route(o, C, bf16);
  if (r.kernel == LnKernel::None) return split ? "error" : "fallback";
  const std::string name = ln_kernel_name(r.kernel);
  return r.kernel == LnKernel::Stats768 ? name : name + "<" + std::to_string(r.nch) + ">";
}

at::Tensor afno_spectral_meta(const at::Tensor& xw, const at::Tensor&, const at::Tensor&, const at::Tensor&,
                              const at::Tensor&, double) {
  return at::empty_like(xw);
}

}  // namespace
}  // namespace amd_dft

// The dispatched ops of this file, once: name and schema.  Each has name_cuda, name_cpu and name_meta above (a
// family's come from AMD_DFT_OP_FAMILY), so an op missing from one backend fails to compile.
#define AMD_DFT_SPECTRAL_OPS(X)                                                                                       \
  X(afno_spectral, "(Tensor x, Tensor w1t, Tensor w2t, Tensor b1, Tensor b2, float lam) -> Tensor")                   \
  X(afno_mlp, "(Tensor x, Tensor w1t, Tensor w2t, Tensor b1, Tensor b2, float lam) -> Tensor")                        \
  X(afno_mlp_out, "(Tensor x, Tensor w1t, Tensor w2t, Tensor b1, Tensor b2, float lam, Tensor(a!) out) -> Tensor(a!)") \
  X(layer_norm, "(Tensor x, Tensor weight, Tensor bias, float eps, Tensor? residual=None) -> (Tensor, Tensor)")       \
  X(ln_stats, "(Tensor x, Tensor? pre=None, float eps=1e-6) -> Tensor")                                               \
  X(ln_stats_merge, "(Tensor part, float eps=1e-6, Tensor? shift=None) -> Tensor")                                    \
  X(layer_norm_split, "(Tensor x, Tensor weight, Tensor bias, float eps, Tensor? pre=None) -> Tensor")                \
  X(instance_norm, "(Tensor x, Tensor? weight=None, Tensor? bias=None, float eps=1e-5) -> Tensor")                    \
  X(instance_norm_out, "(Tensor x, Tensor? weight, Tensor? bias, float eps, Tensor(a!) out) -> Tensor(a!)")           \
  X(instance_norm_stats, "(Tensor x, float eps=1e-5) -> Tensor")                                                      \
  X(fno_mix, "(Tensor x, Tensor w, int path=0) -> Tensor")                                                            \
  X(fno_mix_out, "(Tensor x, Tensor w, int path, Tensor(a!) out) -> Tensor(a!)")                                      \
  X(fno_pointwise, "(Tensor? spec, Tensor x, Tensor w, Tensor? bias=None, bool gelu=True) -> Tensor")                 \
  X(fno_pointwise_out, "(Tensor? spec, Tensor x, Tensor w, Tensor? bias, bool gelu, Tensor(a!) out) -> Tensor(a!)")   \
  X(fno_c2r_pw, "(Tensor yw, Tensor x, Tensor wc, Tensor? bias=None, bool gelu=True) -> Tensor")                      \
  X(fno_c2r_pw_out, "(Tensor yw, Tensor x, Tensor wc, Tensor? bias, bool gelu, Tensor(a!) out) -> Tensor(a!)")        \
  X(fno_c2r, "(Tensor yw, int W, ScalarType? out_dtype=None) -> Tensor")                                              \
  X(legendre, "(Tensor x, Tensor table, Tensor? table_split=None, int tri=0) -> Tensor")                              \
  X(legendre_out, "(Tensor x, Tensor table, Tensor? table_split, int tri, Tensor(a!) out) -> Tensor(a!)")             \
  X(legendre_vec, "(Tensor x, Tensor ta, Tensor tb, Tensor? ta_split=None, Tensor? tb_split=None, int tri=0) -> Tensor") \
  X(legendre_vec_out, "(Tensor x, Tensor ta, Tensor tb, Tensor? ta_split, Tensor? tb_split, int tri, Tensor(a!) out) " \
                      "-> Tensor(a!)")                                                                                \
  X(disco, "(Tensor x, Tensor row_ptr, Tensor idx, Tensor val, int K, int nlat_out, int nlon_out) -> Tensor")         \
  X(disco_out, "(Tensor x, Tensor row_ptr, Tensor idx, Tensor val, int K, int nlat_out, int nlon_out, Tensor(a!) out) " \
               "-> Tensor(a!)")                                                                                       \
  X(disco_t, "(Tensor z, Tensor row_ptr, Tensor idx, Tensor val, int nlat_out, int nlon_out, Tensor? bias=None) "     \
             "-> Tensor")                                                                                             \
  X(disco_t_out, "(Tensor z, Tensor row_ptr, Tensor idx, Tensor val, int nlat_out, int nlon_out, Tensor? bias, "      \
                 "Tensor(a!) out) -> Tensor(a!)")                                                                     \
  X(sfno_mix, "(Tensor c, Tensor w, Tensor? w_split=None, int tri=0) -> Tensor")                                      \
  X(sfno_mix_out, "(Tensor c, Tensor w, Tensor? w_split, int tri, Tensor(a!) out) -> Tensor(a!)")

TORCH_LIBRARY_FRAGMENT(amd_dft, m) {
  AMD_DFT_SPECTRAL_OPS(AMD_DFT_DEF)
  // host only: no dispatch
  m.def("afno_spectral_supported(int H, int block_size) -> bool", &amd_dft::afno_spectral_ok);
  m.def("afno_spectral_shapes() -> int[]", &amd_dft::afno_spectral_shape_list);
  m.def("afno_mlp_info(int block_size, bool split, int tokens) -> str", &amd_dft::afno_mlp_info);
  m.def("ln_info(str op, int C, bool bf16) -> str", &amd_dft::ln_info);
  m.def("instance_norm_info(int planes, int P, bool bf16) -> str", &amd_dft::instance_norm_info);
  m.def("fno_mix_info(int B, int Cin, int Cout, int M, bool bf16=False, int path=0) -> str", &amd_dft::fno_mix_info);
  m.def("fno_pointwise_info(int cin, int cout, bool bf16, int P) -> str", &amd_dft::fno_pointwise_info);
  m.def("fno_c2r_pw_info(int cin, int cout, int m, int W, bool bf16) -> str", &amd_dft::fno_c2r_pw_info);
  m.def("legendre_info(int Q, int R, int M, int cols, int tri, bool bf16=False) -> str", &amd_dft::legendre_info);
  m.def("legendre_vec_info(int Q, int R, int M, int cols, int tri, bool bf16=False) -> str",
        &amd_dft::legendre_vec_info);
  m.def("disco_info(int planes, int nlat_in, int nlon_in, int K, int nlat_out, int nlon_out, int nnz_max, "
        "bool bf16=False) -> str",
        &amd_dft::disco_info);
  m.def("disco_t_info(int planes, int nlat_in, int nlon_in, int K, int nlat_out, int nlon_out, int nnz_max, "
        "bool bf16=False) -> str",
        &amd_dft::disco_t_info);
  m.def("sfno_mix_split(Tensor w) -> Tensor", &amd_dft::sfno_mix_split);
  m.def("sfno_mix_info(int B, int Cin, int Cout, int L, int M, int tri, bool bf16=False) -> str",
        &amd_dft::sfno_mix_info);
}
TORCH_LIBRARY_IMPL(amd_dft, CUDA, m) { AMD_DFT_SPECTRAL_OPS(AMD_DFT_IMPL_CUDA) }
TORCH_LIBRARY_IMPL(amd_dft, CPU, m) { AMD_DFT_SPECTRAL_OPS(AMD_DFT_IMPL_CPU) }
TORCH_LIBRARY_IMPL(amd_dft, Meta, m) { AMD_DFT_SPECTRAL_OPS(AMD_DFT_IMPL_META) }

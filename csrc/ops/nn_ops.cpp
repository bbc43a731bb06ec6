// Torch op layer for the non-spectral FourCastNet pieces: patchify / un-patchify and the
// fused-epilogue linear layer.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <algorithm>

#include "trace.h"
#include "../nn/gemm.h"
#include "../spectral/spectral.h"
#include "checks.h"

namespace amd_dft {
void launch_patch_remap(const void* src, void* dst, int64_t B, int C, int h, int w, bool to_tokens, void* stream,
                        int elem_bytes);

namespace {

// ------------------------------------------------------------------ shared by the ops below
void* current_stream(const c10::Device& d) { return c10::hip::getCurrentHIPStream(d.index()).stream(); }

const void* data_or_null(const at::Tensor& t) { return t.defined() ? t.data_ptr() : nullptr; }

// rows of x when its last dim is k
int64_t rows(const at::Tensor& x, int64_t k) { return x.numel() / std::max<int64_t>(k, 1); }

// empty output with the leading dims of x, last dim n and dtype d, on x's device (so also the Meta shape)
at::Tensor rows_like(const at::Tensor& x, int64_t n, at::ScalarType d) {
  std::vector<int64_t> os(x.sizes().begin(), x.sizes().end());
  os.back() = n;
  return at::empty(os, x.options().dtype(d));
}

// outputs of the statistics GEMMs: (y like x with N features, part [M, N/64, 2] fp32)
std::tuple<at::Tensor, at::Tensor> stats_outputs(const at::Tensor& x, int64_t N, at::ScalarType d) {
  return {rows_like(x, N, d), at::empty({rows(x, x.size(-1)), N / 64, 2}, x.options().dtype(at::kFloat))};
}

// One launch of the hand GEMM.  The constructor takes what every op has -- the contiguous operands, the
// fp32 bias (undefined: none), the output and the problem size -- and does the pointer casts and the int
// narrowing (gemm_supported bounds M, N and K) once; an op then sets only the GemmLaunch fields that make
// it that op.  The tensors must outlive run().
struct Gemm : GemmLaunch {
  Gemm(const at::Tensor& xt, const at::Tensor& wt, const at::Tensor& bt, const at::Tensor& yt, int64_t m, int64_t n,
       int64_t k) {
    x = reinterpret_cast<const uint16_t*>(xt.data_ptr());
    w = reinterpret_cast<const uint16_t*>(wt.data_ptr());
    bias = bt.defined() ? bt.data_ptr<float>() : nullptr;
    y = yt.data_ptr();
    M = static_cast<int>(m);
    N = static_cast<int>(n);
    K = static_cast<int>(k);
  }
  // launches on the device's current HIP stream and returns it (for a kernel that follows)
  void* run(const c10::Device& d) const {
    void* stream = current_stream(d);
    launch_gemm(*this, stream);
    return stream;
  }
};

bool bf16_gemm(const at::Tensor& x, const at::Tensor& w, int64_t M, int64_t N, int64_t K) {
  return x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16 && gemm_supported(M, N, K);
}

void check_act(const char* op, int64_t act, int64_t max_act) {
  TORCH_CHECK(act >= 0 && act <= max_act, "amd_dft.", op, ": act must be 0 (none)",
              max_act == 1 ? " or 1 (gelu)" : ", 1 (gelu), 2 (gelu, tanh form) or 3 (gelu, bf16 erf fit)");
}

// op with its prefix: the patch ops' messages carry no "amd_dft."
void check_bias(const char* op, const c10::optional<at::Tensor>& bias, int64_t N) {
  TORCH_CHECK(!present(bias) || bias->numel() == N, op, ": bias must have N entries");
}

void check_xw(const char* op, const at::Tensor& x, const at::Tensor& w) {
  TORCH_CHECK(w.dim() == 2 && x.size(-1) == w.size(1), "amd_dft.", op, ": x [..., K], w [N, K]");
}

// ------------------------------------------------------------------ patchify / un-patchify
// x [B, C, h*p, w*p] -> [B*h*w, C*p*p]
at::Tensor patchify_cpu(const at::Tensor& x, int64_t p) {
  const int64_t B = x.size(0), C = x.size(1), h = x.size(2) / p, w = x.size(3) / p;
  return x.reshape({B, C, h, p, w, p}).permute({0, 2, 4, 1, 3, 5}).reshape({B * h * w, C * p * p}).contiguous();
}

// t [B, h, w, C*p*p] (feature order (c, py, px)) -> [B, C, h*p, w*p]
at::Tensor unpatchify_cpu(const at::Tensor& t, int64_t C, int64_t h, int64_t w, int64_t p) {
  const int64_t B = t.numel() / (h * w * C * p * p);
  return t.reshape({B, h, w, C, p, p}).permute({0, 3, 1, 4, 2, 5}).reshape({B, C, h * p, w * p}).contiguous();
}

bool vec_ok(const at::Tensor& x, int64_t p) {
  return (x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat) && p == 8 && x.is_contiguous() &&
         reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0;
}

at::Tensor patchify_cuda(const at::Tensor& x_, int64_t p) {
  TORCH_CHECK(x_.dim() == 4 && x_.size(2) % p == 0 && x_.size(3) % p == 0, "patchify: x must be [B, C, h*p, w*p]");
  const c10::DeviceGuard guard(x_.device());
  at::Tensor x = x_.contiguous();
  if (!vec_ok(x, p)) {
    fallback_note("patchify", "needs bf16 / fp32, p == 8, 16-byte aligned");
    return patchify_cpu(x, p);
  }
  const int64_t B = x.size(0), C = x.size(1), h = x.size(2) / p, w = x.size(3) / p;
  at::Tensor out = at::empty({B * h * w, C * p * p}, x.options());
  launch_patch_remap(x.data_ptr(), out.data_ptr(), B, static_cast<int>(C), static_cast<int>(h), static_cast<int>(w), true,
                     current_stream(x.device()), static_cast<int>(x.element_size()));
  return out;
}

at::Tensor unpatchify_cuda(const at::Tensor& t_, int64_t C, int64_t h, int64_t w, int64_t p) {
  TORCH_CHECK(t_.numel() % (h * w * C * p * p) == 0, "unpatchify: size mismatch");
  const c10::DeviceGuard guard(t_.device());
  at::Tensor t = t_.contiguous();
  if (!vec_ok(t, p)) {
    fallback_note("unpatchify", "needs bf16 / fp32, p == 8, 16-byte aligned");
    return unpatchify_cpu(t, C, h, w, p);
  }
  const int64_t B = t.numel() / (h * w * C * p * p);
  at::Tensor out = at::empty({B, C, h * p, w * p}, t.options());
  launch_patch_remap(t.data_ptr(), out.data_ptr(), B, static_cast<int>(C), static_cast<int>(h), static_cast<int>(w), false,
                     current_stream(t.device()), static_cast<int>(t.element_size()));
  return out;
}

at::Tensor patchify_meta(const at::Tensor& x, int64_t p) {
  return at::empty({x.size(0) * (x.size(2) / p) * (x.size(3) / p), x.size(1) * p * p}, x.options());
}
at::Tensor unpatchify_meta(const at::Tensor& t, int64_t C, int64_t h, int64_t w, int64_t p) {
  return at::empty({t.numel() / (h * w * C * p * p), C, h * p, w * p}, t.options());
}

// ------------------------------------------------------------------ fused-epilogue linear
// y = act(x @ w^T + bias) (+ residual); x [..., K] bf16, w [N, K] bf16, y [..., N] bf16.
// act: 0 none, 1 GELU (erf), 2 GELU (tanh form), 3 GELU (the bf16 erf fit below).  CUDA: the hand-written
// MFMA GEMM (csrc/nn/gemm.hip) when N % 64 == 0 and K % 64 == 0 (a ragged last 256-feature panel is masked
// in the kernel), otherwise hipBLASLt through at::linear (counted: fallback_counts / MI_DFT_STRICT).
// act 3: the bf16 paths' erf GELU, x sigmoid(x q(x^2)) (csrc/nn/gelu.h: gelu_erf_fit), same constants
at::Tensor gelu_erf_fit_ref(const at::Tensor& y) {
  const at::Tensor x2 = at::clamp_max(y * y, 64.0);
  const at::Tensor z = y * (x2 * (x2 * 0.0010148165747523308 + -0.10677912831306458) + -2.3011176586151123);
  return y / (at::exp2(z) + 1.0);
}

at::Tensor apply_act_ref(const at::Tensor& y, int64_t act) {
  if (act == 1) return at::gelu(y);
  if (act == 2) return at::gelu(y, "tanh");
  if (act == 3) return gelu_erf_fit_ref(y);
  return y;
}

// x w^T + bias in fp32
at::Tensor linear_f32(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias) {
  return at::linear(x.to(at::kFloat), w.to(at::kFloat),
                    present(bias) ? c10::optional<at::Tensor>(bias->to(at::kFloat)) : c10::nullopt);
}

at::Tensor linear_ref(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, int64_t act,
                      const c10::optional<at::Tensor>& residual) {
  at::Tensor y = apply_act_ref(linear_f32(x, w, bias), act);
  if (present(residual)) y = y + residual->to(at::kFloat);
  return y.to(x.scalar_type());
}

at::Tensor linear_cpu(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, int64_t act,
                      const c10::optional<at::Tensor>& residual) {
  check_act("linear", act, 3);
  check_bias("amd_dft.linear", bias, w.size(0));
  return linear_ref(x, w, bias, act, residual);
}

at::Tensor linear_cuda(const at::Tensor& x_, const at::Tensor& w_, const c10::optional<at::Tensor>& bias,
                       int64_t act, const c10::optional<at::Tensor>& residual) {
  const c10::DeviceGuard guard(x_.device());
  check_act("linear", act, 3);
  check_xw("linear", x_, w_);
  const int64_t K = w_.size(1), N = w_.size(0), M = rows(x_, K);
  check_bias("amd_dft.linear", bias, N);
  if (!bf16_gemm(x_, w_, M, N, K)) {
    fallback_note("linear", "needs bf16 operands, N % 64 == 0, K % 64 == 0 (fp32: use linear3)");
    return linear_ref(x_, w_, bias, act, residual);
  }
  at::Tensor x = x_.contiguous(), w = w_.contiguous(), b = f32_or_undef(bias), r;
  if (present(residual)) {
    TORCH_CHECK(residual->numel() == M * N, "amd_dft.linear: residual must have the output's shape");
    r = residual->to(at::kBFloat16).contiguous();
  }
  at::Tensor y = rows_like(x, N, at::kBFloat16);
  Gemm g(x, w, b, y, M, N, K);
  g.act = static_cast<int>(act);
  g.residual = data_or_null(r);
  g.run(x.device());
  return y;
}

at::Tensor linear_meta(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>&, int64_t,
                       const c10::optional<at::Tensor>&) {
  return rows_like(x, w.size(0), x.scalar_type());
}

// ------------------------------------------------------------------ LayerNorm folded into a GEMM
// linear_ln: y = act(LN(x) W^T + b) computed from the RAW rows x (no normalised copy):
//   w = W * gamma (per k, as used by the GEMM), c1[n] = sum_k w[n, k], bias = W beta + b,
//   stats[m] = (mean_m, rstd_m) of x  ->  y = act(rstd_m * (x w^T - mean_m c1) + bias).
// c1 must be summed from the same (bf16-rounded) w the GEMM reads: x w^T - mean c1 is then
// (x - mean) w exactly, with no cancellation beyond fp32 accumulation.
void check_linear_ln(const at::Tensor& x, const at::Tensor& w, const at::Tensor& c1, const c10::optional<at::Tensor>& bias,
                     const at::Tensor& stats, int64_t act) {
  check_act("linear_ln", act, 3);
  check_xw("linear_ln", x, w);
  const int64_t N = w.size(0), M = rows(x, w.size(1));
  TORCH_CHECK(c1.numel() == N, "amd_dft.linear_ln: c1 must have N entries");
  check_bias("amd_dft.linear_ln", bias, N);
  TORCH_CHECK(stats.numel() == 2 * M && stats.size(-1) == 2, "amd_dft.linear_ln: stats must be [M, 2] (mean, rstd)");
}

at::Tensor linear_ln_ref(const at::Tensor& x, const at::Tensor& w, const at::Tensor& c1, const c10::optional<at::Tensor>& bias,
                         const at::Tensor& stats, int64_t act) {
  const int64_t K = w.size(1);
  at::Tensor xf = x.to(at::kFloat).reshape({-1, K});
  at::Tensor st = stats.to(at::kFloat).reshape({-1, 2});
  at::Tensor t = at::matmul(xf, w.to(at::kFloat).t());
  at::Tensor y = st.select(1, 1).unsqueeze(1) * (t - st.select(1, 0).unsqueeze(1) * c1.to(at::kFloat).reshape({1, -1}));
  if (present(bias)) y = y + bias->to(at::kFloat).reshape({1, -1});
  y = apply_act_ref(y, act);
  std::vector<int64_t> os(x.sizes().begin(), x.sizes().end());
  os.back() = w.size(0);
  return y.reshape(os).to(x.scalar_type());
}

// linear_ln / linear3_ln on the hand GEMM, operands checked: bf16 rows in and out, or (split) split pairs in and out
at::Tensor gemm_ln(const at::Tensor& x_, const at::Tensor& w_, const at::Tensor& c1_, const c10::optional<at::Tensor>& bias,
                   const at::Tensor& stats_, int64_t act, int64_t M, int64_t N, int64_t K, bool split) {
  at::Tensor x = x_.contiguous(), w = w_.contiguous(), b = f32_or_undef(bias);
  at::Tensor c1 = c1_.to(at::kFloat).contiguous(), stats = stats_.to(at::kFloat).contiguous();
  at::Tensor y = rows_like(x, split ? 2 * N : N, at::kBFloat16);
  Gemm g(x, w, b, y, M, N, K);
  g.act = static_cast<int>(act);
  g.ln_stats = stats.data_ptr<float>();
  g.ln_c1 = c1.data_ptr<float>();
  if (split) {
    g.split = 1;
    g.out = 2;
  }
  g.run(x.device());
  return y;
}

at::Tensor linear_ln_cpu(const at::Tensor& x, const at::Tensor& w, const at::Tensor& c1, const c10::optional<at::Tensor>& bias,
                         const at::Tensor& stats, int64_t act) {
  check_linear_ln(x, w, c1, bias, stats, act);
  return linear_ln_ref(x, w, c1, bias, stats, act);
}

at::Tensor linear_ln_cuda(const at::Tensor& x_, const at::Tensor& w_, const at::Tensor& c1_,
                          const c10::optional<at::Tensor>& bias, const at::Tensor& stats_, int64_t act) {
  const c10::DeviceGuard guard(x_.device());
  check_linear_ln(x_, w_, c1_, bias, stats_, act);
  const int64_t K = w_.size(1), N = w_.size(0), M = rows(x_, K);
  if (!bf16_gemm(x_, w_, M, N, K)) {
    fallback_note("linear_ln", "needs bf16 operands, N % 64 == 0, K % 64 == 0");
    return linear_ln_ref(x_, w_, c1_, bias, stats_, act);
  }
  return gemm_ln(x_, w_, c1_, bias, stats_, act, M, N, K, false);
}

at::Tensor linear_ln_meta(const at::Tensor& x, const at::Tensor& w, const at::Tensor&, const c10::optional<at::Tensor>&,
                          const at::Tensor&, int64_t) {
  return rows_like(x, w.size(0), x.scalar_type());
}

// ------------------------------------------------------------------ patch embedding / head
// patch_linear: tokens = patchify(x) @ w^T + bias + pos[token % (h*w)]  ([B*h*w, N] bf16)
// linear_unpatch: image = unpatchify(t @ w^T + bias)                     ([B, C, h*p, w*p])
// CUDA with p == 8 and bf16: one MFMA GEMM each, the (un)patchify folded into its operand
// gather / output scatter (csrc/nn/gemm.hip MODE 1 / 2).  The reference conv / linear +
// permute path is the CPU implementation.  The bf16x3 forms (patch_linear3 / linear_unpatch3,
// below) run the same two launches with split operands and fp32 outputs.

// fp32 token rows y [B*h*w, N] + pos [h*w, N], broadcast over the batch
at::Tensor add_pos(const at::Tensor& y, const c10::optional<at::Tensor>& pos, int64_t hw) {
  if (!present(pos)) return y;
  const int64_t N = y.size(-1);
  return (y.reshape({-1, hw, N}) + pos->to(at::kFloat).reshape({1, hw, N})).reshape({-1, N});
}

// the gather GEMM: x is the contiguous bf16 image [B, C, h*8, w*8] or (split) its planes [2, B, C, h*8, w*8];
// tokens, bias and pos are bf16 / fp32 / bf16, on the split path all fp32
at::Tensor gemm_patch(const char* op, const at::Tensor& x, const at::Tensor& w_, const c10::optional<at::Tensor>& bias,
                      const c10::optional<at::Tensor>& pos, int64_t M, int64_t N, int64_t C, int64_t h, int64_t w,
                      bool split) {
  const at::ScalarType dt = split ? at::kFloat : at::kBFloat16;
  at::Tensor wc = w_.contiguous(), b = f32_or_undef(bias), r;
  if (present(pos)) {
    TORCH_CHECK(pos->numel() == h * w * N, op, ": pos must be [h*w, N]");
    r = pos->to(dt).contiguous();
  }
  at::Tensor y = at::empty({M, N}, x.options().dtype(dt));
  Gemm g(x, wc, b, y, M, N, C * 64);
  g.residual = data_or_null(r);
  g.res_rows = static_cast<int>(h * w);
  g.gC = static_cast<int>(C);
  g.gh = static_cast<int>(h);
  g.gw = static_cast<int>(w);
  if (split) {
    g.split = 1;
    g.out = 1;
    g.x_lo = x.numel() / 2;
  }
  g.run(x.device());
  return y;
}

// the scatter GEMM: t bf16 rows or (split) split pairs, image bf16 / fp32.  N % 256 != 0 (C % 4 != 0):
// token-major GEMM with a ragged last panel, then the remap kernel
at::Tensor gemm_unpatch(const at::Tensor& t_, const at::Tensor& w_, const c10::optional<at::Tensor>& bias, int64_t M,
                        int64_t N, int64_t K, int64_t C, int64_t h, int64_t wd, bool split) {
  at::Tensor t = t_.contiguous(), wc = w_.contiguous(), b = f32_or_undef(bias);
  const int64_t B = M / (h * wd);
  at::Tensor y = at::empty({B, C, h * 8, wd * 8}, t.options().dtype(split ? at::kFloat : at::kBFloat16));
  const bool ragged = N % 256 != 0;
  at::Tensor yt = ragged ? at::empty({M, N}, y.options()) : y;
  Gemm g(t, wc, b, yt, M, N, K);
  if (!ragged) {
    g.sC = static_cast<int>(C);
    g.sh = static_cast<int>(h);
    g.sw = static_cast<int>(wd);
  }
  if (split) {
    g.split = 1;
    g.out = 1;
  }
  void* stream = g.run(t.device());
  if (ragged)
    launch_patch_remap(yt.data_ptr(), y.data_ptr(), B, static_cast<int>(C), static_cast<int>(h), static_cast<int>(wd),
                       false, stream, static_cast<int>(y.element_size()));
  return y;
}

at::Tensor patch_linear_cpu(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias,
                            const c10::optional<at::Tensor>& pos, int64_t p) {
  check_bias("patch_linear", bias, w.size(0));
  at::Tensor y = linear_ref(patchify_cpu(x, p), w, bias, 0, c10::nullopt).to(at::kFloat);
  return add_pos(y, pos, (x.size(2) / p) * (x.size(3) / p)).to(x.scalar_type()).contiguous();
}

at::Tensor patch_linear_cuda(const at::Tensor& x_, const at::Tensor& w_, const c10::optional<at::Tensor>& bias,
                             const c10::optional<at::Tensor>& pos, int64_t p) {
  const c10::DeviceGuard guard(x_.device());
  TORCH_CHECK(x_.dim() == 4 && x_.size(2) % p == 0 && x_.size(3) % p == 0, "patch_linear: x must be [B, C, h*p, w*p]");
  TORCH_CHECK(w_.dim() == 2 && w_.size(1) == x_.size(1) * p * p, "patch_linear: w must be [N, C*p*p]");
  const int64_t B = x_.size(0), C = x_.size(1), h = x_.size(2) / p, w = x_.size(3) / p, N = w_.size(0);
  const int64_t M = B * h * w, K = C * p * p;
  check_bias("patch_linear", bias, N);
  if (!(p == 8 && bf16_gemm(x_, w_, M, N, K) && x_.numel() < (int64_t(1) << 31))) {  // ATen ops on the device tensors
    fallback_note("patch_linear", "needs bf16, p == 8, N % 64 == 0 (fp32: use patch_linear3)");
    return patch_linear_cpu(x_, w_, bias, pos, p);
  }
  return gemm_patch("patch_linear", x_.contiguous(), w_, bias, pos, M, N, C, h, w, false);
}

at::Tensor patch_linear_meta(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>&,
                             const c10::optional<at::Tensor>&, int64_t p) {
  return at::empty({x.size(0) * (x.size(2) / p) * (x.size(3) / p), w.size(0)}, x.options());
}

at::Tensor linear_unpatch_cpu(const at::Tensor& t, const at::Tensor& w, const c10::optional<at::Tensor>& bias,
                              int64_t C, int64_t h, int64_t wd, int64_t p) {
  check_bias("linear_unpatch", bias, w.size(0));
  return unpatchify_cpu(linear_ref(t, w, bias, 0, c10::nullopt), C, h, wd, p);
}

at::Tensor linear_unpatch_cuda(const at::Tensor& t_, const at::Tensor& w_, const c10::optional<at::Tensor>& bias,
                               int64_t C, int64_t h, int64_t wd, int64_t p) {
  const c10::DeviceGuard guard(t_.device());
  TORCH_CHECK(w_.dim() == 2 && t_.size(-1) == w_.size(1) && w_.size(0) == C * p * p,
              "linear_unpatch: t [..., K], w [C*p*p, K] in (c, py, px) feature order");
  const int64_t K = w_.size(1), N = w_.size(0), M = rows(t_, K);
  TORCH_CHECK(M % (h * wd) == 0, "linear_unpatch: token count must be a multiple of h*w");
  check_bias("linear_unpatch", bias, N);
  if (!(p == 8 && bf16_gemm(t_, w_, M, N, K) && M * N < (int64_t(1) << 31))) {
    fallback_note("linear_unpatch", "needs bf16, p == 8, N % 64 == 0 (fp32: use linear_unpatch3)");
    return linear_unpatch_cpu(t_, w_, bias, C, h, wd, p);
  }
  return gemm_unpatch(t_, w_, bias, M, N, K, C, h, wd, false);
}

at::Tensor linear_unpatch_meta(const at::Tensor& t, const at::Tensor& w, const c10::optional<at::Tensor>&, int64_t C,
                               int64_t h, int64_t wd, int64_t p) {
  return at::empty({t.numel() / w.size(1) / (h * wd), C, h * p, wd * p}, t.options());
}

// ------------------------------------------------------------------ bf16x3 (fp32-class) GEMMs
// An fp32 operand is carried as a bf16 pair a = hi + lo (hi = bf16(a), lo = bf16(a - hi)):
// split_bf16 packs rows as [..., 2K] k32-interleaved (every 32 columns [hi(32) | lo(32)],
// rows=true) or planes [2, ...] (rows=false).
// linear3 / patch_linear3 / linear_unpatch3 take split operands and run the 3-product GEMM
// (csrc/nn/gemm.hip SPLIT mode) with fp32 accumulation and fp32 (or split-pair) outputs.
// k32-interleaved split rows: every 32 columns c.. stored as [hi(32) | lo(32)]
at::Tensor unsplit_rows(const at::Tensor& xs) {
  const int64_t K2 = xs.size(-1);
  TORCH_CHECK(K2 % 64 == 0, "amd_dft: split rows must have a last dim that is a multiple of 64");
  std::vector<int64_t> s(xs.sizes().begin(), xs.sizes().end() - 1);
  std::vector<int64_t> v = s;
  v.insert(v.end(), {K2 / 64, 2, 32});
  s.push_back(K2 / 2);
  return xs.to(at::kFloat).reshape(v).sum(-2).reshape(s);
}

at::Tensor split_ref(const at::Tensor& x, bool rows) {
  at::Tensor xf = x.to(at::kFloat);
  at::Tensor hi = xf.to(at::kBFloat16);
  at::Tensor lo = (xf - hi.to(at::kFloat)).to(at::kBFloat16);
  if (!rows) return at::stack({hi, lo}, 0).contiguous();
  const int64_t K = x.size(-1);
  TORCH_CHECK(K % 32 == 0, "amd_dft.split_bf16: rows need a last dim that is a multiple of 32");
  std::vector<int64_t> v(x.sizes().begin(), x.sizes().end() - 1), o = v;
  v.insert(v.end(), {K / 32, 32});
  o.push_back(2 * K);
  return at::cat({hi.reshape(v), lo.reshape(v)}, -1).reshape(o).contiguous();
}

at::Tensor split_bf16_cpu(const at::Tensor& x, bool rows) { return split_ref(x, rows); }

// empty bf16 pairs of x on its device: rows [..., 2K] or planes [2, ...]
at::Tensor split_like(const at::Tensor& x, bool rows) {
  std::vector<int64_t> os(x.sizes().begin(), x.sizes().end());
  if (rows) os.back() = 2 * os.back();
  else os.insert(os.begin(), 2);
  return at::empty(os, x.options().dtype(at::kBFloat16));
}

at::Tensor split_bf16_cuda(const at::Tensor& x_, bool rows) {
  const c10::DeviceGuard guard(x_.device());
  TORCH_CHECK(x_.scalar_type() == at::kFloat, "amd_dft.split_bf16: x must be float32");
  TORCH_CHECK(x_.dim() >= 1, "amd_dft.split_bf16: x must have at least one dim");
  at::Tensor x = vec_aligned(x_.contiguous());
  const int64_t cols = x.size(-1);
  TORCH_CHECK(x.numel() % 8 == 0 && (!rows || cols % 32 == 0),
              "amd_dft.split_bf16: needs multiples of 8 elements (rows: a last dim that is a multiple of 32)");
  at::Tensor y = split_like(x, rows);
  launch_split_bf16(x.data_ptr<float>(), reinterpret_cast<uint16_t*>(y.data_ptr()), x.numel(), static_cast<int>(cols),
                    rows, current_stream(x.device()));
  return y;
}

at::Tensor split_bf16_meta(const at::Tensor& x, bool rows) { return split_like(x, rows); }

void check_split_linear(const at::Tensor& xs, const at::Tensor& ws, const c10::optional<at::Tensor>& bias,
                        const char* op) {
  TORCH_CHECK(xs.scalar_type() == at::kBFloat16 && ws.scalar_type() == at::kBFloat16, "amd_dft.", op,
              ": split operands must be bfloat16 pairs");
  TORCH_CHECK(ws.dim() == 2 && ws.size(1) % 2 == 0, "amd_dft.", op, ": ws must be [N, 2K] = [hi | lo]");
  TORCH_CHECK(!present(bias) || bias->numel() == ws.size(0), "amd_dft.", op, ": bias must have N entries");
}

// split rows against split weights of the same K
void check_split_rows(const at::Tensor& xs, const at::Tensor& ws, const c10::optional<at::Tensor>& bias,
                      const char* op) {
  check_split_linear(xs, ws, bias, op);
  TORCH_CHECK(xs.size(-1) == ws.size(1), "amd_dft.", op, ": xs [..., 2K], ws [N, 2K]");
}

at::Tensor linear3_cpu(const at::Tensor& xs, const at::Tensor& ws, const c10::optional<at::Tensor>& bias, int64_t act,
                       const c10::optional<at::Tensor>& residual, bool split_out) {
  check_split_rows(xs, ws, bias, "linear3");
  check_act("linear3", act, 1);
  at::Tensor y = apply_act_ref(linear_f32(unsplit_rows(xs), unsplit_rows(ws), bias), act);
  if (present(residual)) y = y + residual->to(at::kFloat).reshape(y.sizes());
  return split_out ? split_ref(y, true) : y.contiguous();
}

at::Tensor linear3_cuda(const at::Tensor& xs_, const at::Tensor& ws_, const c10::optional<at::Tensor>& bias,
                        int64_t act, const c10::optional<at::Tensor>& residual, bool split_out) {
  const c10::DeviceGuard guard(xs_.device());
  check_split_rows(xs_, ws_, bias, "linear3");
  check_act("linear3", act, 1);
  const int64_t K = ws_.size(1) / 2, N = ws_.size(0), M = rows(xs_, 2 * K);
  TORCH_CHECK(gemm_supported(M, N, K), "amd_dft.linear3: the bf16x3 GEMM needs N % 64 == 0 and K % 64 == 0 (got N=",
              N, ", K=", K, ")");
  TORCH_CHECK(!(split_out && present(residual) && (act != 0 || present(bias))),
              "amd_dft.linear3: a split-pair output takes a residual only without activation and bias");
  at::Tensor xs = xs_.contiguous(), ws = ws_.contiguous(), b = f32_or_undef(bias), r;
  if (present(residual)) {
    TORCH_CHECK(residual->numel() == M * N, "amd_dft.linear3: residual must have the output's shape");
    r = residual->to(at::kFloat).contiguous();
  }
  at::Tensor y = rows_like(xs, split_out ? 2 * N : N, split_out ? at::kBFloat16 : at::kFloat);
  Gemm g(xs, ws, b, y, M, N, K);
  g.act = static_cast<int>(act);
  g.residual = data_or_null(r);
  g.split = 1;
  g.out = split_out ? 2 : 1;
  g.run(xs.device());
  return y;
}

at::Tensor linear3_meta(const at::Tensor& xs, const at::Tensor& ws, const c10::optional<at::Tensor>&, int64_t,
                        const c10::optional<at::Tensor>&, bool split_out) {
  return rows_like(xs, split_out ? 2 * ws.size(0) : ws.size(0), split_out ? at::kBFloat16 : at::kFloat);
}

// ------------------------------------------------------------------ fc2 with the next LayerNorm's statistics
// linear_stats, the bf16 FourCastNet block: y = x w^T + residual (bf16) and, from the same epilogue, the
// next LayerNorm's partial statistics of y + pre -- taken on the stored (bf16-rounded) y, so they
// describe exactly the tensor that LayerNorm reads: part [M, N/64, 2] = per 64-feature chunk
// (mean, M2), merged by ln_stats_merge (replaces an ln_stats pass over y).
// linear3_stats, the fp32 block: y = xs ws^T + residual (bf16x3, fp32 out) with the same partials;
// ln_stats_merge turns them into (mean, rstd) without another pass over y
std::tuple<at::Tensor, at::Tensor> chunk_partials(const at::Tensor& y, const c10::optional<at::Tensor>& pre, int64_t N) {
  at::Tensor w = y.to(at::kFloat).reshape({-1, N});
  if (present(pre)) w = w + pre->to(at::kFloat).reshape({1, N});
  w = w.reshape({w.size(0), N / 64, 64});
  at::Tensor mean = w.mean(2);
  at::Tensor m2 = (w - mean.unsqueeze(2)).pow(2).sum(2);
  return {y, at::stack({mean, m2}, 2).contiguous()};
}

void check_pre(const char* op, const c10::optional<at::Tensor>& pre, int64_t N) {
  TORCH_CHECK(!present(pre) || pre->numel() == N, "amd_dft.", op, ": pre must have N entries");
}

// the kernel always reads pre (zeros when absent): an optional load behind a branch made the compiler
// wait for it -- and for every store before it -- right where it was issued
at::Tensor stats_pre(const char* op, const c10::optional<at::Tensor>& pre, int64_t N, const at::Tensor& like) {
  check_pre(op, pre, N);
  return present(pre) ? f32_or_undef(pre) : at::zeros({N}, like.options().dtype(at::kFloat));
}

void check_linear_stats(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& pre) {
  check_xw("linear_stats", x, w);
  TORCH_CHECK(w.size(0) % 64 == 0, "amd_dft.linear_stats: N must be a multiple of 64");
  check_pre("linear_stats", pre, w.size(0));
}

std::tuple<at::Tensor, at::Tensor> linear_stats_cpu(const at::Tensor& x, const at::Tensor& w, const at::Tensor& residual,
                                                    const c10::optional<at::Tensor>& pre) {
  check_linear_stats(x, w, pre);
  return chunk_partials(linear_ref(x, w, c10::nullopt, 0, residual), pre, w.size(0));
}

std::tuple<at::Tensor, at::Tensor> linear_stats_cuda(const at::Tensor& x_, const at::Tensor& w_, const at::Tensor& residual,
                                                     const c10::optional<at::Tensor>& pre_) {
  const c10::DeviceGuard guard(x_.device());
  check_linear_stats(x_, w_, pre_);
  const int64_t K = w_.size(1), N = w_.size(0), M = rows(x_, K);
  TORCH_CHECK(residual.numel() == M * N, "amd_dft.linear_stats: residual must have the output's shape");
  if (!bf16_gemm(x_, w_, M, N, K)) {
    fallback_note("linear_stats", "needs bf16 operands, N % 64 == 0, K % 64 == 0");
    return chunk_partials(linear_ref(x_, w_, c10::nullopt, 0, residual), pre_, N);
  }
  at::Tensor x = x_.contiguous(), w = w_.contiguous(), r = residual.to(at::kBFloat16).contiguous();
  at::Tensor pre = stats_pre("linear_stats", pre_, N, x);
  auto [y, part] = stats_outputs(x, N, at::kBFloat16);
  Gemm g(x, w, at::Tensor(), y, M, N, K);
  g.residual = r.data_ptr();
  g.stats_part = part.data_ptr<float>();
  g.stats_pre = pre.data_ptr<float>();
  g.run(x.device());
  return {y, part};
}

std::tuple<at::Tensor, at::Tensor> linear_stats_meta(const at::Tensor& x, const at::Tensor& w, const at::Tensor&,
                                                     const c10::optional<at::Tensor>&) {
  return stats_outputs(x, w.size(0), x.scalar_type());
}

std::tuple<at::Tensor, at::Tensor> linear3_stats_cpu(const at::Tensor& xs, const at::Tensor& ws, const at::Tensor& residual,
                                                     const c10::optional<at::Tensor>& pre) {
  at::Tensor y = linear3_cpu(xs, ws, c10::nullopt, 0, residual, false);
  TORCH_CHECK(ws.size(0) % 64 == 0, "amd_dft.linear3_stats: N must be a multiple of 64");
  return chunk_partials(y, pre, ws.size(0));
}

// linear3_stats_pr: the residual stream carried as c2r_ln_add_split's split pairs (no fp32 copy of it):
// residual = m + (hi + lo), rpairs [M, 2N] bf16 k32-interleaved pairs of x - m, rstats [M, 2] with m = rstats[:, 0]
// (the block's LN1 statistics, which centred those pairs).  2^-18 of |x - m| off the fp32 residual.
// rlo2 (optional): the split's third term bf16(x - m - (hi + lo)) [M, N] (c2r_ln_add_split out_mode 2): the
// residual then matches the fp32 stream to ~2^-27 of |x - m| (fp32 rounding: 2^-24 of |x|)
at::Tensor pairs_residual_cpu(const at::Tensor& rpairs, const at::Tensor& rstats, int64_t N,
                              const c10::optional<at::Tensor>& rlo2) {
  at::Tensor pr = rpairs.to(at::kFloat).reshape({-1, N / 32, 2, 32});
  at::Tensor z = (pr.select(2, 0) + pr.select(2, 1)).reshape({-1, N});
  if (present(rlo2)) z = z + rlo2->to(at::kFloat).reshape({-1, N});
  return z + rstats.to(at::kFloat).reshape({-1, 2}).select(1, 0).unsqueeze(1);
}

void check_pairs_residual(const at::Tensor& rpairs, const at::Tensor& rstats, int64_t M, int64_t N) {
  TORCH_CHECK(rpairs.scalar_type() == at::kBFloat16 && rpairs.numel() == M * 2 * N,
              "amd_dft.linear3_stats_pr: rpairs must be [M, 2N] bf16 split pairs");
  TORCH_CHECK(rstats.numel() == M * 2, "amd_dft.linear3_stats_pr: rstats must be [M, 2] (shift, rstd)");
  TORCH_CHECK(N % 32 == 0, "amd_dft.linear3_stats_pr: N must be a multiple of 32");
}

std::tuple<at::Tensor, at::Tensor> linear3_stats_pr_cpu(const at::Tensor& xs, const at::Tensor& ws, const at::Tensor& rpairs,
                                                        const at::Tensor& rstats, const c10::optional<at::Tensor>& pre,
                                                        const c10::optional<at::Tensor>& rlo2) {
  const int64_t N = ws.size(0), M = rows(xs, xs.size(-1));
  check_pairs_residual(rpairs, rstats, M, N);
  return linear3_stats_cpu(xs, ws, pairs_residual_cpu(rpairs, rstats, N, rlo2), pre);
}

// Both statistics GEMMs of the fp32 block.  rstats == nullptr: residual is the [M, N] tensor, read as fp32.
// Otherwise the pairs form: residual = rpairs and rlo2, both left as the bf16 they are, with rstats as fp32.
std::tuple<at::Tensor, at::Tensor> gemm3_stats(const char* op, const at::Tensor& xs_, const at::Tensor& ws_,
                                               const at::Tensor& residual, const at::Tensor* rstats,
                                               const c10::optional<at::Tensor>& rlo2, const c10::optional<at::Tensor>& pre_) {
  const c10::DeviceGuard guard(xs_.device());
  check_split_rows(xs_, ws_, c10::nullopt, op);
  const int64_t K = ws_.size(1) / 2, N = ws_.size(0), M = rows(xs_, 2 * K);
  TORCH_CHECK(gemm_supported(M, N, K), "amd_dft.", op, ": the bf16x3 GEMM needs N % 64 == 0 and K % 64 == 0");
  at::Tensor xs = xs_.contiguous(), ws = ws_.contiguous(), r, rs, rl;
  if (rstats) {
    check_pairs_residual(residual, *rstats, M, N);
    r = residual.contiguous();
    rs = rstats->to(at::kFloat).contiguous();
    if (present(rlo2)) {
      TORCH_CHECK(rlo2->scalar_type() == at::kBFloat16 && rlo2->numel() == M * N,
                  "amd_dft.linear3_stats_pr: rlo2 must be [M, N] bf16");
      rl = rlo2->contiguous();
    }
  } else {
    TORCH_CHECK(residual.numel() == M * N, "amd_dft.", op, ": residual must have the output's shape");
    r = residual.to(at::kFloat).contiguous();
  }
  at::Tensor pre = stats_pre(op, pre_, N, xs);
  auto [y, part] = stats_outputs(xs, N, at::kFloat);
  Gemm g(xs, ws, at::Tensor(), y, M, N, K);
  g.split = 1;
  g.out = 1;
  g.residual = r.data_ptr();
  g.res_mean = rstats ? rs.data_ptr<float>() : nullptr;
  g.res_lo2 = reinterpret_cast<const uint16_t*>(data_or_null(rl));
  g.stats_part = part.data_ptr<float>();
  g.stats_pre = pre.data_ptr<float>();
  g.run(xs.device());
  return {y, part};
}

std::tuple<at::Tensor, at::Tensor> linear3_stats_cuda(const at::Tensor& xs, const at::Tensor& ws, const at::Tensor& residual,
                                                      const c10::optional<at::Tensor>& pre) {
  return gemm3_stats("linear3_stats", xs, ws, residual, nullptr, c10::nullopt, pre);
}

std::tuple<at::Tensor, at::Tensor> linear3_stats_pr_cuda(const at::Tensor& xs, const at::Tensor& ws, const at::Tensor& rpairs,
                                                         const at::Tensor& rstats, const c10::optional<at::Tensor>& pre,
                                                         const c10::optional<at::Tensor>& rlo2) {
  return gemm3_stats("linear3_stats_pr", xs, ws, rpairs, &rstats, rlo2, pre);
}

std::tuple<at::Tensor, at::Tensor> linear3_stats_meta(const at::Tensor& xs, const at::Tensor& ws, const at::Tensor&,
                                                      const c10::optional<at::Tensor>&) {
  return stats_outputs(xs, ws.size(0), at::kFloat);
}

std::tuple<at::Tensor, at::Tensor> linear3_stats_pr_meta(const at::Tensor& xs, const at::Tensor& ws, const at::Tensor&,
                                                         const at::Tensor&, const c10::optional<at::Tensor>&,
                                                         const c10::optional<at::Tensor>&) {
  return stats_outputs(xs, ws.size(0), at::kFloat);
}

// fc1 of the fp32 FourCastNet block: y = split(act(LN(x) W^T + b)) from the split pairs of the RAW
// residual stream x (the AFNO C2R epilogue writes them, c2r_ln_add_split), the LayerNorm folded into
// the bf16x3 GEMM's epilogue exactly as linear_ln does for bf16: ws = split(W * gamma),
// c1[n] = sum_k (hi + lo)(ws)[n, k] (from the split pairs the GEMM reads), bias = W beta + b,
// stats [M, 2] = (mean, rstd) of x.  Output: split-pair rows (the next GEMM's operand).
void check_linear3_ln(const at::Tensor& xs, const at::Tensor& ws, const at::Tensor& c1, const c10::optional<at::Tensor>& bias,
                      const at::Tensor& stats, int64_t act) {
  check_split_rows(xs, ws, bias, "linear3_ln");
  check_act("linear3_ln", act, 1);
  const int64_t N = ws.size(0), M = rows(xs, ws.size(1));
  TORCH_CHECK(c1.numel() == N, "amd_dft.linear3_ln: c1 must have N entries");
  TORCH_CHECK(stats.numel() == 2 * M && stats.size(-1) == 2, "amd_dft.linear3_ln: stats must be [M, 2] (mean, rstd)");
}

at::Tensor linear3_ln_cpu(const at::Tensor& xs, const at::Tensor& ws, const at::Tensor& c1, const c10::optional<at::Tensor>& bias,
                          const at::Tensor& stats, int64_t act) {
  check_linear3_ln(xs, ws, c1, bias, stats, act);
  return split_ref(linear_ln_ref(unsplit_rows(xs), unsplit_rows(ws), c1, bias, stats, act), true);
}

at::Tensor linear3_ln_cuda(const at::Tensor& xs_, const at::Tensor& ws_, const at::Tensor& c1_,
                           const c10::optional<at::Tensor>& bias, const at::Tensor& stats_, int64_t act) {
  const c10::DeviceGuard guard(xs_.device());
  check_linear3_ln(xs_, ws_, c1_, bias, stats_, act);
  const int64_t K = ws_.size(1) / 2, N = ws_.size(0), M = rows(xs_, 2 * K);
  TORCH_CHECK(gemm_supported(M, N, K), "amd_dft.linear3_ln: the bf16x3 GEMM needs N % 64 == 0 and K % 64 == 0 (got N=",
              N, ", K=", K, ")");
  return gemm_ln(xs_, ws_, c1_, bias, stats_, act, M, N, K, true);
}

at::Tensor linear3_ln_meta(const at::Tensor& xs, const at::Tensor& ws, const at::Tensor&, const c10::optional<at::Tensor>&,
                           const at::Tensor&, int64_t) {
  return rows_like(xs, 2 * ws.size(0), xs.scalar_type());
}

// xs = split planes [2, B, C, h*p, w*p] of the fp32 image; ws [N, 2*C*p*p]; fp32 tokens [B*h*w, N]
// patch_linear3 takes the image either as bf16 split planes [2, B, C, H, W] or as the raw fp32 image
// [B, C, H, W] (split here first).  Round 5 measured folding that split into the GEMM's fragment reads
// (the raw fp32 gathered into LDS, split per read): the embed GEMM went from 2.32 to 4.69 ms, more
// than the 0.90 ms split pass it removed (profiles/patch_embed_raw_f32_r5.txt), so the pass stays.
bool raw_f32_image(const at::Tensor& xs) { return xs.dim() == 4 && xs.scalar_type() == at::kFloat; }

at::Tensor patch_linear3_cpu(const at::Tensor& xs, const at::Tensor& ws, const c10::optional<at::Tensor>& bias,
                             const c10::optional<at::Tensor>& pos, int64_t p) {
  const bool raw = raw_f32_image(xs);
  check_split_linear(raw ? ws : xs, ws, bias, "patch_linear3");
  TORCH_CHECK(raw || (xs.dim() == 5 && xs.size(0) == 2),
              "amd_dft.patch_linear3: xs must be split planes [2, B, C, H, W] or the fp32 image [B, C, H, W]");
  // the split pair of the raw image is exactly what the GEMM multiplies (hi + lo of each value)
  at::Tensor planes = raw ? split_ref(xs, false) : xs;
  at::Tensor x = planes.select(0, 0).to(at::kFloat) + planes.select(0, 1).to(at::kFloat);
  at::Tensor y = linear_f32(patchify_cpu(x, p), unsplit_rows(ws), bias);
  return add_pos(y, pos, (x.size(2) / p) * (x.size(3) / p)).contiguous();
}

at::Tensor patch_linear3_cuda(const at::Tensor& xs_, const at::Tensor& ws_, const c10::optional<at::Tensor>& bias,
                              const c10::optional<at::Tensor>& pos, int64_t p) {
  const c10::DeviceGuard guard(xs_.device());
  const bool raw = raw_f32_image(xs_);
  check_split_linear(raw ? ws_ : xs_, ws_, bias, "patch_linear3");
  const int o = raw ? 0 : 1;  // leading plane dim of the split form
  TORCH_CHECK((raw || (xs_.dim() == 5 && xs_.size(0) == 2)) && xs_.size(2 + o) % p == 0 && xs_.size(3 + o) % p == 0,
              "amd_dft.patch_linear3: xs must be split planes [2, B, C, h*p, w*p] or the fp32 image [B, C, h*p, w*p]");
  const int64_t B = xs_.size(o), C = xs_.size(1 + o), h = xs_.size(2 + o) / p, w = xs_.size(3 + o) / p, N = ws_.size(0);
  const int64_t M = B * h * w, K = C * p * p;
  TORCH_CHECK(p == 8 && ws_.size(1) == 2 * K && gemm_supported(M, N, K) && xs_.numel() < (int64_t(1) << 31),
              "amd_dft.patch_linear3: needs p == 8, ws [N, 2*C*64], N % 64 == 0 and < 2^31 image elements");
  at::Tensor xs = raw ? split_bf16_cuda(xs_, false) : xs_.contiguous();
  return gemm_patch("amd_dft.patch_linear3", xs, ws_, bias, pos, M, N, C, h, w, true);
}

at::Tensor patch_linear3_meta(const at::Tensor& xs, const at::Tensor& ws, const c10::optional<at::Tensor>&,
                              const c10::optional<at::Tensor>&, int64_t p) {
  const int o = raw_f32_image(xs) ? 0 : 1;
  return at::empty({xs.size(o) * (xs.size(2 + o) / p) * (xs.size(3 + o) / p), ws.size(0)}, xs.options().dtype(at::kFloat));
}

at::Tensor linear_unpatch3_cpu(const at::Tensor& ts, const at::Tensor& ws, const c10::optional<at::Tensor>& bias,
                               int64_t C, int64_t h, int64_t wd, int64_t p) {
  check_split_linear(ts, ws, bias, "linear_unpatch3");
  return unpatchify_cpu(linear_f32(unsplit_rows(ts), unsplit_rows(ws), bias), C, h, wd, p);
}

at::Tensor linear_unpatch3_cuda(const at::Tensor& ts_, const at::Tensor& ws_, const c10::optional<at::Tensor>& bias,
                                int64_t C, int64_t h, int64_t wd, int64_t p) {
  const c10::DeviceGuard guard(ts_.device());
  check_split_linear(ts_, ws_, bias, "linear_unpatch3");
  const int64_t K = ws_.size(1) / 2, N = ws_.size(0), M = rows(ts_, 2 * K);
  TORCH_CHECK(ts_.size(-1) == 2 * K && N == C * p * p && p == 8 && M % (h * wd) == 0 && gemm_supported(M, N, K),
              "amd_dft.linear_unpatch3: ts [..., 2K], ws [C*64, 2K] in (c, py, px) order, p == 8");
  return gemm_unpatch(ts_, ws_, bias, M, N, K, C, h, wd, true);
}

at::Tensor linear_unpatch3_meta(const at::Tensor& ts, const at::Tensor& ws, const c10::optional<at::Tensor>&, int64_t C,
                                int64_t h, int64_t wd, int64_t p) {
  return at::empty({ts.numel() / ws.size(1) / (h * wd), C, h * p, wd * p}, ts.options().dtype(at::kFloat));
}

}  // namespace
}  // namespace amd_dft

// The ops of this file, once: name and schema.  Each has name_cuda, name_cpu and name_meta above, so an
// op missing from one backend fails to compile.
#define AMD_DFT_NN_OPS(X)                                                                                             \
  X(patchify, "(Tensor x, int p) -> Tensor")                                                                          \
  X(unpatchify, "(Tensor t, int C, int h, int w, int p) -> Tensor")                                                   \
  X(linear, "(Tensor x, Tensor w, Tensor? bias=None, int act=0, Tensor? residual=None) -> Tensor")                    \
  X(linear_ln, "(Tensor x, Tensor w, Tensor c1, Tensor? bias, Tensor stats, int act=0) -> Tensor")                    \
  X(patch_linear, "(Tensor x, Tensor w, Tensor? bias=None, Tensor? pos=None, int p=8) -> Tensor")                     \
  X(linear_unpatch, "(Tensor t, Tensor w, Tensor? bias, int C, int h, int w, int p=8) -> Tensor")                     \
  X(split_bf16, "(Tensor x, bool rows=True) -> Tensor")                                                               \
  X(linear3, "(Tensor xs, Tensor ws, Tensor? bias=None, int act=0, Tensor? residual=None, bool split_out=False) -> Tensor") \
  X(linear3_stats, "(Tensor xs, Tensor ws, Tensor residual, Tensor? pre=None) -> (Tensor, Tensor)")                   \
  X(linear3_stats_pr, "(Tensor xs, Tensor ws, Tensor rpairs, Tensor rstats, Tensor? pre=None, Tensor? rlo2=None) -> " \
                      "(Tensor, Tensor)")                                                                             \
  X(linear_stats, "(Tensor x, Tensor w, Tensor residual, Tensor? pre=None) -> (Tensor, Tensor)")                      \
  X(linear3_ln, "(Tensor xs, Tensor ws, Tensor c1, Tensor? bias, Tensor stats, int act=0) -> Tensor")                 \
  X(patch_linear3, "(Tensor xs, Tensor ws, Tensor? bias=None, Tensor? pos=None, int p=8) -> Tensor")                  \
  X(linear_unpatch3, "(Tensor ts, Tensor ws, Tensor? bias, int C, int h, int w, int p=8) -> Tensor")

TORCH_LIBRARY_FRAGMENT(amd_dft, m) { AMD_DFT_NN_OPS(AMD_DFT_DEF) }
TORCH_LIBRARY_IMPL(amd_dft, CUDA, m) { AMD_DFT_NN_OPS(AMD_DFT_IMPL_CUDA) }
TORCH_LIBRARY_IMPL(amd_dft, CPU, m) { AMD_DFT_NN_OPS(AMD_DFT_IMPL_CPU) }
TORCH_LIBRARY_IMPL(amd_dft, Meta, m) { AMD_DFT_NN_OPS(AMD_DFT_IMPL_META) }

// PyTorch custom-op layer for the MI355X DFT kernels (namespace `amd_dft`).
//
// Reference parity: the TensorRT plugins `Rfft` / `Irfft` version "1"
// (/root/reference/src/dft_plugins/dft_plugins.cpp:385, :475, :43) with attributes
// normalized/onesided/signal_ndim (:500-503) and their shape rules (:361-382, :415-436).
// Here they are `torch.ops.amd_dft.Rfft` / `Irfft`, registered by static initialisers on
// dlopen exactly like the reference's PluginRegistrar (:573-576).  Attribute violations
// raise (the reference only asserts: SURVEY Q2).
//
// General ops (the native building blocks):
//   r2c(x, dim, scale, keep, out_dtype)           real -> half spectrum, trailing re/im dim
//   c2r(x, dim, out_size, scale, keep, out_dtype) half spectrum -> real
//   c2c(x, dim, inverse, scale, out_dtype)
// with optional mode pruning (`keep` = (lo, hi) per transformed dim) used by the FNO/AFNO
// spectral layers.

#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPGraphsC10Utils.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <list>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <unordered_map>

#include "trace.h"
#include "../fft/fft_fixed.h"
#include "../fft/fft_plan.h"
#include "../spectral/dft_gemm.h"
#include "../spectral/spectral.h"
#include "checks.h"
#include "plan_cache.h"
#include "tuning.h"

namespace amd_dft {
namespace {

// ------------------------------------------------------------------ helpers
DType to_dtype(at::ScalarType t) {
  if (t == at::kFloat) return DType::F32;
  if (t == at::kBFloat16) return DType::BF16;
  TORCH_CHECK(false, "amd_dft: unsupported dtype ", t, " (float32 and bfloat16 are supported)");
}

struct DimSpec {
  int axis;
  int64_t n;       // full transform length
  int64_t lo, hi;  // kept / stored ranges
};

std::vector<int> norm_dims(at::IntArrayRef dim, int64_t ndim) {
  std::vector<int> d;
  for (int64_t v : dim) {
    const int64_t w = v < 0 ? v + ndim : v;
    TORCH_CHECK(w >= 0 && w < ndim, "amd_dft: dim ", v, " out of range for a tensor of rank ", ndim);
    TORCH_CHECK(std::find(d.begin(), d.end(), static_cast<int>(w)) == d.end(), "amd_dft: repeated dim ", v);
    d.push_back(static_cast<int>(w));
  }
  TORCH_CHECK(!d.empty(), "amd_dft: at least one dim must be transformed");
  return d;
}

// keep: empty or 2 entries per dim (in the order given); -1 entries mean "full".
std::vector<std::pair<int64_t, int64_t>> parse_keep(at::IntArrayRef keep, size_t nd) {
  std::vector<std::pair<int64_t, int64_t>> k(nd, {-1, -1});
  if (keep.empty()) return k;
  TORCH_CHECK(keep.size() == 2 * nd, "amd_dft: keep must have 2 entries (lo, hi) per transformed dim");
  for (size_t i = 0; i < nd; ++i) k[i] = {keep[2 * i], keep[2 * i + 1]};
  return k;
}

at::Tensor alloc_complex(const std::vector<int64_t>& logical, const at::TensorOptions& o, at::ScalarType dt) {
  std::vector<int64_t> s = logical;
  s.push_back(2);
  return at::empty(s, o.dtype(dt));
}

void run_pass_large(Kind kind, const at::Tensor& in, const at::Tensor& out, const std::vector<int64_t>& in_shape,
                    const std::vector<int64_t>& out_shape, int axis, int64_t L, int in_lo, int in_hi, int out_lo,
                    int out_hi, float scale, bool inverse, const void* add1, const void* add2);

// The kernels read a complex element with one load of the whole (re, im) pair.  A contiguous view
// at an odd scalar offset into a larger buffer is aligned to one scalar only: copy it (allocations
// are pair-aligned; a pointer test, no cost for an aligned tensor).
at::Tensor pair_aligned(const at::Tensor& x) {
  if (x.numel() == 0 || reinterpret_cast<uintptr_t>(x.data_ptr()) % (2 * x.element_size()) == 0) return x;
  return x.clone(at::MemoryFormat::Contiguous);
}

int64_t lds_limit() {
  static const int64_t lim = max_lds_length();
  return lim;
}

// LayerNorm fused into the IO of an AFNO W-direction pass (see PassDesc::ln_stats)
struct LnIO {
  const float* stats = nullptr;
  const float* gamma = nullptr;
  const float* beta = nullptr;
  const float* pre = nullptr;
};

// FNO mode mixing fused into the gather of a pruned C2C (see PassDesc::mix_w)
struct MixIO {
  const float* w = nullptr;
  int cin = 0, cout = 0;
};

// Everything of a pass descriptor that the kernel selection reads (apply_plan, set_axis_geometry, the mode windows,
// choose_tiling, finalize_vec_flags), on the host alone.  run_pass launches from it; fft_pass_info and afno_w_info
// describe from it, so what they report is what a launch decides.  `in` / `out` only have their alignment tested
// (the info ops pass none: taken as aligned).  Returns false when no tiling of the length fits LDS.
bool build_pass_desc(PassDesc& d, Kind kind, const Plan1D& plan, const std::vector<int64_t>& in_shape,
                     const std::vector<int64_t>& out_shape, int axis, int64_t in_lo, int64_t in_hi, int64_t out_lo,
                     int64_t out_hi, bool inverse, DType tin, DType tout, const void* in = nullptr,
                     void* out = nullptr) {
  d.kind = kind;
  apply_plan(d, plan);
  set_axis_geometry(d, in_shape, out_shape, axis, kind != Kind::R2C, kind != Kind::C2R);
  d.in_lo = static_cast<int32_t>(in_lo);
  d.in_hi = static_cast<int32_t>(in_hi);
  d.out_lo = static_cast<int32_t>(out_lo);
  d.out_hi = static_cast<int32_t>(out_hi);
  d.inverse = inverse ? 1 : 0;
  d.tin = tin;
  d.tout = tout;
  d.in = in;
  d.out = out;
  if (!choose_tiling(d)) return false;
  finalize_vec_flags(d, tin == DType::BF16 ? 2 : 4, tout == DType::BF16 ? 2 : 4);
  return true;
}

// Returns false only for an LnIO / MixIO pass that no specialised kernel covers (nothing launched).
bool run_pass(Kind kind, const at::Tensor& in, const at::Tensor& out, const std::vector<int64_t>& in_shape,
              const std::vector<int64_t>& out_shape, int axis, int64_t L, int in_lo, int in_hi, int out_lo,
              int out_hi, float scale, bool inverse, const void* add1 = nullptr, const void* add2 = nullptr,
              const LnIO* ln = nullptr, const MixIO* mix = nullptr) {
  if ((ln || mix) && L > lds_limit()) return false;
  if (L > lds_limit()) {
    run_pass_large(kind, in, out, in_shape, out_shape, axis, L, in_lo, in_hi, out_lo, out_hi, scale, inverse, add1,
                   add2);
    return true;
  }
  auto dp = get_plan(L, in.device());
  PassDesc d;
  TORCH_CHECK(build_pass_desc(d, kind, dp->plan, in_shape, out_shape, axis, in_lo, in_hi, out_lo, out_hi, inverse,
                              to_dtype(in.scalar_type()), to_dtype(out.scalar_type()), in.data_ptr(), out.data_ptr()),
              "amd_dft: transform length ", L, " exceeds the LDS-resident limit (", max_lds_length(), ")");
  d.tw = dp->tw.data_ptr();
  d.scale = scale;
  d.add1 = add1;
  d.add2 = add2;
  void* stream = c10::hip::getCurrentHIPStream(in.device().index()).stream();
  if (ln) {
    d.ln_stats = ln->stats;
    d.ln_gamma = ln->gamma;
    d.ln_beta = ln->beta;
    d.ln_pre = ln->pre;
    return launch_fft_fixed(d, stream);
  }
  if (mix) {
    d.mix_w = mix->w;
    d.mix_cin = mix->cin;
    d.mix_cout = mix->cout;
    return launch_fft_fixed(d, stream);
  }
  launch_fft_pass(d, stream);
  return true;
}

// ------------------------------------------------------------------ lengths beyond one LDS-resident pass
// cuFFT (the reference's backend) takes any length; the Stockham kernels keep a whole signal in
// LDS (<= lds_limit() points).  Longer transforms are composed from LDS-resident ones:
//  * four-step (Bailey): N = N1*N2 -> N1-point FFTs along the strided axis, twiddle
//    e^{-+2 pi i k1 n2 / N}, N2-point FFTs, transpose (N1, N2 recurse if still too long);
//  * Bluestein (chirp-z) when N has no usable factor (a large prime): a length-M >= 2N-1
//    smooth convolution done with the same kernels.
// The glue (twiddle multiply, transposes, padding) is ATen elementwise work on the device.
at::Tensor c2c_full(const at::Tensor& z, bool inverse);

at::Tensor c2c_lastdim_kernels(const at::Tensor& z, int axis, bool inverse) {
  // z: complex64 contiguous; transform along `axis` with the native pass (recurses if long)
  at::Tensor zr = at::view_as_real(z);
  std::vector<int64_t> shape(z.sizes().begin(), z.sizes().end());
  at::Tensor out = at::empty_like(zr);
  const int64_t n = shape[axis];
  run_pass(Kind::C2C, zr, out, shape, shape, axis, n, static_cast<int>(n), 0, static_cast<int>(n), 0, 1.f, inverse);
  return at::view_as_complex(out);
}

int64_t split_length(int64_t N) {
  // divisor closest to sqrt(N) with N1 <= limit (N2 may recurse); 0 if N is prime
  int64_t best = 0;
  const double r = std::sqrt(static_cast<double>(N));
  for (int64_t d = 2; d * d <= N; ++d) {
    if (N % d) continue;
    for (int64_t c : {d, N / d}) {
      if (c > lds_limit() || c == N) continue;
      if (!best || std::fabs(static_cast<double>(c) - r) < std::fabs(static_cast<double>(best) - r)) best = c;
    }
  }
  return best;
}

int64_t smooth_at_least(int64_t n) {
  for (int64_t m = n;; ++m) {
    int64_t k = m;
    for (int64_t p : {2, 3, 5}) while (k % p == 0) k /= p;
    if (k == 1) return m;
  }
}

at::Tensor phase_table(int64_t rows, int64_t cols, int64_t N, double sign, const at::Device& dev) {
  // exp(sign * 2 pi i * ((r * c) mod N) / N), exact integer angle reduction, fp64 trig
  auto o = at::TensorOptions().dtype(at::kLong).device(dev);
  at::Tensor idx = at::remainder(at::arange(rows, o).unsqueeze(1) * at::arange(cols, o).unsqueeze(0), N);
  at::Tensor ang = idx.to(at::kDouble) * (sign * 2.0 * M_PI / static_cast<double>(N));
  return at::polar(at::ones_like(ang), ang).to(at::kComplexFloat);
}

at::Tensor four_step(const at::Tensor& z, int64_t N1, bool inverse) {
  const int64_t N = z.size(-1), N2 = N / N1;
  std::vector<int64_t> s3(z.sizes().begin(), z.sizes().end() - 1);
  s3.push_back(N1);
  s3.push_back(N2);
  at::Tensor a = c2c_lastdim_kernels(z.reshape(s3).contiguous(), static_cast<int>(s3.size()) - 2, inverse);
  a = a * phase_table(N1, N2, N, inverse ? 1.0 : -1.0, z.device());
  a = c2c_lastdim_kernels(a.contiguous(), static_cast<int>(s3.size()) - 1, inverse);
  return a.transpose(-1, -2).reshape(z.sizes()).contiguous();
}

at::Tensor bluestein(const at::Tensor& z, bool inverse) {
  if (inverse) return at::conj_physical(bluestein(at::conj_physical(z), false));
  const int64_t N = z.size(-1), M = smooth_at_least(2 * N - 1);
  auto lo = at::TensorOptions().dtype(at::kLong).device(z.device());
  at::Tensor n = at::arange(N, lo);
  at::Tensor ang = at::remainder(n * n, 2 * N).to(at::kDouble) * (-M_PI / static_cast<double>(N));
  at::Tensor w = at::polar(at::ones_like(ang), ang).to(at::kComplexFloat);  // e^{-i pi n^2 / N}
  std::vector<int64_t> sa(z.sizes().begin(), z.sizes().end());
  sa.back() = M;
  at::Tensor a = at::zeros(sa, z.options());
  a.narrow(-1, 0, N).copy_(z * w);
  at::Tensor b = at::zeros({M}, z.options());
  at::Tensor cw = at::conj_physical(w);
  b.narrow(0, 0, N).copy_(cw);
  if (N > 1) b.narrow(0, M - N + 1, N - 1).copy_(cw.narrow(0, 1, N - 1).flip(0));
  at::Tensor fa = c2c_full(a, false), fb = c2c_full(b.unsqueeze(0), false).squeeze(0);
  at::Tensor c = c2c_full((fa * fb).contiguous(), true) * (1.0 / static_cast<double>(M));
  return (c.narrow(-1, 0, N) * w).contiguous();
}

at::Tensor c2c_full(const at::Tensor& z, bool inverse) {
  // z: complex64 contiguous [..., N]; unnormalised transform along the last dim
  const int64_t N = z.size(-1);
  if (N <= lds_limit()) return c2c_lastdim_kernels(z, static_cast<int>(z.dim()) - 1, inverse);
  const int64_t N1 = split_length(N);
  return N1 ? four_step(z, N1, inverse) : bluestein(z, inverse);
}

void run_pass_large(Kind kind, const at::Tensor& in, const at::Tensor& out, const std::vector<int64_t>& in_shape,
                    const std::vector<int64_t>& out_shape, int axis, int64_t L, int in_lo, int in_hi, int out_lo,
                    int out_hi, float scale, bool inverse, const void* add1, const void* add2) {
  const auto cf = in.options().dtype(at::kComplexFloat);
  std::vector<int64_t> full_shape = in_shape;
  full_shape[axis] = L;
  at::Tensor z;
  if (kind == Kind::R2C) {
    at::Tensor xr = in.to(at::kFloat).reshape(in_shape);
    z = at::complex(xr, at::zeros_like(xr));
  } else {
    std::vector<int64_t> s2 = in_shape;
    s2.push_back(2);
    at::Tensor st = at::view_as_complex(in.to(at::kFloat).reshape(s2).contiguous());
    z = at::zeros(full_shape, cf);
    if (kind == Kind::C2C) {
      if (in_lo) z.narrow(axis, 0, in_lo).copy_(st.narrow(axis, 0, in_lo));
      if (in_hi) z.narrow(axis, L - in_hi, in_hi).copy_(st.narrow(axis, in_lo, in_hi));
    } else {  // C2R: Hermitian extension of the stored half spectrum
      const int64_t kmax = std::min<int64_t>(in_lo, L / 2 + 1);
      z.narrow(axis, 0, kmax).copy_(st.narrow(axis, 0, kmax));
      const int64_t m = std::min<int64_t>(kmax, (L + 1) / 2) - 1;
      if (m > 0) z.narrow(axis, L - m, m).copy_(at::conj_physical(st.narrow(axis, 1, m).flip({axis})));
    }
  }
  at::Tensor r = c2c_full(z.movedim(axis, -1).contiguous(), inverse).movedim(-1, axis);
  if (scale != 1.f) r = r * static_cast<double>(scale);
  if (kind == Kind::C2R) {
    at::Tensor y = at::real(r);
    for (const void* ad : {add1, add2})
      if (ad) y = y + at::from_blob(const_cast<void*>(ad), out_shape, out.options()).to(at::kFloat);
    out.copy_(y.reshape(out.sizes()));
    return;
  }
  at::Tensor o;
  if (kind == Kind::R2C) {
    o = r.narrow(axis, 0, out_lo);
  } else {
    std::vector<at::Tensor> parts;
    if (out_lo) parts.push_back(r.narrow(axis, 0, out_lo));
    if (out_hi) parts.push_back(r.narrow(axis, L - out_hi, out_hi));
    o = parts.size() == 1 ? parts[0] : at::cat(parts, axis);
  }
  out.copy_(at::view_as_real(o.contiguous()).reshape(out.sizes()));
}

// ------------------------------------------------------------------ shape logic (shared)
struct R2CShape {
  std::vector<DimSpec> specs;  // sorted by axis ascending
  std::vector<int64_t> out_logical;
};

R2CShape r2c_shape(at::IntArrayRef sizes, at::IntArrayRef dim, at::IntArrayRef keep) {
  const int64_t nd = static_cast<int64_t>(sizes.size());
  auto dims = norm_dims(dim, nd);
  auto kp = parse_keep(keep, dims.size());
  R2CShape r;
  for (size_t i = 0; i < dims.size(); ++i) r.specs.push_back({dims[i], sizes[dims[i]], kp[i].first, kp[i].second});
  std::sort(r.specs.begin(), r.specs.end(), [](const DimSpec& a, const DimSpec& b) { return a.axis < b.axis; });
  r.out_logical.assign(sizes.begin(), sizes.end());
  for (size_t i = 0; i < r.specs.size(); ++i) {
    DimSpec& s = r.specs[i];
    const bool last = i + 1 == r.specs.size();
    TORCH_CHECK(s.n >= 1, "amd_dft: transform length must be >= 1");
    const int64_t full = last ? s.n / 2 + 1 : s.n;
    if (s.lo < 0) { s.lo = full; s.hi = 0; }
    if (s.hi < 0) s.hi = 0;
    TORCH_CHECK(!last || s.hi == 0, "amd_dft: the innermost (half-spectrum) dim keeps only low modes (hi == 0)");
    TORCH_CHECK(s.lo + s.hi <= full && s.lo >= 0, "amd_dft: kept modes (", s.lo, ", ", s.hi, ") exceed ", full);
    r.out_logical[s.axis] = s.lo + s.hi;
  }
  return r;
}

struct C2RShape {
  std::vector<DimSpec> specs;
  std::vector<int64_t> in_logical, out_real;
};

C2RShape c2r_shape(at::IntArrayRef sizes_with_2, at::IntArrayRef dim, at::IntArrayRef out_size, at::IntArrayRef keep) {
  TORCH_CHECK(sizes_with_2.size() >= 2 && sizes_with_2.back() == 2,
              "amd_dft: complex input must be a real tensor with a trailing dim of size 2");
  std::vector<int64_t> logical(sizes_with_2.begin(), sizes_with_2.end() - 1);
  const int64_t nd = static_cast<int64_t>(logical.size());
  auto dims = norm_dims(dim, nd);
  TORCH_CHECK(out_size.size() == dims.size(), "amd_dft: out_size needs one entry per transformed dim");
  auto kp = parse_keep(keep, dims.size());
  C2RShape r;
  r.in_logical = logical;
  for (size_t i = 0; i < dims.size(); ++i) r.specs.push_back({dims[i], out_size[i], kp[i].first, kp[i].second});
  std::sort(r.specs.begin(), r.specs.end(), [](const DimSpec& a, const DimSpec& b) { return a.axis < b.axis; });
  r.out_real = logical;
  for (size_t i = 0; i < r.specs.size(); ++i) {
    DimSpec& s = r.specs[i];
    const bool last = i + 1 == r.specs.size();
    const int64_t stored = logical[s.axis];
    TORCH_CHECK(s.n >= 1, "amd_dft: output length must be >= 1");
    if (s.lo < 0) { s.lo = stored; s.hi = 0; }
    if (s.hi < 0) s.hi = 0;
    TORCH_CHECK(s.lo + s.hi == stored, "amd_dft: keep (", s.lo, ", ", s.hi, ") does not match stored size ", stored,
                " along dim ", s.axis);
    const int64_t full = last ? s.n / 2 + 1 : s.n;
    TORCH_CHECK(!last || s.hi == 0, "amd_dft: the innermost (half-spectrum) dim stores only low modes (hi == 0)");
    // Inputs longer than the Hermitian half are truncated (torch.fft.irfft semantics).
    if (s.lo + s.hi > full) {
      TORCH_CHECK(s.hi == 0, "amd_dft: stored modes exceed the transform length along dim ", s.axis);
    }
    r.out_real[s.axis] = s.n;
  }
  return r;
}

// ------------------------------------------------------------------ DFT-as-GEMM (pruned R2C)
// A pruned R2C along the innermost, contiguous axis that keeps few modes runs as an MFMA GEMM
// (csrc/spectral/dft_gemm.hip) instead of a full Stockham FFT.  MI_DFT_GEMM=0 disables it.
bool use_dftw(const at::Tensor& in, const DimSpec& s, at::ScalarType out_t) {
  static const bool enabled = [] {
    const char* e = tuning_env("MI_DFT_GEMM");
    return !(e && std::string(e) == "0");
  }();
  if (!enabled || out_t != at::kFloat || !in.is_contiguous()) return false;
  if (s.axis != in.dim() - 1 || s.hi != 0) return false;
  // fp32 inputs stay on the Stockham kernels (~1e-7): the GEMM's bf16x3 split of fp32 data is
  // good to ~4e-6 relative; bf16 inputs are exact operands and get fp32-grade results.
  if (in.scalar_type() != at::kBFloat16) return false;
  if (s.n < 64 || 8 * s.lo > s.n || !dftw_r2c_supported(static_cast<int>(s.n), static_cast<int>(s.lo))) return false;
  return in.numel() < (int64_t(1) << 31);
}

void run_dftw(const at::Tensor& in, const at::Tensor& out, const DimSpec& s, float scale) {
  auto tabs = get_dft_gemm_tables(DftTable::R2C, static_cast<int>(s.n), static_cast<int>(s.lo), in.device());
  DftwR2CLaunch p;
  p.x = in.data_ptr();
  p.out = out.data_ptr();
  p.b0 = tabs.first.data_ptr();
  p.phase = tabs.second.data_ptr();
  p.R = static_cast<int>(in.numel() / s.n);
  p.W = static_cast<int>(s.n);
  p.m = static_cast<int>(s.lo);
  p.scale = scale;
  p.bf16 = in.scalar_type() == at::kBFloat16;
  launch_dftw_r2c(p, current_stream(in));
}

at::Tensor r2c_cuda(const at::Tensor& x_, at::IntArrayRef dim, double scale, at::IntArrayRef keep,
                    std::optional<at::ScalarType> out_dtype);

// Explicit DFT-GEMM R2C along the last dim (any supported dtype): [..., W] -> [..., m, 2] fp32.
at::Tensor dftw_r2c_cuda(const at::Tensor& x_, int64_t m, double scale) {
  const c10::DeviceGuard guard(x_.device());
  at::Tensor x = x_.contiguous();
  TORCH_CHECK(x.dim() >= 1 && (x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16),
              "amd_dft.dftw_r2c: x must be float32 or bfloat16");
  const int64_t W = x.size(-1);
  TORCH_CHECK(m >= 1 && m <= W / 2 + 1, "amd_dft.dftw_r2c: needs 1 <= m <= W/2+1");
  if (!dftw_r2c_supported(static_cast<int>(W), static_cast<int>(m)))  // outside the GEMM kernel: pruned Stockham R2C
  {
    const std::vector<int64_t> d{x.dim() - 1}, k{m, 0};
    return r2c_cuda(x, d, scale, k, at::kFloat);
  }
  TORCH_CHECK(x.numel() < (int64_t(1) << 31), "amd_dft.dftw_r2c: tensor too large");
  std::vector<int64_t> os(x.sizes().begin(), x.sizes().end());
  os.back() = m;
  os.push_back(2);
  at::Tensor out = at::empty(os, x.options().dtype(at::kFloat));
  if (x.numel() == 0) return out;
  DimSpec s{static_cast<int>(x.dim() - 1), W, m, 0};
  run_dftw(x, out, s, static_cast<float>(scale));
  return checked(out, "dftw_r2c");
}

at::Tensor dftw_r2c_cpu(const at::Tensor& x, int64_t m, double scale) {
  at::Tensor y = at::fft_rfft(x.to(at::kDouble), c10::nullopt, -1).narrow(-1, 0, m) * scale;
  return at::view_as_real(y.to(at::kComplexFloat).contiguous()).contiguous();
}

at::Tensor dftw_r2c_meta(const at::Tensor& x, int64_t m, double) {
  std::vector<int64_t> os(x.sizes().begin(), x.sizes().end());
  os.back() = m;
  os.push_back(2);
  return at::empty(os, x.options().dtype(at::kFloat));
}

// ------------------------------------------------------------------ CUDA (HIP) impls
at::Tensor r2c_cuda(const at::Tensor& x_, at::IntArrayRef dim, double scale, at::IntArrayRef keep,
                    std::optional<at::ScalarType> out_dtype) {
  const c10::DeviceGuard guard(x_.device());
  at::Tensor x = x_.contiguous();
  to_dtype(x.scalar_type());
  const at::ScalarType odt = out_dtype.value_or(x.scalar_type());
  to_dtype(odt);
  R2CShape sh = r2c_shape(x.sizes(), dim, keep);
  auto opts = x.options();
  if (x.numel() == 0) return alloc_complex(sh.out_logical, opts, odt).zero_();
  std::vector<int64_t> cur(x.sizes().begin(), x.sizes().end());
  at::Tensor cur_t = x;
  const int ns = static_cast<int>(sh.specs.size());
  // innermost first: R2C on the last transformed axis, then C2C outwards.
  for (int i = ns - 1; i >= 0; --i) {
    const DimSpec& s = sh.specs[i];
    std::vector<int64_t> nxt = cur;
    nxt[s.axis] = s.lo + s.hi;
    const bool final_pass = i == 0;
    at::Tensor out = alloc_complex(nxt, opts, final_pass ? odt : at::kFloat);
    const float sc = final_pass ? static_cast<float>(scale) : 1.0f;
    if (i == ns - 1 && use_dftw(cur_t, s, out.scalar_type())) {
      run_dftw(cur_t, out, s, sc);
    } else if (i == ns - 1) {
      run_pass(Kind::R2C, cur_t, out, cur, nxt, s.axis, s.n, static_cast<int>(s.n), 0, static_cast<int>(s.lo), 0,
               sc, false);
    } else {
      run_pass(Kind::C2C, cur_t, out, cur, nxt, s.axis, s.n, static_cast<int>(s.n), 0, static_cast<int>(s.lo),
               static_cast<int>(s.hi), sc, false);
    }
    cur = nxt;
    cur_t = out;
  }
  return checked(cur_t, "r2c");
}

at::Tensor c2r_cuda_impl(const at::Tensor& x_, at::IntArrayRef dim, at::IntArrayRef out_size, double scale,
                         at::IntArrayRef keep, std::optional<at::ScalarType> out_dtype,
                         const std::optional<at::Tensor>& add1, const std::optional<at::Tensor>& add2) {
  const c10::DeviceGuard guard(x_.device());
  at::Tensor x = pair_aligned(x_.contiguous());
  to_dtype(x.scalar_type());
  const at::ScalarType odt = out_dtype.value_or(x.scalar_type());
  to_dtype(odt);
  C2RShape sh = c2r_shape(x.sizes(), dim, out_size, keep);
  auto opts = x.options();
  if (x.numel() == 0) return at::zeros(sh.out_real, opts.dtype(odt));
  std::vector<int64_t> cur = sh.in_logical;
  at::Tensor cur_t = x;
  const int ns = static_cast<int>(sh.specs.size());
  // C2C (inverse) on the outer axes first (outermost first), C2R on the innermost last.
  for (int i = 0; i < ns; ++i) {
    const DimSpec& s = sh.specs[i];
    std::vector<int64_t> nxt = cur;
    nxt[s.axis] = s.n;
    const bool final_pass = i == ns - 1;
    const float sc = final_pass ? static_cast<float>(scale) : 1.0f;
    if (final_pass) {
      at::Tensor out = at::empty(nxt, opts.dtype(odt));
      const void* a1 = nullptr;
      const void* a2 = nullptr;
      for (int k = 0; k < 2; ++k) {
        const auto& ad = k == 0 ? add1 : add2;
        if (!ad.has_value()) continue;
        TORCH_CHECK(ad->sizes() == out.sizes() && ad->scalar_type() == odt && ad->is_contiguous() &&
                        ad->device() == out.device(),
                    "amd_dft.c2r_add: addend must be contiguous with the output's shape, dtype and device");
        (k == 0 ? a1 : a2) = ad->data_ptr();
      }
      const int64_t half = s.n / 2 + 1;
      const int in_lo = static_cast<int>(std::min<int64_t>(s.lo, half));
      // When more modes are stored than the half spectrum, the extra ones are ignored; the
      // stored stride along the axis stays the stored size (geometry from `cur`).
      run_pass(Kind::C2R, cur_t, out, cur, nxt, s.axis, s.n, in_lo, 0, static_cast<int>(s.n), 0, sc, true, a1, a2);
      cur_t = out;
    } else {
      at::Tensor out = alloc_complex(nxt, opts, at::kFloat);
      run_pass(Kind::C2C, cur_t, out, cur, nxt, s.axis, s.n, static_cast<int>(s.lo), static_cast<int>(s.hi),
               static_cast<int>(s.n), 0, sc, true);
      cur_t = out;
    }
    cur = nxt;
  }
  return checked(cur_t, "c2r");
}

at::Tensor c2r_cuda(const at::Tensor& x, at::IntArrayRef dim, at::IntArrayRef out_size, double scale,
                    at::IntArrayRef keep, std::optional<at::ScalarType> out_dtype) {
  return c2r_cuda_impl(x, dim, out_size, scale, keep, out_dtype, std::nullopt, std::nullopt);
}

at::Tensor c2r_add_cuda(const at::Tensor& x, at::IntArrayRef dim, at::IntArrayRef out_size, double scale,
                        at::IntArrayRef keep, const std::optional<at::Tensor>& add1,
                        const std::optional<at::Tensor>& add2, std::optional<at::ScalarType> out_dtype) {
  return c2r_cuda_impl(x, dim, out_size, scale, keep, out_dtype, add1, add2);
}

at::Tensor c2c_cuda(const at::Tensor& x_, at::IntArrayRef dim, bool inverse, double scale,
                    std::optional<at::ScalarType> out_dtype) {
  const c10::DeviceGuard guard(x_.device());
  at::Tensor x = pair_aligned(x_.contiguous());
  TORCH_CHECK(x.dim() >= 2 && x.size(-1) == 2, "amd_dft: complex input must have a trailing dim of size 2");
  to_dtype(x.scalar_type());
  const at::ScalarType odt = out_dtype.value_or(x.scalar_type());
  to_dtype(odt);
  std::vector<int64_t> cur(x.sizes().begin(), x.sizes().end() - 1);
  auto dims = norm_dims(dim, static_cast<int64_t>(cur.size()));
  std::sort(dims.begin(), dims.end());
  if (x.numel() == 0) return at::empty_like(x, x.options().dtype(odt));
  at::Tensor cur_t = x;
  for (size_t i = 0; i < dims.size(); ++i) {
    const int ax = dims[dims.size() - 1 - i];
    const bool final_pass = i + 1 == dims.size();
    at::Tensor out = alloc_complex(cur, x.options(), final_pass ? odt : at::kFloat);
    const int64_t n = cur[ax];
    run_pass(Kind::C2C, cur_t, out, cur, cur, ax, n, static_cast<int>(n), 0, static_cast<int>(n), 0,
             final_pass ? static_cast<float>(scale) : 1.0f, inverse);
    cur_t = out;
  }
  return checked(cur_t, "c2c");
}

// Pruned C2C along one axis: input stores modes [0, in_lo) u [n - in_hi, n) of a length-n
// transform, output keeps [0, out_lo) u [n - out_hi, n).  Unnormalised, times `scale`.
int64_t c2c_axis_dim(const at::Tensor& x, int64_t dim) {  // `dim` among the logical dims (without re/im), from 0
  const int64_t nd = x.dim() - 1;
  dim = dim < 0 ? dim + nd : dim;
  TORCH_CHECK(dim >= 0 && dim < nd, "amd_dft.c2c_axis: dim out of range");
  return dim;
}

// Returns the transformed dim, normalised.
int64_t check_c2c_axis(const at::Tensor& x, int64_t dim, int64_t n, int64_t in_lo, int64_t in_hi, int64_t out_lo,
                       int64_t out_hi) {
  TORCH_CHECK(x.dim() >= 2 && x.size(-1) == 2, "amd_dft.c2c_axis: complex input needs a trailing dim of size 2");
  dim = c2c_axis_dim(x, dim);
  TORCH_CHECK(n >= 1 && in_lo >= 0 && in_hi >= 0 && out_lo >= 0 && out_hi >= 0 && in_lo + in_hi <= n &&
                  out_lo + out_hi <= n && in_lo + in_hi >= 1,
              "amd_dft.c2c_axis: bad mode windows");
  TORCH_CHECK(x.size(dim) == in_lo + in_hi, "amd_dft.c2c_axis: dim ", dim, " stores ", x.size(dim),
              " modes, expected in_lo + in_hi = ", in_lo + in_hi);
  return dim;
}

at::Tensor c2c_axis_cuda(const at::Tensor& x_, int64_t dim, int64_t n, int64_t in_lo, int64_t in_hi, int64_t out_lo,
                         int64_t out_hi, bool inverse, double scale) {
  const c10::DeviceGuard guard(x_.device());
  at::Tensor x = pair_aligned(x_.contiguous());
  to_dtype(x.scalar_type());
  dim = check_c2c_axis(x, dim, n, in_lo, in_hi, out_lo, out_hi);
  std::vector<int64_t> cur(x.sizes().begin(), x.sizes().end() - 1);
  std::vector<int64_t> nxt = cur;
  nxt[dim] = out_lo + out_hi;
  at::Tensor out = alloc_complex(nxt, x.options(), at::kFloat);
  if (out.numel() == 0) return out;
  run_pass(Kind::C2C, x, out, cur, nxt, static_cast<int>(dim), n, static_cast<int>(in_lo), static_cast<int>(in_hi),
           static_cast<int>(out_lo), static_cast<int>(out_hi), static_cast<float>(scale), inverse);
  return checked(out, "c2c_axis");
}

at::Tensor c2c_axis_cpu(const at::Tensor& x, int64_t dim, int64_t n, int64_t in_lo, int64_t in_hi, int64_t out_lo,
                        int64_t out_hi, bool inverse, double scale) {
  dim = check_c2c_axis(x, dim, n, in_lo, in_hi, out_lo, out_hi);
  at::Tensor xc = at::view_as_complex(x.to(at::kDouble).contiguous());
  std::vector<int64_t> full_shape(xc.sizes().begin(), xc.sizes().end());
  full_shape[dim] = n;
  at::Tensor full = at::zeros(full_shape, xc.options());
  if (in_lo) full.narrow(dim, 0, in_lo).copy_(xc.narrow(dim, 0, in_lo));
  if (in_hi) full.narrow(dim, n - in_hi, in_hi).copy_(xc.narrow(dim, in_lo, in_hi));
  at::Tensor y = inverse ? at::fft_ifft(full, n, dim, "forward") : at::fft_fft(full, n, dim, "backward");
  y = y * scale;
  std::vector<at::Tensor> parts;
  if (out_lo) parts.push_back(y.narrow(dim, 0, out_lo));
  if (out_hi) parts.push_back(y.narrow(dim, n - out_hi, out_hi));
  at::Tensor r = parts.size() == 1 ? parts[0] : at::cat(parts, dim);
  return at::view_as_real(r.to(at::kComplexFloat).contiguous()).contiguous();
}

// FNO spectral layer middle, inverse half: ym[b, o, s, c] = sum_i xm[b, i, s, c] w[i, o, s, c]
// (complex mode mixing), then the pruned inverse C2C along s (stored modes [0, in_lo) u
// [n - in_hi, n) of a length-n transform, all n outputs), times `scale`:
//   xm [B, Cin, in_lo + in_hi, I, 2], w [Cin, Cout, (in_lo + in_hi) * I, 2] -> [B, Cout, n, I, 2].
// On the GPU the mixing runs inside the first pass' gather of the fixed column kernels (one
// kernel, the mixed modes are never stored); otherwise fno_mix + c2c_axis.
void check_mix_c2c(const at::Tensor& xm, const at::Tensor& w, int64_t n, int64_t in_lo, int64_t in_hi) {
  TORCH_CHECK(xm.dim() == 5 && xm.size(4) == 2, "amd_dft.fno_mix_c2c: xm must be [B, Cin, S, I, 2]");
  TORCH_CHECK(xm.size(2) == in_lo + in_hi && in_lo >= 0 && in_hi >= 0 && in_lo + in_hi <= n && in_lo + in_hi >= 1,
              "amd_dft.fno_mix_c2c: xm stores ", xm.size(2), " modes, expected in_lo + in_hi <= n");
  TORCH_CHECK(w.dim() >= 3 && w.size(0) == xm.size(1) && w.size(-1) == 2 &&
                  w.numel() == w.size(0) * w.size(1) * xm.size(2) * xm.size(3) * 2,
              "amd_dft.fno_mix_c2c: w must be [Cin, Cout, S * I, 2]");
}

at::Tensor fno_mix_op(const at::Tensor& x, const at::Tensor& w, int64_t path) {
  static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("amd_dft::fno_mix", "").typed<at::Tensor(
      const at::Tensor&, const at::Tensor&, int64_t)>();
  return op.call(x, w, path);
}

at::Tensor fno_mix_c2c_unfused(const at::Tensor& xm, const at::Tensor& w, int64_t n, int64_t in_lo, int64_t in_hi,
                               double scale, bool cuda, int64_t mix_path = 0) {
  const int64_t B = xm.size(0), Cin = xm.size(1), S = xm.size(2), I = xm.size(3), Cout = w.size(1);
  at::Tensor ym = fno_mix_op(xm.reshape({B, Cin, S * I, 2}), w.reshape({Cin, Cout, S * I, 2}), mix_path)
                      .reshape({B, Cout, S, I, 2});
  return cuda ? c2c_axis_cuda(ym, 2, n, in_lo, in_hi, n, 0, true, scale) : c2c_axis_cpu(ym, 2, n, in_lo, in_hi, n, 0, true, scale);
}

// Batch size from which the default mixing path is the batched MFMA GEMM (fno_mix.hip, the per-mode
// weights read once per 8-mode tile for the whole batch) + the pruned inverse C2C, instead of the
// mixing gather inside the inverse transform (which re-reads every mode's weights once per sample):
// bench/bench_fno.py --mix-path, profiles/fno_batched_mix_r4.txt.
constexpr int64_t kFnoMixMfmaMinBatch = 8;

// path: 0 = auto (by batch size, above), 1 = mixing gather inside the inverse H transform,
//       2 = batched MFMA mixing + pruned inverse C2C (two kernels)
at::Tensor fno_mix_c2c_cuda(const at::Tensor& xm_, const at::Tensor& w_, int64_t n, int64_t in_lo, int64_t in_hi,
                            double scale, int64_t path) {
  const c10::DeviceGuard guard(xm_.device());
  check_mix_c2c(xm_, w_, n, in_lo, in_hi);
  TORCH_CHECK(path >= 0 && path <= 2, "amd_dft.fno_mix_c2c: path must be 0 (auto), 1 (gather) or 2 (mfma)");
  at::Tensor xm = xm_.to(at::kFloat).contiguous();
  at::Tensor w = w_.to(at::kFloat).contiguous();
  const int64_t B = xm.size(0), Cin = xm.size(1), S = xm.size(2), I = xm.size(3), Cout = w.size(1);
  at::Tensor out = alloc_complex({B, Cout, n, I}, xm.options(), at::kFloat);
  if (out.numel() == 0) return out;
  // the MFMA kernel's LDS tile: 8 modes x (batch x 2Cin + 2Cin x 2Cout + batch x 2Cout) fp32, padded
  const int64_t Kp = (2 * Cin + 3) & ~3, Bp = (B + 15) & ~15, Np = (2 * Cout + 15) & ~15;
  const bool fits = 4 * 8 * (Bp * Kp + Kp * Np + Bp * Np) <= 160 * 1024;
  const bool mfma = path == 2 || (path == 0 && B >= kFnoMixMfmaMinBatch);
  if (mfma && fits)
    return checked(fno_mix_c2c_unfused(xm, w, n, in_lo, in_hi, scale, true, 2), "fno_mix_c2c");
  if (Cin < (int64_t(1) << 15) && Cout < (int64_t(1) << 15)) {
    const MixIO mix{w.data_ptr<float>(), static_cast<int>(Cin), static_cast<int>(Cout)};
    if (run_pass(Kind::C2C, xm, out, {B, Cout, S, I}, {B, Cout, n, I}, 2, n, static_cast<int>(in_lo),
                 static_cast<int>(in_hi), static_cast<int>(n), 0, static_cast<float>(scale), true, nullptr, nullptr,
                 nullptr, &mix))
      return checked(out, "fno_mix_c2c");
  }
  // no fixed column kernel for this length / layout: the two native kernels
  return checked(fno_mix_c2c_unfused(xm, w, n, in_lo, in_hi, scale, true), "fno_mix_c2c");
}

at::Tensor fno_mix_c2c_cpu(const at::Tensor& xm, const at::Tensor& w, int64_t n, int64_t in_lo, int64_t in_hi,
                           double scale, int64_t /*path*/) {
  check_mix_c2c(xm, w, n, in_lo, in_hi);
  return fno_mix_c2c_unfused(xm.to(at::kFloat).contiguous(), w.to(at::kFloat).contiguous(), n, in_lo, in_hi, scale, false);
}

at::Tensor fno_mix_c2c_meta(const at::Tensor& xm, const at::Tensor& w, int64_t n, int64_t, int64_t, double, int64_t) {
  return at::empty({xm.size(0), w.size(1), n, xm.size(3), 2}, xm.options().dtype(at::kFloat));
}

at::Tensor c2c_axis_meta(const at::Tensor& x, int64_t dim, int64_t n, int64_t in_lo, int64_t in_hi, int64_t out_lo,
                         int64_t out_hi, bool, double) {
  std::vector<int64_t> s(x.sizes().begin(), x.sizes().end());
  s[c2c_axis_dim(x, dim)] = out_lo + out_hi;
  return at::empty(s, x.options().dtype(at::kFloat));
}

// ------------------------------------------------------------------ CPU impls (torch.fft)
at::Tensor select_modes(at::Tensor y, int axis, int64_t lo, int64_t hi) {
  const int64_t n = y.size(axis);
  if (lo + hi == n && hi == 0) return y;
  if (hi == 0) return y.narrow(axis, 0, lo);
  return at::cat({y.narrow(axis, 0, lo), y.narrow(axis, n - hi, hi)}, axis);
}

at::Tensor r2c_cpu(const at::Tensor& x, at::IntArrayRef dim, double scale, at::IntArrayRef keep,
                   std::optional<at::ScalarType> out_dtype) {
  to_dtype(x.scalar_type());
  const at::ScalarType odt = out_dtype.value_or(x.scalar_type());
  to_dtype(odt);
  R2CShape sh = r2c_shape(x.sizes(), dim, keep);
  std::vector<int64_t> dims;
  for (auto& s : sh.specs) dims.push_back(s.axis);
  at::Tensor y = at::fft_rfftn(x.to(at::kFloat), std::nullopt, dims, "backward");
  for (auto& s : sh.specs) y = select_modes(y, s.axis, s.lo, s.hi);
  at::Tensor r = at::view_as_real(y.contiguous()).mul(scale);
  return r.to(odt).contiguous();
}

at::Tensor c2r_cpu(const at::Tensor& x, at::IntArrayRef dim, at::IntArrayRef out_size, double scale,
                   at::IntArrayRef keep, std::optional<at::ScalarType> out_dtype) {
  to_dtype(x.scalar_type());
  const at::ScalarType odt = out_dtype.value_or(x.scalar_type());
  to_dtype(odt);
  C2RShape sh = c2r_shape(x.sizes(), dim, out_size, keep);
  at::Tensor X = at::view_as_complex(x.to(at::kFloat).contiguous());
  const size_t ns = sh.specs.size();
  std::vector<int64_t> dims, sizes;
  for (size_t i = 0; i < ns; ++i) {
    const DimSpec& s = sh.specs[i];
    dims.push_back(s.axis);
    sizes.push_back(s.n);
    const bool last = i + 1 == ns;
    const int64_t full = last ? s.n / 2 + 1 : s.n;
    if (s.lo + s.hi > full) {
      X = X.narrow(s.axis, 0, full);
      continue;
    }
    if (s.lo + s.hi == full) continue;
    std::vector<int64_t> zs(X.sizes().begin(), X.sizes().end());
    zs[s.axis] = full;
    at::Tensor Z = at::zeros(zs, X.options());
    Z.narrow(s.axis, 0, s.lo).copy_(X.narrow(s.axis, 0, s.lo));
    if (s.hi > 0) Z.narrow(s.axis, full - s.hi, s.hi).copy_(X.narrow(s.axis, s.lo, s.hi));
    X = Z;
  }
  at::Tensor y = at::fft_irfftn(X, sizes, dims, "forward").mul(scale);
  return y.to(odt).contiguous();
}

at::Tensor c2r_add_cpu(const at::Tensor& x, at::IntArrayRef dim, at::IntArrayRef out_size, double scale,
                       at::IntArrayRef keep, const std::optional<at::Tensor>& add1,
                       const std::optional<at::Tensor>& add2, std::optional<at::ScalarType> out_dtype) {
  at::Tensor y = c2r_cpu(x, dim, out_size, scale, keep, at::kFloat);
  if (add1.has_value()) y = y + add1->to(at::kFloat);
  if (add2.has_value()) y = y + add2->to(at::kFloat);
  return y.to(out_dtype.value_or(x.scalar_type())).contiguous();
}

at::Tensor c2c_cpu(const at::Tensor& x, at::IntArrayRef dim, bool inverse, double scale,
                   std::optional<at::ScalarType> out_dtype) {
  TORCH_CHECK(x.dim() >= 2 && x.size(-1) == 2, "amd_dft: complex input must have a trailing dim of size 2");
  to_dtype(x.scalar_type());
  const at::ScalarType odt = out_dtype.value_or(x.scalar_type());
  to_dtype(odt);
  auto dims = norm_dims(dim, x.dim() - 1);
  std::vector<int64_t> d64(dims.begin(), dims.end());
  at::Tensor X = at::view_as_complex(x.to(at::kFloat).contiguous());
  at::Tensor y = inverse ? at::fft_ifftn(X, std::nullopt, d64, "forward") : at::fft_fftn(X, std::nullopt, d64, "backward");
  return at::view_as_real(y.contiguous()).mul(scale).to(odt).contiguous();
}

// ------------------------------------------------------------------ Meta impls
at::Tensor r2c_meta(const at::Tensor& x, at::IntArrayRef dim, double, at::IntArrayRef keep,
                    std::optional<at::ScalarType> out_dtype) {
  R2CShape sh = r2c_shape(x.sizes(), dim, keep);
  return alloc_complex(sh.out_logical, x.options(), out_dtype.value_or(x.scalar_type()));
}
at::Tensor c2r_meta(const at::Tensor& x, at::IntArrayRef dim, at::IntArrayRef out_size, double,
                    at::IntArrayRef keep, std::optional<at::ScalarType> out_dtype) {
  C2RShape sh = c2r_shape(x.sizes(), dim, out_size, keep);
  return at::empty(sh.out_real, x.options().dtype(out_dtype.value_or(x.scalar_type())));
}
at::Tensor c2r_add_meta(const at::Tensor& x, at::IntArrayRef dim, at::IntArrayRef out_size, double scale,
                        at::IntArrayRef keep, const std::optional<at::Tensor>&, const std::optional<at::Tensor>&,
                        std::optional<at::ScalarType> out_dtype) {
  return c2r_meta(x, dim, out_size, scale, keep, out_dtype);
}
at::Tensor c2c_meta(const at::Tensor& x, at::IntArrayRef, bool, double, std::optional<at::ScalarType> out_dtype) {
  return at::empty_like(x, x.options().dtype(out_dtype.value_or(x.scalar_type())));
}

// ------------------------------------------------------------------ LayerNorm-fused AFNO W passes
// x' = x + pre (per channel), LN(x') = (x' - mean) * rstd * gamma + beta with per-token stats
// from ln_stats.  Channel-last [..., W, C]: the transform axis is dim -2, channels last.  Four ops:
//   r2c_ln            scale * rfft_W(LN(x'))[..., :keep, :, :]
//   c2r_ln_add        out = scale * irfft_W(X) + x' + LN(x'),  X = [..., km, C, 2], x = stored residual stream [..., W, C]
//   c2r_ln_add_split  fp32: (out, its bf16x3 split-pair rows, its per-64-channel LayerNorm partials)
//   c2r_ln_add_part   bf16: (out, its per-64-channel LayerNorm partials)
// They share their checks (check_wln), their canonical arguments (WlnArgs), their route (wln_route, which
// afno_w_info reports) and the one launch of the kernels of afno_wfft.hip (launch_wln).
enum class WlnOp { R2cLn, C2rLnAdd, C2rLnAddSplit, C2rLnAddPart };
constexpr const char* kWlnNames[] = {"r2c_ln", "c2r_ln_add", "c2r_ln_add_split", "c2r_ln_add_part"};  // by WlnOp
const char* wln_name(WlnOp op) { return kWlnNames[static_cast<int>(op)]; }

// pre: undefined for none
at::Tensor ln_apply(const at::Tensor& x, const at::Tensor& stats, const at::Tensor& g, const at::Tensor& b,
                    const at::Tensor& pre, at::Tensor* xp_out) {
  at::Tensor xp = x.to(at::kFloat);
  if (pre.defined()) xp = xp + pre.to(at::kFloat);
  std::vector<int64_t> ss(x.sizes().begin(), x.sizes().end());
  ss.back() = 1;
  at::Tensor st = stats.to(at::kFloat).reshape({-1, 2});
  at::Tensor mean = st.select(1, 0).reshape(ss), rstd = st.select(1, 1).reshape(ss);
  if (xp_out) *xp_out = xp;
  return (xp - mean) * rstd * g.to(at::kFloat) + b.to(at::kFloat);
}

// ---- checks, the same on every backend and before any work
void check_ln_args(const at::Tensor& x, int64_t dim, const at::Tensor& stats, const at::Tensor& g,
                   const at::Tensor& b, const std::optional<at::Tensor>& pre, const char* op) {
  TORCH_CHECK(x.dim() >= 2, "amd_dft.", op, ": needs a [..., W, C] channel-last tensor");
  TORCH_CHECK(dim == x.dim() - 2 || dim == -2, "amd_dft.", op, ": the transform axis must be dim -2 (channel-last)");
  const int64_t C = x.size(-1);
  TORCH_CHECK(g.numel() == C && b.numel() == C && (!pre.has_value() || pre->numel() == C), "amd_dft.", op,
              ": gamma/beta/pre must have one entry per channel");
  TORCH_CHECK(stats.numel() == 2 * (x.numel() / std::max<int64_t>(C, 1)), "amd_dft.", op,
              ": stats must hold (mean, rstd) per token");
}

void check_c2r_ln_spec(const at::Tensor& X, const at::Tensor& x, int64_t n, const char* op) {
  const int64_t axis = x.dim() - 2;
  TORCH_CHECK(X.dim() == x.dim() + 1 && X.size(-1) == 2 && x.size(axis) == n &&
                  X.sizes().slice(0, axis) == x.sizes().slice(0, axis) && X.size(axis + 1) == x.size(-1) &&
                  X.size(axis) <= n / 2 + 1,
              "amd_dft.", op, ": X must be [..., km, C, 2] with the leading dims and C of x and km <= n/2+1");
}

// Why an op takes no call of these dtypes / this channel count, on any backend (nullptr: it does).  `in` is the dtype
// of the transform's input (x for r2c_ln, X for the C2R ops), `out` of its output (the C2R ops': the residual stream's).
const char* wln_refusal(WlnOp op, int64_t C, at::ScalarType in, at::ScalarType out) {
  const bool split = op == WlnOp::C2rLnAddSplit, part = op == WlnOp::C2rLnAddPart;
  if (split && !(in == at::kFloat && out == at::kFloat)) return "split-pair outputs come with the fp32 residual stream";
  if (part && !(in == at::kBFloat16 && out == at::kBFloat16))
    return "bf16 spectrum and residual stream (the fp32 block uses c2r_ln_add_split)";
  if ((split || part) && C % 64 != 0) return "C must be a multiple of 64";
  return nullptr;
}

// X is not looked at for r2c_ln, nor n; out_mode only for c2r_ln_add_split
void check_wln(WlnOp op, const at::Tensor& X, const at::Tensor& x, int64_t dim, int64_t n, const at::Tensor& stats,
               const at::Tensor& g, const at::Tensor& b, const std::optional<at::Tensor>& pre, int64_t out_mode = 1) {
  const char* name = wln_name(op);
  check_ln_args(x, dim, stats, g, b, pre, name);
  if (op == WlnOp::R2cLn) return;
  const char* why = wln_refusal(op, x.size(-1), X.scalar_type(), x.scalar_type());
  TORCH_CHECK(!why, "amd_dft.", name, ": ", why);
  TORCH_CHECK(op != WlnOp::C2rLnAddSplit || (out_mode >= 0 && out_mode <= 2), "amd_dft.", name,
              ": out_mode must be 0, 1 or 2");
  check_c2r_ln_spec(X, x, n, name);
}

// ---- results, written once: the device forms allocate with these, the meta forms return them
int64_t r2c_ln_kept(const at::Tensor& x, int64_t keep) {  // keep < 0: the whole half spectrum
  const std::vector<int64_t> dv{x.dim() - 2}, kv{keep, 0};
  return r2c_shape(x.sizes(), dv, kv).specs[0].lo;
}

at::Tensor r2c_ln_empty(const at::Tensor& x, int64_t km, std::optional<at::ScalarType> out_dtype) {
  std::vector<int64_t> s(x.sizes().begin(), x.sizes().end());
  s[x.dim() - 2] = km;
  return alloc_complex(s, x.options(), out_dtype.value_or(x.scalar_type()));
}

at::Tensor c2r_ln_add_empty(const at::Tensor& x) { return at::empty(x.sizes(), x.options()); }

at::Tensor ln_partials_empty(const at::Tensor& x) {  // [tokens, C/64, 2] fp32
  const int64_t C = x.size(-1);
  return at::empty({x.numel() / std::max<int64_t>(C, 1), C / 64, 2}, x.options().dtype(at::kFloat));
}

// (out [..., W, C] bf16, part)
std::tuple<at::Tensor, at::Tensor> c2r_ln_add_part_empty(const at::Tensor& x) {
  return {c2r_ln_add_empty(x), ln_partials_empty(x)};
}

// (first, pairs [tokens, 2C] bf16, part); first by out_mode: 1 the fp32 output [..., W, C]; 2 instead its bf16
// third split term (lo2, [tokens, C]); 0 neither
std::tuple<at::Tensor, at::Tensor, at::Tensor> c2r_ln_add_split_empty(const at::Tensor& x, int64_t out_mode) {
  const int64_t C = x.size(-1), M = x.numel() / std::max<int64_t>(C, 1);
  const auto bf = x.options().dtype(at::kBFloat16);
  return {out_mode == 1 ? c2r_ln_add_empty(x) : out_mode == 2 ? at::empty({M, C}, bf) : at::empty({0}, x.options()),
          at::empty({M, 2 * C}, bf), ln_partials_empty(x)};
}

// ---- canonical arguments of a device call
struct WlnArgs {
  at::Tensor x, X;                     // contiguous, 16-byte aligned; X undefined for r2c_ln
  at::Tensor stats, gamma, beta, pre;  // fp32, contiguous, 16-byte aligned; pre undefined when there is none
  int64_t axis = 0, n = 0, C = 0;      // the transform axis (dim -2) and length, channels
  int64_t km = 0;                      // modes kept (r2c_ln) or stored in X
  int64_t M = 0, O = 0;                // tokens; [n, C] planes
  const float* pre_ptr() const { return pre.defined() ? pre.data_ptr<float>() : nullptr; }
  LnIO ln() const { return {stats.data_ptr<float>(), gamma.data_ptr<float>(), beta.data_ptr<float>(), pre_ptr()}; }
};

// n: the C2R ops' output length; keep: r2c_ln's kept modes (each ignored by the other kind)
WlnArgs wln_args(WlnOp op, const at::Tensor& X, const at::Tensor& x, int64_t dim, int64_t n, int64_t keep,
                 const at::Tensor& stats, const at::Tensor& g, const at::Tensor& b,
                 const std::optional<at::Tensor>& pre, int64_t out_mode = 1) {
  check_wln(op, X, x, dim, n, stats, g, b, pre, out_mode);
  WlnArgs a;
  a.x = vec_aligned(x.contiguous());
  if (op != WlnOp::R2cLn) a.X = vec_aligned(X.contiguous());
  a.stats = vec_aligned(stats.to(at::kFloat).contiguous());
  a.gamma = vec_aligned(g.to(at::kFloat).contiguous());
  a.beta = vec_aligned(b.to(at::kFloat).contiguous());
  a.pre = vec_aligned(f32_or_undef(pre));
  a.axis = a.x.dim() - 2;
  a.n = a.x.size(a.axis);
  a.C = a.x.size(-1);
  a.km = op == WlnOp::R2cLn ? r2c_ln_kept(a.x, keep) : a.X.size(a.axis);
  a.M = a.x.numel() / std::max<int64_t>(a.C, 1);
  a.O = a.M / std::max<int64_t>(a.n, 1);
  return a;
}

// The one launch of the two-pass kernels of afno_wfft.hip, and the only code that fills an AfnoWLaunch: the R2C when
// the pack has no spectrum, else the C2R, whose instance follows from the dtype and the extra outputs (pairs and
// part: SPLIT, with out or lo2 or neither; part alone: PART).
void launch_wln(const WlnArgs& a, double scale, void* out, uint16_t* lo2 = nullptr, uint16_t* pairs = nullptr,
                float* part = nullptr) {
  AfnoWLaunch p;
  p.x = a.x.data_ptr();
  p.stats = a.stats.data_ptr<float>();
  p.gamma = a.gamma.data_ptr<float>();
  p.beta = a.beta.data_ptr<float>();
  p.pre = a.pre_ptr();
  p.spec = a.X.defined() ? a.X.data_ptr() : nullptr;
  p.out = out;
  p.lo2 = lo2;
  p.pairs = pairs;
  p.part = part;
  p.O = static_cast<int>(a.O);
  p.L = static_cast<int>(a.n);
  p.C = static_cast<int>(a.C);
  p.KM = static_cast<int>(a.km);
  p.scale = static_cast<float>(scale);
  p.f32 = a.x.scalar_type() == at::kFloat ? 1 : 0;  // these kernels take one dtype for x, the spectrum and out
  (a.X.defined() ? launch_afno_w_c2r_ln : launch_afno_w_r2c_ln)(p, current_stream(a.x));
}

// ---- route
// MI_DFT_NO_AFNO_W=1 (A/B, read once): LayerNorm-fused AFNO W-transforms on the generic fixed
// Stockham kernels instead of afno_wfft.hip (same results)
bool afno_w_enabled() {
  static const bool on = tuning_env("MI_DFT_NO_AFNO_W") == nullptr;
  return on;
}

// Whether afno_wfft.hip runs a call whose dtypes one of its instances covers: the specialised shape, and O = the
// number of [L, C] planes
bool afno_w_takes(int64_t L, int64_t C, int64_t KM, int64_t O) {
  return afno_w_enabled() && L < (int64_t(1) << 31) && C < (int64_t(1) << 31) && KM < (int64_t(1) << 31) &&
         afno_w_supported(static_cast<int>(L), static_cast<int>(C), static_cast<int>(KM)) && O < (int64_t(1) << 31);
}

enum class WlnKernel {
  Wfft,      // the two-pass kernels of afno_wfft.hip
  Stockham,  // the fixed Stockham kernels' LayerNorm pass, if one is compiled for the pass: launch_fft_fixed (inside
             // run_pass) decides for the ops and describe_fft_fixed for afno_w_info, both on build_pass_desc's
             // descriptor; a pass they decline goes the Aten way.  wln_route offers it up to lds_limit() only, the
             // bound of run_pass's first line (a LayerNorm pass is never composed from shorter ones)
  Aten,      // ATen LayerNorm + the plain transform (counted by fallback_counts)
  None,      // the op raises
};
struct WlnRoute {
  WlnKernel kernel;
  const char* reason;  // None: why the op raises; Aten, and Stockham once declined: why no fused kernel ran
};

// Where a non-empty call of the family runs on the device.  The ops dispatch on it, afno_w_info prints it.
// in / out: as for wln_refusal.
WlnRoute wln_route(WlnOp op, int64_t L, int64_t C, int64_t KM, int64_t O, at::ScalarType in, at::ScalarType out) {
  if (const char* why = wln_refusal(op, C, in, out)) return {WlnKernel::None, why};
  const bool bf16 = in == at::kBFloat16 && out == at::kBFloat16, f32 = in == at::kFloat && out == at::kFloat;
  if ((bf16 || f32) && afno_w_takes(L, C, KM, O)) return {WlnKernel::Wfft, ""};
  // From here on c2r_ln_add_split and c2r_ln_add_part run c2r_ln_add and compute their extra outputs with ATen:
  // the rest is c2r_ln_add's route for them.  The Stockham LayerNorm pass covers bf16 in and out only.
  if (!bf16) return {WlnKernel::Aten, "no LayerNorm-fused fp32 kernel for this shape"};
  return {L >= 1 && L <= lds_limit() ? WlnKernel::Stockham : WlnKernel::Aten, "no LayerNorm-fused kernel for this shape"};
}

// An empty spectrum skips the hand kernels
WlnRoute c2r_ln_route(WlnOp op, const WlnArgs& a) {
  if (a.X.numel() == 0) return {WlnKernel::Aten, "empty spectrum"};
  return wln_route(op, a.n, a.C, a.km, a.O, a.X.scalar_type(), a.x.scalar_type());
}

// ---- r2c_ln
at::Tensor r2c_ln_cuda(const at::Tensor& x_, int64_t dim, double scale, int64_t keep, const at::Tensor& stats_,
                       const at::Tensor& g_, const at::Tensor& b_, const std::optional<at::Tensor>& pre_,
                       std::optional<at::ScalarType> out_dtype) {
  const c10::DeviceGuard guard(x_.device());
  const WlnArgs a = wln_args(WlnOp::R2cLn, at::Tensor(), x_, dim, 0, keep, stats_, g_, b_, pre_);
  const at::ScalarType idt = a.x.scalar_type(), odt = out_dtype.value_or(idt);
  to_dtype(idt);
  to_dtype(odt);
  at::Tensor out = r2c_ln_empty(a.x, a.km, odt);
  if (a.x.numel() == 0) return out.zero_();
  const WlnKernel k = wln_route(WlnOp::R2cLn, a.n, a.C, a.km, a.O, idt, odt).kernel;
  if (k == WlnKernel::Wfft) {
    launch_wln(a, scale, out.data_ptr());
    return checked(out, "r2c_ln");
  }
  if (k == WlnKernel::Stockham) {
    const LnIO ln = a.ln();
    const std::vector<int64_t> cur = a.x.sizes().vec(), nxt(out.sizes().begin(), out.sizes().end() - 1);
    if (run_pass(Kind::R2C, a.x, out, cur, nxt, static_cast<int>(a.axis), a.n, static_cast<int>(a.n), 0,
                 static_cast<int>(a.km), 0, static_cast<float>(scale), false, nullptr, nullptr, &ln))
      return checked(out, "r2c_ln");
  }
  // no specialised kernel for this shape: normalise with ATen, then the plain R2C
  fallback_note("r2c_ln", "no LayerNorm-fused W-transform for this shape/dtype: ATen LayerNorm + the plain R2C");
  at::Tensor h = ln_apply(a.x, a.stats, a.gamma, a.beta, a.pre, nullptr).to(idt);
  const std::vector<int64_t> dv{a.axis}, kv{a.km, 0};
  return r2c_cuda(h, dv, scale, kv, odt);
}

at::Tensor r2c_ln_cpu(const at::Tensor& x, int64_t dim, double scale, int64_t keep, const at::Tensor& stats,
                      const at::Tensor& g, const at::Tensor& b, const std::optional<at::Tensor>& pre,
                      std::optional<at::ScalarType> out_dtype) {
  check_wln(WlnOp::R2cLn, at::Tensor(), x, dim, 0, stats, g, b, pre);
  at::Tensor h = ln_apply(x, stats, g, b, pre.value_or(at::Tensor()), nullptr).to(x.scalar_type());
  const std::vector<int64_t> dv{x.dim() - 2}, kv{keep, 0};
  return r2c_cpu(h, dv, scale, kv, out_dtype);
}

at::Tensor r2c_ln_meta(const at::Tensor& x, int64_t, double, int64_t keep, const at::Tensor&, const at::Tensor&,
                       const at::Tensor&, const std::optional<at::Tensor>&, std::optional<at::ScalarType> out_dtype) {
  return r2c_ln_empty(x, r2c_ln_kept(x, keep), out_dtype);
}

// ---- c2r_ln_add
// On the device from checked arguments: the op itself, and what the split and part ops run outside the specialised
// shape (counted as c2r_ln_add's fallback when ATen computes it).
at::Tensor c2r_ln_add_device(const WlnArgs& a, double scale) {
  const WlnKernel k = c2r_ln_route(WlnOp::C2rLnAdd, a).kernel;
  if (k == WlnKernel::Wfft || k == WlnKernel::Stockham) {
    at::Tensor out = c2r_ln_add_empty(a.x);
    if (k == WlnKernel::Wfft) {
      launch_wln(a, scale, out.data_ptr());
      return checked(out, "c2r_ln_add");
    }
    const LnIO ln = a.ln();
    const std::vector<int64_t> cur(a.X.sizes().begin(), a.X.sizes().end() - 1), nxt = a.x.sizes().vec();
    if (run_pass(Kind::C2R, a.X, out, cur, nxt, static_cast<int>(a.axis), a.n, static_cast<int>(a.km), 0,
                 static_cast<int>(a.n), 0, static_cast<float>(scale), true, a.x.data_ptr(), nullptr, &ln))
      return checked(out, "c2r_ln_add");
  }
  fallback_note("c2r_ln_add", "no LayerNorm-fused W-transform for this shape/dtype: ATen LayerNorm + the plain C2R");
  at::Tensor xp;
  at::Tensor h = ln_apply(a.x, a.stats, a.gamma, a.beta, a.pre, &xp);
  const std::vector<int64_t> dv{a.axis}, nv{a.n}, kv{a.km, 0};
  const at::ScalarType dt = a.x.scalar_type();
  return c2r_add_cuda(a.X, dv, nv, scale, kv, xp.to(dt).contiguous(), h.to(dt).contiguous(), dt);
}

// With ATen from checked arguments: the CPU forms of the three C2R ops
at::Tensor c2r_ln_add_aten(const at::Tensor& X, int64_t n, double scale, const at::Tensor& x, const at::Tensor& stats,
                           const at::Tensor& g, const at::Tensor& b, const std::optional<at::Tensor>& pre) {
  const int64_t axis = x.dim() - 2;
  at::Tensor xp;
  at::Tensor h = ln_apply(x, stats, g, b, pre.value_or(at::Tensor()), &xp);
  const std::vector<int64_t> dv{axis}, nv{n}, kv{X.size(axis), 0};
  at::Tensor y = c2r_cpu(X, dv, nv, scale, kv, at::kFloat);
  return (y + xp + h).to(x.scalar_type()).contiguous();
}

at::Tensor c2r_ln_add_cuda(const at::Tensor& X, int64_t dim, int64_t n, double scale, const at::Tensor& x,
                           const at::Tensor& stats, const at::Tensor& g, const at::Tensor& b,
                           const std::optional<at::Tensor>& pre) {
  const c10::DeviceGuard guard(X.device());
  return c2r_ln_add_device(wln_args(WlnOp::C2rLnAdd, X, x, dim, n, 0, stats, g, b, pre), scale);
}

at::Tensor c2r_ln_add_cpu(const at::Tensor& X, int64_t dim, int64_t n, double scale, const at::Tensor& x,
                          const at::Tensor& stats, const at::Tensor& g, const at::Tensor& b,
                          const std::optional<at::Tensor>& pre) {
  check_wln(WlnOp::C2rLnAdd, X, x, dim, n, stats, g, b, pre);
  return c2r_ln_add_aten(X, n, scale, x, stats, g, b, pre);
}

at::Tensor c2r_ln_add_meta(const at::Tensor&, int64_t, int64_t, double, const at::Tensor& x, const at::Tensor&,
                           const at::Tensor&, const at::Tensor&, const std::optional<at::Tensor>&) {
  return c2r_ln_add_empty(x);
}

// ---- c2r_ln_add_split
// c2r_ln_add + the residual stream's bf16x3 split-pair rows and per-64-channel LayerNorm partials
// (mean, M2), all from the one C2R epilogue (afno_wfft.hip SPLIT instantiation): the fp32 block's
// fc1 then reads the pairs with LN2 folded in (linear3_ln) -- no LayerNorm / split pass.
// The pairs hold out - mean(x) per token (stats[:, 0], the input's LayerNorm mean): centred, the
// split keeps 2^-17 of the deviation rather than of |out|, and ln_stats_merge(part, eps, stats)
// gives fc1 the matching centred mean.
// Returns (out [..., W, C] fp32, pairs [tokens, 2C] bf16, part [tokens, C/64, 2] fp32).
std::tuple<at::Tensor, at::Tensor, at::Tensor> split_and_partials(const at::Tensor& y, const at::Tensor& stats) {
  const int64_t C = y.size(-1);
  at::Tensor rows = y.reshape({-1, C}).to(at::kFloat);
  const int64_t M = rows.size(0);
  at::Tensor z = rows - stats.reshape({-1, 2}).select(1, 0).to(at::kFloat).unsqueeze(1);
  at::Tensor hi = z.to(at::kBFloat16);
  at::Tensor lo = (z - hi.to(at::kFloat)).to(at::kBFloat16);
  at::Tensor pairs = at::cat({hi.reshape({M, C / 32, 32}), lo.reshape({M, C / 32, 32})}, -1).reshape({M, 2 * C}).contiguous();
  at::Tensor w = rows.reshape({M, C / 64, 64});
  at::Tensor mean = w.mean(2);
  at::Tensor m2 = (w - mean.unsqueeze(2)).pow(2).sum(2);
  return {y, pairs, at::stack({mean, m2}, 2).contiguous()};
}

// (out, pairs, part) of the ATen paths -> out_mode's first result: out (1), its lo2 term
// bf16(out - m - (hi + lo)) (2, m = stats[:, 0], the pairs' centring) or nothing (0)
std::tuple<at::Tensor, at::Tensor, at::Tensor> out_mode_result(std::tuple<at::Tensor, at::Tensor, at::Tensor> r,
                                                                const at::Tensor& stats, int64_t out_mode) {
  if (out_mode == 1) return r;
  at::Tensor& out = std::get<0>(r);
  if (out_mode == 0) {
    out = at::empty({0}, out.options());
    return r;
  }
  const int64_t C = out.size(-1);
  at::Tensor z = out.reshape({-1, C}).to(at::kFloat) - stats.to(at::kFloat).reshape({-1, 2}).select(1, 0).unsqueeze(1);
  at::Tensor pr = std::get<1>(r).to(at::kFloat).reshape({-1, C / 32, 2, 32});
  out = (z - (pr.select(2, 0) + pr.select(2, 1)).reshape({-1, C})).to(at::kBFloat16);
  return r;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> c2r_ln_add_split_cuda(const at::Tensor& X, int64_t dim, int64_t n, double scale,
                                                                     const at::Tensor& x, const at::Tensor& stats,
                                                                     const at::Tensor& g, const at::Tensor& b,
                                                                     const std::optional<at::Tensor>& pre, int64_t out_mode) {
  const c10::DeviceGuard guard(X.device());
  const WlnArgs a = wln_args(WlnOp::C2rLnAddSplit, X, x, dim, n, 0, stats, g, b, pre, out_mode);
  if (c2r_ln_route(WlnOp::C2rLnAddSplit, a).kernel == WlnKernel::Wfft) {
    auto [out, pairs, part] = c2r_ln_add_split_empty(a.x, out_mode);
    launch_wln(a, scale, out_mode == 1 ? out.data_ptr() : nullptr,
               out_mode == 2 ? reinterpret_cast<uint16_t*>(out.data_ptr()) : nullptr,
               reinterpret_cast<uint16_t*>(pairs.data_ptr()), part.data_ptr<float>());
    return {checked(out, "c2r_ln_add_split"), pairs, part};
  }
  fallback_note("c2r_ln_add_split", "no fused W-transform for this shape: c2r_ln_add + ATen split / statistics");
  return out_mode_result(split_and_partials(c2r_ln_add_device(a, scale), a.stats), a.stats, out_mode);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> c2r_ln_add_split_cpu(const at::Tensor& X, int64_t dim, int64_t n, double scale,
                                                                    const at::Tensor& x, const at::Tensor& stats,
                                                                    const at::Tensor& g, const at::Tensor& b,
                                                                    const std::optional<at::Tensor>& pre, int64_t out_mode) {
  check_wln(WlnOp::C2rLnAddSplit, X, x, dim, n, stats, g, b, pre, out_mode);
  return out_mode_result(split_and_partials(c2r_ln_add_aten(X, n, scale, x, stats, g, b, pre), stats), stats, out_mode);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> c2r_ln_add_split_meta(const at::Tensor&, int64_t, int64_t, double,
                                                                     const at::Tensor& x, const at::Tensor&, const at::Tensor&,
                                                                     const at::Tensor&, const std::optional<at::Tensor>&,
                                                                     int64_t out_mode) {
  return c2r_ln_add_split_empty(x, out_mode);
}

// ---- c2r_ln_add_part
// bf16 block: c2r_ln_add + the next LayerNorm's per-64-channel partials (mean, M2) of the STORED
// (bf16-rounded) output, from the one C2R epilogue (afno_wfft.hip PART instantiation); ln_stats_merge
// turns them into LN2's (mean, rstd) without an ln_stats pass over the residual stream.
// Returns (out [..., W, C] bf16, part [tokens, C/64, 2] fp32).
std::tuple<at::Tensor, at::Tensor> out_and_partials(const at::Tensor& y) {
  const int64_t C = y.size(-1);
  at::Tensor w = y.reshape({-1, C / 64, 64}).to(at::kFloat);
  at::Tensor mean = w.mean(2);
  at::Tensor m2 = (w - mean.unsqueeze(2)).pow(2).sum(2);
  return {y, at::stack({mean, m2}, 2).contiguous()};
}

std::tuple<at::Tensor, at::Tensor> c2r_ln_add_part_cuda(const at::Tensor& X, int64_t dim, int64_t n, double scale,
                                                        const at::Tensor& x, const at::Tensor& stats, const at::Tensor& g,
                                                        const at::Tensor& b, const std::optional<at::Tensor>& pre) {
  const c10::DeviceGuard guard(X.device());
  const WlnArgs a = wln_args(WlnOp::C2rLnAddPart, X, x, dim, n, 0, stats, g, b, pre);
  if (c2r_ln_route(WlnOp::C2rLnAddPart, a).kernel == WlnKernel::Wfft) {
    auto [out, part] = c2r_ln_add_part_empty(a.x);
    launch_wln(a, scale, out.data_ptr(), nullptr, nullptr, part.data_ptr<float>());
    return {checked(out, "c2r_ln_add_part"), part};
  }
  fallback_note("c2r_ln_add_part", "no fused W-transform for this shape: c2r_ln_add + ATen statistics");
  return out_and_partials(c2r_ln_add_device(a, scale));
}

std::tuple<at::Tensor, at::Tensor> c2r_ln_add_part_cpu(const at::Tensor& X, int64_t dim, int64_t n, double scale,
                                                       const at::Tensor& x, const at::Tensor& stats, const at::Tensor& g,
                                                       const at::Tensor& b, const std::optional<at::Tensor>& pre) {
  check_wln(WlnOp::C2rLnAddPart, X, x, dim, n, stats, g, b, pre);
  return out_and_partials(c2r_ln_add_aten(X, n, scale, x, stats, g, b, pre));
}

std::tuple<at::Tensor, at::Tensor> c2r_ln_add_part_meta(const at::Tensor&, int64_t, int64_t, double, const at::Tensor& x,
                                                        const at::Tensor&, const at::Tensor&, const at::Tensor&,
                                                        const std::optional<at::Tensor>&) {
  return c2r_ln_add_part_empty(x);
}

// ------------------------------------------------------------------ ONNX-contrib parity ops
void check_contrib_attrs(int64_t normalized, int64_t onesided, int64_t signal_ndim) {
  // dft_plugins.cpp:54-57 ("mimics limitations of ONNX Contrib ops").
  TORCH_CHECK(normalized == 0, "amd_dft.Rfft/Irfft: only normalized=0 is supported (got ", normalized, ")");
  TORCH_CHECK(onesided == 1, "amd_dft.Rfft/Irfft: only onesided=1 is supported (got ", onesided, ")");
  TORCH_CHECK(signal_ndim >= 1 && signal_ndim <= 3, "amd_dft.Rfft/Irfft: signal_ndim must be in [1, 3] (got ",
              signal_ndim, ")");
}

at::Tensor contrib_rfft(const at::Tensor& x, int64_t normalized, int64_t onesided, int64_t signal_ndim) {
  check_contrib_attrs(normalized, onesided, signal_ndim);
  TORCH_CHECK(x.dim() >= signal_ndim, "amd_dft.Rfft: input rank ", x.dim(), " < signal_ndim ", signal_ndim);
  TORCH_CHECK(x.dim() < 8, "amd_dft.Rfft: input rank must be < 8 (output adds a dim; dft_plugins.cpp:369)");
  std::vector<int64_t> dims;
  for (int64_t i = signal_ndim; i >= 1; --i) dims.push_back(x.dim() - i);
  static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("amd_dft::r2c", "").typed<decltype(r2c_cpu)>();
  return op.call(x, dims, 1.0, {}, std::nullopt);
}

at::Tensor contrib_irfft(const at::Tensor& x, int64_t normalized, int64_t onesided, int64_t signal_ndim) {
  check_contrib_attrs(normalized, onesided, signal_ndim);
  TORCH_CHECK(x.dim() >= signal_ndim + 1 && x.size(-1) == 2,
              "amd_dft.Irfft: input must be [..., signal dims, 2] with rank >= signal_ndim + 1");
  const int64_t nd = x.dim() - 1;
  std::vector<int64_t> dims, sizes;
  int64_t total = 1;
  for (int64_t i = signal_ndim; i >= 1; --i) {
    const int64_t ax = nd - i;
    dims.push_back(ax);
    const int64_t n = i == 1 ? 2 * (x.size(ax) - 1) : x.size(ax);  // dft_plugins.cpp:428-434
    TORCH_CHECK(n >= 1, "amd_dft.Irfft: last signal dim must be >= 2");
    sizes.push_back(n);
    total *= n;
  }
  static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("amd_dft::c2r", "").typed<decltype(c2r_cpu)>();
  // "backward" normalisation: 1/prod(n) on the inverse (dft_plugins.cpp:457-468), in double.
  return op.call(x, dims, sizes, 1.0 / static_cast<double>(total), {}, std::nullopt);
}

// ------------------------------------------------------------------ introspection
std::string plan_info(int64_t n) {
  TORCH_CHECK(n >= 1 && n < (1 << 30), "amd_dft.plan_info: bad length");
  Plan1D p = make_plan_1d(static_cast<int32_t>(n));
  std::ostringstream os;
  os << describe(p) << " lds_limit=" << max_lds_length();
  return os.str();
}

Kind parse_kind(const std::string& kind, const char* op) {
  if (kind == "r2c") return Kind::R2C;
  if (kind == "c2r") return Kind::C2R;
  TORCH_CHECK(kind == "c2c", "amd_dft.", op, ": kind must be r2c, c2r or c2c");
  return Kind::C2C;
}

// Which kernel one full (unpruned) transform pass along `axis` would launch, from the functions
// run_pass uses (make_plan_1d, apply_plan, set_axis_geometry, choose_tiling, the fixed kernels'
// selection), on the host alone: no device, no allocation, pointers taken as aligned.  `shape` is
// the pass input's logical shape (without the trailing re/im dim), `n` the transform length
// (default: shape[axis]; for c2r 2 * (shape[axis] - 1)).
std::string fft_pass_info(std::string kind_s, at::IntArrayRef shape, int64_t axis, int64_t n, bool bf16_in,
                          bool bf16_out) {
  const Kind kind = parse_kind(kind_s, "fft_pass_info");
  const int64_t nd = static_cast<int64_t>(shape.size());
  axis = axis < 0 ? axis + nd : axis;
  TORCH_CHECK(axis >= 0 && axis < nd, "amd_dft.fft_pass_info: axis out of range");
  for (int64_t v : shape) TORCH_CHECK(v >= 1, "amd_dft.fft_pass_info: empty shape");
  const int64_t stored = shape[axis];
  const int64_t L = n > 0 ? n : (kind == Kind::C2R ? 2 * (stored - 1) : stored);
  TORCH_CHECK(L >= 1 && L < (1 << 30), "amd_dft.fft_pass_info: bad length");
  if (L > lds_limit()) return "large L=" + std::to_string(L);
  const int64_t half = L / 2 + 1;
  TORCH_CHECK(kind == Kind::C2R || stored == L, "amd_dft.fft_pass_info: shape[axis] must be the transform length");
  std::vector<int64_t> in_shape(shape.begin(), shape.end()), out_shape = in_shape;
  out_shape[axis] = kind == Kind::R2C ? half : L;
  PassDesc d;
  TORCH_CHECK(build_pass_desc(d, kind, make_plan_1d(static_cast<int32_t>(L)), in_shape, out_shape, static_cast<int>(axis),
                              kind == Kind::C2R ? std::min(stored, half) : L, 0, kind == Kind::R2C ? half : L, 0,
                              kind == Kind::C2R, bf16_in ? DType::BF16 : DType::F32, bf16_out ? DType::BF16 : DType::F32),
              "amd_dft.fft_pass_info: length exceeds the LDS-resident limit");
  const int64_t nsig = kind == Kind::C2C ? d.I : (d.I + 1) / 2;
  std::ostringstream os;
  FixedLaunchInfo fi;
  if (describe_fft_fixed(d, fi)) {
    const FixedCfg& c = fixed_configs()[fi.cfg];
    os << "fixed L=" << c.L << " cols=" << (c.cols ? 1 : 0) << " TP=" << c.TP << " T=" << c.T << " cfg=" << fi.cfg
       << " tiles=" << fi.tiles_per_outer << " blocks=" << fi.nblocks << " xcd=" << (fi.xcd ? 1 : 0)
       << " pairvec=" << (fi.pairvec ? 1 : 0);
  } else {
    const bool cols = d.Si_in < d.Sn_in || d.Si_out < d.Sn_out;
    os << "generic L=" << d.L << " radices=[";
    for (int i = 0; i < d.npass; ++i) os << (i ? "," : "") << d.radix[i];
    os << "] cols=" << (cols ? 1 : 0) << " logT=" << d.logT << " nthreads=" << d.nthreads
       << " tiles=" << d.tiles_per_outer << " blocks=" << d.O * d.tiles_per_outer << " lds=" << pass_lds_bytes(d)
       << " vec_in=" << d.vec_in << " vec_out=" << d.vec_out;
  }
  os << " I=" << d.I << " O=" << d.O << " nsig=" << nsig;
  return os.str();
}

// Which route an aligned call of a LayerNorm-fused W-transform takes on the device (host only: no device, no
// allocation): wln_route's answer, the one the ops dispatch on, printed.
//   "wfft c2r_bf16_part slabs=3 stage=fp16"                  the two-pass kernels of afno_wfft.hip and the instance
//   "stockham L=180 TP=15 T=16 cfg=27 pairvec=1"              the fixed Stockham kernels' LayerNorm pass (bf16 only)
//   "aten <reason>"                                           ATen LayerNorm + the plain transform (counted by
//                                                             fallback_counts)
//   "none <reason>"                                           the op raises
// c2r_ln_add_split / c2r_ln_add_part outside the specialised shape compute their extra outputs with ATen on top of
// c2r_ln_add: "aten epilogue; c2r_ln_add: <its route>".
std::string afno_w_info(std::string op_s, int64_t L, int64_t C, int64_t KM, bool bf16) {
  const auto* found = std::find(std::begin(kWlnNames), std::end(kWlnNames), op_s);
  TORCH_CHECK(found != std::end(kWlnNames),
              "amd_dft.afno_w_info: op must be r2c_ln, c2r_ln_add, c2r_ln_add_split or c2r_ln_add_part");
  TORCH_CHECK(L >= 1 && L < (1 << 30) && C >= 1 && C < (1 << 30) && KM >= 1 && KM <= L / 2 + 1,
              "amd_dft.afno_w_info: needs L, C >= 1 and 1 <= KM <= L / 2 + 1");
  const WlnOp op = static_cast<WlnOp>(found - std::begin(kWlnNames));
  const bool r2c = op == WlnOp::R2cLn, split = op == WlnOp::C2rLnAddSplit, part = op == WlnOp::C2rLnAddPart;
  const at::ScalarType dt = bf16 ? at::kBFloat16 : at::kFloat;
  const WlnRoute r = wln_route(op, L, C, KM, 1, dt, dt);
  std::ostringstream os;
  if (r.kernel == WlnKernel::None) {
    os << "none " << r.reason;
    return os.str();
  }
  if (r.kernel == WlnKernel::Wfft) {
    os << "wfft " << afno_w_instance_name(afno_w_instance(!r2c, !bf16, split, split || part)) << " slabs=" << C / 64
       << " stage=" << (bf16 ? "fp16" : "fp32");
    return os.str();
  }
  if (split || part) os << "aten epilogue; c2r_ln_add: ";
  if (r.kernel == WlnKernel::Stockham) {  // the pass the ops hand to run_pass, on one [L, C] plane
    const std::vector<int64_t> in_shape{1, r2c ? L : KM, C}, out_shape{1, r2c ? KM : L, C};
    PassDesc d;
    FixedLaunchInfo fi;
    if (build_pass_desc(d, r2c ? Kind::R2C : Kind::C2R, make_plan_1d(static_cast<int32_t>(L)), in_shape, out_shape, 1,
                        r2c ? L : KM, 0, r2c ? KM : L, 0, !r2c, DType::BF16, DType::BF16)) {
      alignas(16) static const float probe[4] = {0.f, 0.f, 0.f, 0.f};  // non-null, aligned stand-ins: only tested, never read
      d.ln_stats = d.ln_gamma = d.ln_beta = probe;
      if (!r2c) d.add1 = probe;
      if (describe_fft_fixed(d, fi)) {
        const FixedCfg& c = fixed_configs()[fi.cfg];
        os << "stockham L=" << c.L << " TP=" << c.TP << " T=" << c.T << " cfg=" << fi.cfg << " pairvec=" << (fi.pairvec ? 1 : 0);
        return os.str();
      }
    }
  }
  os << "aten " << r.reason;
  return os.str();
}

// The compiled fixed configurations, one "L cols TP T r,r,..." entry per table index, ';'-separated.
std::string fft_fixed_configs() {
  std::ostringstream os;
  for (const FixedCfg& c : fixed_configs()) {
    os << c.L << ' ' << (c.cols ? 1 : 0) << ' ' << c.TP << ' ' << c.T << ' ';
    for (int i = 0; i < c.npass; ++i) os << (i ? "," : "") << c.radix[i];
    os << ';';
  }
  return os.str();
}

// Brute force over the selection score: how often each table index wins for I in 1..I_max, O in 1..O_max
// with the default radix order of L.
std::vector<int64_t> fft_fixed_sweep(std::string kind_s, int64_t L, bool cols, int64_t I_max, int64_t O_max) {
  const Kind kind = parse_kind(kind_s, "fft_fixed_sweep");
  TORCH_CHECK(L >= 1 && L < (1 << 30), "amd_dft.fft_fixed_sweep: bad length");
  const std::vector<int32_t> rad = factorize(static_cast<int32_t>(L));
  std::vector<int64_t> wins(fixed_configs().size(), 0);
  for (int64_t O = 1; O <= O_max; ++O)
    for (int64_t I = 1; I <= I_max; ++I) {
      const int b = select_fixed_config(kind, static_cast<int32_t>(L), cols, I, O, rad.data(), static_cast<int32_t>(rad.size()));
      if (b >= 0) ++wins[b];
    }
  return wins;
}

std::string plugin_registry() {
  // Mirrors the two TensorRT plugin creators (dft_plugins.cpp:497-570): name, version,
  // namespace, field list in the creator's order.
  return R"([{"name": "Rfft", "version": "1", "namespace": "", "domain": "com.microsoft", "op": "amd_dft::Rfft",)"
         R"( "fields": [{"name": "normalized", "type": "INT32", "default": 0},)"
         R"( {"name": "onesided", "type": "INT32", "default": 1},)"
         R"( {"name": "signal_ndim", "type": "INT32", "default": 1}]},)"
         R"( {"name": "Irfft", "version": "1", "namespace": "", "domain": "com.microsoft", "op": "amd_dft::Irfft",)"
         R"( "fields": [{"name": "normalized", "type": "INT32", "default": 0},)"
         R"( {"name": "onesided", "type": "INT32", "default": 1},)"
         R"( {"name": "signal_ndim", "type": "INT32", "default": 1}]}])";
}

int64_t plan_cache_size() { return static_cast<int64_t>(plan_cache_entries()); }
void plan_cache_clear() { plan_cache_reset(); }
int64_t plan_cache_pinned_count() { return static_cast<int64_t>(plan_cache_pinned()); }

}  // namespace
}  // namespace amd_dft

// The dispatched ops of this file, once: name and schema.  Each has name_cuda, name_cpu and name_meta above, so an op
// missing from one backend fails to compile.
#define AMD_DFT_DFT_OPS(X)                                                                                            \
  X(r2c, "(Tensor x, int[] dim, float scale=1.0, int[] keep=[], ScalarType? out_dtype=None) -> Tensor")               \
  X(c2r, "(Tensor x, int[] dim, int[] out_size, float scale=1.0, int[] keep=[], ScalarType? out_dtype=None) -> Tensor") \
  X(c2c, "(Tensor x, int[] dim, bool inverse=False, float scale=1.0, ScalarType? out_dtype=None) -> Tensor")          \
  X(c2r_add, "(Tensor x, int[] dim, int[] out_size, float scale=1.0, int[] keep=[], Tensor? add1=None, "              \
             "Tensor? add2=None, ScalarType? out_dtype=None) -> Tensor")                                              \
  X(c2c_axis, "(Tensor x, int dim, int n, int in_lo, int in_hi, int out_lo, int out_hi, bool inverse=False, "         \
              "float scale=1.0) -> Tensor")                                                                           \
  X(dftw_r2c, "(Tensor x, int m, float scale=1.0) -> Tensor")                                                         \
  X(fno_mix_c2c, "(Tensor xm, Tensor w, int n, int in_lo, int in_hi, float scale=1.0, int path=0) -> Tensor")         \
  X(r2c_ln, "(Tensor x, int dim, float scale, int keep, Tensor stats, Tensor gamma, Tensor beta, Tensor? pre=None, "  \
            "ScalarType? out_dtype=None) -> Tensor")                                                                  \
  X(c2r_ln_add, "(Tensor X, int dim, int n, float scale, Tensor x, Tensor stats, Tensor gamma, Tensor beta, "         \
                "Tensor? pre=None) -> Tensor")                                                                        \
  X(c2r_ln_add_split, "(Tensor X, int dim, int n, float scale, Tensor x, Tensor stats, Tensor gamma, Tensor beta, "   \
                      "Tensor? pre=None, int out_mode=1) -> (Tensor, Tensor, Tensor)")                                \
  X(c2r_ln_add_part, "(Tensor X, int dim, int n, float scale, Tensor x, Tensor stats, Tensor gamma, Tensor beta, "    \
                     "Tensor? pre=None) -> (Tensor, Tensor)")

TORCH_LIBRARY(amd_dft, m) {
  AMD_DFT_DFT_OPS(AMD_DFT_DEF)
  // composite: they call r2c / c2r through the dispatcher
  m.def("Rfft(Tensor x, int normalized=0, int onesided=1, int signal_ndim=1) -> Tensor");
  m.def("Irfft(Tensor x, int normalized=0, int onesided=1, int signal_ndim=1) -> Tensor");
  m.def("plan_info(int n) -> str", &amd_dft::plan_info);
  m.def("fft_pass_info(str kind, int[] shape, int axis, int n=-1, bool bf16_in=False, bool bf16_out=False) -> str",
        &amd_dft::fft_pass_info);
  m.def("afno_w_info(str op, int L, int C, int KM, bool bf16) -> str", &amd_dft::afno_w_info);
  m.def("fft_fixed_configs() -> str", &amd_dft::fft_fixed_configs);
  m.def("fft_fixed_sweep(str kind, int L, bool cols, int I_max, int O_max) -> int[]", &amd_dft::fft_fixed_sweep);
  m.def("plugin_registry() -> str", &amd_dft::plugin_registry);
  m.def("plan_cache_size() -> int", &amd_dft::plan_cache_size);
  m.def("plan_cache_clear() -> ()", &amd_dft::plan_cache_clear);
  m.def("plan_cache_pinned() -> int", &amd_dft::plan_cache_pinned_count);
}
TORCH_LIBRARY_IMPL(amd_dft, CUDA, m) { AMD_DFT_DFT_OPS(AMD_DFT_IMPL_CUDA) }
TORCH_LIBRARY_IMPL(amd_dft, CPU, m) { AMD_DFT_DFT_OPS(AMD_DFT_IMPL_CPU) }
TORCH_LIBRARY_IMPL(amd_dft, Meta, m) { AMD_DFT_DFT_OPS(AMD_DFT_IMPL_META) }
TORCH_LIBRARY_IMPL(amd_dft, CompositeImplicitAutograd, m) {
  m.impl("Rfft", &amd_dft::contrib_rfft);
  m.impl("Irfft", &amd_dft::contrib_irfft);
}

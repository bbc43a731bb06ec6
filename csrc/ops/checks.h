// Opt-in output validation for the device ops (the reference only
// asserts and always returns 0 from enqueue).  MI_DFT_CHECK_FINITE=1 makes every op verify
// that its output is finite and raise otherwise.  It synchronises the stream, so it is
// skipped while a hipGraph is being captured.
#pragma once

#include <ATen/ATen.h>
#include <c10/hip/HIPGraphsC10Utils.h>
#include <c10/hip/HIPStream.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>

namespace amd_dft {

// Both switches start from their environment variable and can be flipped at run time
// (torch.ops.amd_dft.set_finite_check / set_strict; utils.runtime.finite_checks / strict_mode).
inline bool env_flag(const char* name) {
  const char* e = std::getenv(name);
  return e && std::string(e) != "0";
}
inline std::atomic<bool>& finite_check_flag() {
  static std::atomic<bool> on{env_flag("MI_DFT_CHECK_FINITE")};
  return on;
}
inline std::atomic<bool>& strict_flag() {
  static std::atomic<bool> on{env_flag("MI_DFT_STRICT")};
  return on;
}
inline bool finite_check_enabled() { return finite_check_flag().load(std::memory_order_relaxed); }

inline const at::Tensor& checked(const at::Tensor& out, const char* op) {
  if (finite_check_enabled() && out.defined() && out.numel() > 0 &&
      c10::hip::currentStreamCaptureStatusMayInitCtx() == c10::hip::CaptureStatus::None) {
    const bool ok = at::isfinite(out).all().item<bool>();
    TORCH_CHECK(ok, "amd_dft.", op, ": output contains NaN/Inf (MI_DFT_CHECK_FINITE=1)");
  }
  return out;
}

// ---- visible fallbacks: every time a GPU op routes to ATen / a vendor
// library instead of its hand kernel it is counted per op, warned once per op, and raises
// when MI_DFT_STRICT=1 (tests and benches assert zero fallbacks on the hot paths).
struct FallbackRegistry {
  std::mutex mu;
  std::map<std::string, int64_t> counts;
  std::atomic<int64_t> total{0};
};
inline FallbackRegistry& fallback_registry() {
  static FallbackRegistry r;
  return r;
}
inline void fallback_note(const char* op, const char* why) {
  TORCH_CHECK(!strict_flag().load(std::memory_order_relaxed), "amd_dft.", op, ": no hand kernel for this call (", why, ") and MI_DFT_STRICT=1");
  auto& r = fallback_registry();
  bool first = false;
  {
    std::lock_guard<std::mutex> g(r.mu);
    first = r.counts[op]++ == 0;
  }
  r.total.fetch_add(1);
  if (first) TORCH_WARN("amd_dft.", op, ": falling back to ATen (", why, "); counted in amd_dft.fallback_counts()");
}

// ---- optional tensor arguments (a schema's "Tensor?"): None arrives as nullopt or as an undefined tensor
inline bool present(const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); }
// the tensor as contiguous fp32 (what the kernels read for bias, c1, stats and pre), undefined when absent
inline at::Tensor f32_or_undef(const c10::optional<at::Tensor>& t) {
  return present(t) ? t->to(at::kFloat).contiguous() : at::Tensor();
}

// ---- alignment of kernel inputs
// A kernel that loads `bytes` at a time reads tensors that start on that boundary (a pointer test; allocations do, a
// contiguous view at an odd element offset into a larger buffer does not): t itself, or its own contiguous copy.
inline at::Tensor aligned_to(const at::Tensor& t, uintptr_t bytes) {
  if (!t.defined() || t.numel() == 0 || reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0) return t;
  return t.clone(at::MemoryFormat::Contiguous);
}
// The LayerNorm-fused W-transforms (afno_wfft.hip) and the LayerNorm kernels (layernorm.hip) move 8 or 16 bytes
// per lane, and the former DMA 16-byte pieces of the residual tile and its statistics into LDS: every tensor they
// read starts on a 16-byte boundary.
inline at::Tensor vec_aligned(const at::Tensor& x) { return aligned_to(x, 16); }

// the stream the kernels of an op on t's device are launched on
inline hipStream_t current_stream(const at::Tensor& t) {
  return c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

// ---- padded extents of the MFMA kernels' operands
constexpr int64_t ceil16(int64_t v) { return (v + 15) / 16 * 16; }
constexpr int64_t ceil32(int64_t v) { return (v + 31) / 32 * 32; }

// AFNO block-MLP weights [NB, k, k], or their bf16x3 split [NB, k, 2k] (k32-interleaved (hi, lo) rows), as fp32
// [NB, k, k]
inline at::Tensor unsplit_k32(const at::Tensor& w, const char* op) {
  const int64_t k = w.size(1);
  if (w.size(2) == k) return w.to(at::kFloat);
  TORCH_CHECK(k % 32 == 0, op, ": split weights need 2 * block_size % 32 == 0");
  return w.to(at::kFloat).reshape({w.size(0), k, k / 32, 2, 32}).sum(3).reshape({w.size(0), k, k});
}

}  // namespace amd_dft

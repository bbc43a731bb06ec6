// Compile-time specialised Stockham configurations (host-visible table).
//
// For the hot transform lengths (FourCastNet / FNO grids and powers of two) the radix
// sequence, threads per FFT (TP) and FFTs per workgroup (T) are template parameters of
// fft_fixed_kernel (fft_fixed.hip): every loop is unrolled, strides along the transform are
// constants, the first pass reads global memory straight into registers and the last pass
// writes global memory straight from registers (C2C / C2R), so only NPASS-1 LDS round
// trips remain.  The generic runtime-radix kernel (fft_kernels.hip) covers everything else.
#pragma once

#include <cstdint>
#include <vector>

#include "fft_desc.h"

namespace amd_dft {

struct FixedCfg {
  int32_t L;
  bool cols;      // true: signals interleaved along the fast global dim (lane = signal)
  int32_t TP;     // threads per FFT
  int32_t T;      // FFTs per workgroup
  int32_t npass;
  int32_t radix[4];
};

// All compiled configurations (order = preference for the same (L, cols)).
const std::vector<FixedCfg>& fixed_configs();
// Radix order used for L by the fixed kernels (empty if L has no fixed config).
std::vector<int32_t> fixed_radices(int32_t L);
// The selection score: index in fixed_configs() of the configuration that a pass of this kind
// and length over I inner signals and O outer indices runs (cols: column-like layout; radix: the
// plan's radix order), or -1 when no configuration applies.
int select_fixed_config(Kind kind, int32_t L, bool cols, int64_t I, int64_t O, const int32_t* radix, int32_t npass);
// Launch the best fixed configuration for d; returns false when none applies.
bool launch_fft_fixed(const PassDesc& d, void* stream);
// What launch_fft_fixed(d) would launch, without touching a device; false when it would launch
// nothing (the generic kernel runs).
struct FixedLaunchInfo {
  int cfg = -1;  // index in fixed_configs()
  int64_t nblocks = 0;
  int32_t tiles_per_outer = 0;
  bool xcd = false;      // XCD-aware tile order
  bool pairvec = false;  // paired-vector IO variant
};
bool describe_fft_fixed(const PassDesc& d, FixedLaunchInfo& info);


}  // namespace amd_dft

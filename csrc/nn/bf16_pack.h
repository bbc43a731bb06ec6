// fp32 -> packed bf16 pairs for the MFMA kernels: the rounding every bf16 store uses, and the bf16x3 split
// (v = hi + lo up to 2^-17 relative) every fp32 operand is staged with.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace amd_dft {

// two floats -> packed bf16x2 (v_cvt_pk_bf16_f32, round-to-nearest-even)
__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  bf16x2 v;
  v[0] = static_cast<__bf16>(a);
  v[1] = static_cast<__bf16>(b);
  return __builtin_bit_cast(uint32_t, v);
}
// hi = bf16(a, b); lo = bf16(a - hi.a, b - hi.b)
__device__ __forceinline__ void split_pk(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = pk_bf16(a, b);
  lo = pk_bf16(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}

}  // namespace amd_dft

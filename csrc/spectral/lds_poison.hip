// Test support: fill every CU's LDS with NaNs (lds_poison) and read back what a later kernel finds there
// (lds_probe).  The MFMA spectral kernels write zeros into the ragged edges of their LDS images because
// 0 * stale-NaN is NaN; LDS normally holds small finite leftovers, so a forgotten zero-fill computes 0 * finite = 0
// and passes every test.  After lds_poison it does not (tests/test_kernel_bounds_gpu.py).
//
// Both kernels take the largest dynamic LDS the device reports for a workgroup (160 KiB on gfx950, a whole CU's LDS:
// lds_poison_info() gives the figure and the test asserts it), so one workgroup owns a CU's LDS while it
// runs, and launch kLdsPoisonRounds workgroups per CU.  The poison kernel stores the word 0x7fc07fc0 -- a quiet NaN
// as fp32 and as two bf16 -- over all of it, several passes, so the workgroups outlast the dispatch ramp and every
// CU takes its share; it writes nothing to global memory.  The probe kernel reads its LDS without writing it and
// stores, per thread, how many words held the pattern; that only means something while no kernel ran in between
// and the runtime does not clear LDS between kernels, which is what the probe is there to measure.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "spectral.h"

namespace amd_dft {
namespace {

constexpr int kThreads = 256;
constexpr int kPoisonPasses = 8;

__global__ void __launch_bounds__(kThreads) lds_poison_kernel(int words) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_words[];
  volatile uint32_t* lds = lds_words;  // volatile: the stores are issued although nothing here reads them
  for (int pass = 0; pass < kPoisonPasses; ++pass)
    for (int i = threadIdx.x; i < words; i += kThreads) lds[i] = kLdsPoisonWord;
}

__global__ void __launch_bounds__(kThreads) lds_probe_kernel(int words, int32_t* __restrict__ hits) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_words[];
  const volatile uint32_t* lds = lds_words;  // volatile: loads of memory this kernel never wrote are still issued
  int32_t n = 0;
  for (int i = threadIdx.x; i < words; i += kThreads) n += lds[i] == kLdsPoisonWord ? 1 : 0;
  hits[static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x] = n;
}

void check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("amd_dft: lds_poison: ") + what + ": " + hipGetErrorString(e));
}

}  // namespace

LdsPoisonGeo lds_poison_geometry() {
  int dev = 0, cus = 0, bytes = 0;
  check(hipGetDevice(&dev), "hipGetDevice");
  check(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev), "CU count");
  check(hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev), "LDS per workgroup");
  if (cus <= 0 || bytes < 4) throw std::runtime_error("amd_dft: lds_poison: the device reports no LDS");
  LdsPoisonGeo g;
  g.wgs = static_cast<int64_t>(cus) * kLdsPoisonRounds;
  g.threads = kThreads;
  g.words = bytes / 4;
  return g;
}

void launch_lds_poison(void* stream) {
  const LdsPoisonGeo g = lds_poison_geometry();
  const size_t bytes = static_cast<size_t>(g.words) * 4;
  check(hipFuncSetAttribute(reinterpret_cast<const void*>(&lds_poison_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)),
        "dynamic LDS limit");
  hipLaunchKernelGGL(lds_poison_kernel, dim3(static_cast<uint32_t>(g.wgs)), dim3(kThreads), bytes,
                     static_cast<hipStream_t>(stream), static_cast<int>(g.words));
  check(hipGetLastError(), "launch");
}

void launch_lds_probe(int32_t* hits, void* stream) {
  const LdsPoisonGeo g = lds_poison_geometry();
  const size_t bytes = static_cast<size_t>(g.words) * 4;
  check(hipFuncSetAttribute(reinterpret_cast<const void*>(&lds_probe_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)),
        "dynamic LDS limit");
  hipLaunchKernelGGL(lds_probe_kernel, dim3(static_cast<uint32_t>(g.wgs)), dim3(kThreads), bytes,
                     static_cast<hipStream_t>(stream), static_cast<int>(g.words), hits);
  check(hipGetLastError(), "launch");
}

}  // namespace amd_dft

// Internal (non-ABI) launcher of peaks.hip, called from abi_common.cpp. The public C ABI is include/m3s.h.
#pragma once
#include <hip/hip_runtime.h>

extern "C" hipError_t m3s_launch_peak_fma_f32(float* out, int blocks, int iters, hipStream_t s);

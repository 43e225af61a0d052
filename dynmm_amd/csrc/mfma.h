// The fp32 accumulator vectors and the two fp32 MFMA shapes the kernels of libdynmm_hip.so are built on.
#pragma once
#include <hip/hip_runtime.h>

namespace dynmm {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// v_mfma_f32_16x16x4_f32 and v_mfma_f32_32x32x2_f32: c += a . b, one A and one B value per lane.
__device__ __forceinline__ f32x4 mfma_16x16x4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_32x32x2(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

}  // namespace dynmm

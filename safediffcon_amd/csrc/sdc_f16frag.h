// The fp16 operand fragment of the fp16-operand kernels (*_f16.hip): eight halves, one lane's K fragment of v_mfma_f32_32x32x16_f16,
// and its formation from the registers of a 32x32 fp32 accumulator.  One definition for every translation unit.
#pragma once
#include "sdc_common.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// registers r0 .. r0 + 7 of an accumulator, scaled and rounded to nearest even: one K fragment of the next product
__device__ __forceinline__ half8 frag(const f32x16& acc, int r0, float scale = 1.0f) {
    half8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = (_Float16)(acc[r0 + j] * scale);
    return h;
}

}  // namespace

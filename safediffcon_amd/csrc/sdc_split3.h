// The exact three-way bf16 split of the bf16-split kernels: one definition for every translation unit.
#pragma once
#include "sdc_common.h"

namespace {

// x = h + m + l exactly (finite x): hardware RNE conversions, exact fp32 residuals
__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
#pragma clang fp contract(off)
    h = (__bf16)x;
    const float r = x - (float)h;
    m = (__bf16)r;
    l = (__bf16)(r - (float)m);
}

}  // namespace

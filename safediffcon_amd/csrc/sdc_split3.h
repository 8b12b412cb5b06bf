// The vocabulary of the bf16-split kernels, one definition for every translation unit: the exact three-way
// split, its 8-wide form on operand fragments, and the order of a product's six terms.
#pragma once
#include "sdc_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// x = h + m + l exactly (finite x): hardware RNE conversions, exact fp32 residuals
__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
#pragma clang fp contract(off)
    h = (__bf16)x;
    const float r = x - (float)h;
    m = (__bf16)r;
    l = (__bf16)(r - (float)m);
}

// v[0 .. 7] -> the three pieces of one K fragment
__device__ __forceinline__ void split3x8(const float* v, bf16x8& h, bf16x8& m, bf16x8& l) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        __bf16 ph, pm, pl;
        split3(v[i], ph, pm, pl);
        h[i] = ph; m[i] = pm; l[i] = pl;
    }
}

// a b ~= a3 b1 + a2 b2 + a1 b3 + a2 b1 + a1 b2 + a1 b1 (pieces numbered from 0 here): term t multiplies piece X3_PA[t] of a with piece
// X3_PB[t] of b.  Smallest terms first, so that the small terms meet in the accumulator before the main term's magnitude sets its ulp;
// the three dropped terms are below 2^-24 |a b|.
constexpr int X3_PA[6] = {2, 1, 0, 1, 0, 0}, X3_PB[6] = {0, 1, 2, 0, 1, 0};

}  // namespace

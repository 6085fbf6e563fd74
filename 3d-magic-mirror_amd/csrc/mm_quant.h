// mm_quant.h -- the 8-bit quantiser of the exports (mm_export.hip) and of the composite (mm_composite.hip): one definition, so a frame
// is the same bytes whichever kernel wrote it.  include/mm_render.h (Export) has the arithmetic.
#pragma once
#include "mm_device.h"

namespace mm {

__device__ inline unsigned quant(float x, int nearest) {
    MM_FP_EXACT
    float q = x * 255.0f;
    if (nearest) q = q + 0.5f;
    q = fminf(fmaxf(q, 0.0f), 255.0f);                        // fmaxf returns the operand that is not NaN: NaN -> 0
    return (unsigned)q;                                       // toward zero
}

// what to_tensor of the saved byte gives
__device__ inline float unquant(unsigned q) { MM_FP_EXACT return (float)q / 255.0f; }

}  // namespace mm

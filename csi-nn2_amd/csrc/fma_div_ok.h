// fma_div_ok.h -- the host's side of div_by_scale (common.h): the one check of the range in which it equals the division.
// No HIP header: reduce_canon.h and matmul_canon.h, which stand-alone programs compile, include it too.
#pragma once

namespace shl {

// div_by_scale(x, so, RN(1 / so)) == x / so when 2^-40 <= so <= 2^40 and no dividend exceeds `bound` <= 2^60 (the range
// conv_plan.hip:fma_division_ok admits).  Every caller states its own bound; a NaN in either argument gives false
static inline bool fma_div_ok(double bound, float so)
{
    return so >= 0x1p-40f && so <= 0x1p40f && bound <= 0x1p60;
}

}  // namespace shl

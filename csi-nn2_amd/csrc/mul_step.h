// mul_step.h -- the element function of CSINN_OP_MUL (source/reference/mul.c:21-40 inside shl_ref_diso_callback_base), for the
// two places that compute it: the broadcasting product's kernels (eltwise.hip) and the scale step of the fused attention kernel
// (attention.hip).  One definition, so that the fused launch equals the product's own launch by construction.  R: any record
// with the members of MulRec (eltwise.hip's MulArgs carries them next to its geometry).
#pragma once
#include <math.h>

#include "common.h"
#include "fma_div_ok.h"

namespace shl {

struct MulRec {
    float sa, za, sb, zb, so, zo, inv_so;
    int32_t fma_div;   // div_by_scale is exact for every product these records can give
    int32_t a_second;  // a is the reference's SECOND input: whose NaN goes through
};

// div_by_scale(p, so, RN(1 / so)) == p / so for every product the records can give (common.h; the range
// conv_plan.hip:fma_division_ok admits: 2^-40 <= so <= 2^40, |p| <= 2^60, p finite)
static inline bool mul_fma_ok(float a_scale, int32_t a_zp, float b_scale, int32_t b_zp, float out_scale)
{
    const double bound = (128.0 + fabs((double)a_zp)) * fabs((double)a_scale) * (128.0 + fabs((double)b_zp)) * fabs((double)b_scale);
    return fma_div_ok(bound, out_scale);
}

template <typename R>
__device__ __forceinline__ int mul_i8_one(int qa, int qb, const R &m)
{
    const float x = __fmul_rn(__fsub_rn((float)qa, m.za), m.sa);  // int8_to_float_base (source/nn2/utils.c:499-502)
    const float y = __fmul_rn(__fsub_rn((float)qb, m.zb), m.sb);
    const float p = __fmul_rn(x, y);
    const float d = m.fma_div ? div_by_scale(p, m.so, m.inv_so) : __fdiv_rn(p, m.so);
    return sat8_from_float(__fadd_rn(rintf(d), m.zo));  // float_to_int8_base (:550-560)
}

// the product of two binary16 values as the reference's x86 build gives it.  Only NaNs need care: float32_to_float16_base
// keeps a NaN's sign; the reference multiplies input1's element by input0's (mul.c:23 as compiled), so of two NaN operands
// input1's goes through, with its own sign; inf * 0 makes the default NaN, whose sign bit is set on x86
template <typename R>
__device__ __forceinline__ uint16_t mul_f16_one(uint16_t ha, uint16_t hb, const R &m)
{
    const uint16_t h1 = m.a_second ? ha : hb, h0 = m.a_second ? hb : ha;  // the reference's input1, input0
    if ((h1 & 0x7FFFu) > 0x7C00u) return (uint16_t)(0x7FFFu | (h1 & 0x8000u));
    if ((h0 & 0x7FFFu) > 0x7C00u) return (uint16_t)(0x7FFFu | (h0 & 0x8000u));
    const float p = __fmul_rn(f16_bits_to_float(ha), f16_bits_to_float(hb));
    if (p != p) return (uint16_t)0xFFFFu;
    return float_to_f16_bits_ref(p);
}

}  // namespace shl

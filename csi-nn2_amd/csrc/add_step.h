// add_step.h -- the element function of CSINN_OP_ADD (source/reference/add.c:21-24 inside shl_ref_diso_callback_base), for the
// two places that compute it: the broadcasting add's kernels (eltwise.hip) and the store of a matmul with a fused bias
// (matmul.hip).  One definition, so that the fused launch equals matmul followed by add by construction.
#pragma once
#include <math.h>

#include "common.h"

namespace shl {

// the records of an int8 sum: a and b dequantised, the sum requantised
struct AddRec {
    float sa, za, sb, zb, so, zo, inv_so;
    int32_t fma_div;  // div_by_scale is exact for every sum these records can give
};

// div_by_scale(r, so, RN(1 / so)) == r / so for every sum the records can give (common.h; the range
// conv_plan.hip:fma_division_ok admits: 2^-40 <= so <= 2^40, |r| <= 2^60, r finite)
static inline AddRec add_rec(float a_scale, int32_t a_zp, float b_scale, int32_t b_zp, float out_scale, int32_t out_zp)
{
    AddRec r;
    r.sa = a_scale, r.za = (float)a_zp, r.sb = b_scale, r.zb = (float)b_zp;
    r.so = out_scale, r.zo = (float)out_zp, r.inv_so = 1.0f / out_scale;
    const double bound = (128.0 + fabs((double)a_zp)) * fabs((double)a_scale) + (128.0 + fabs((double)b_zp)) * fabs((double)b_scale);
    r.fma_div = fma_div_ok(bound, out_scale);
    return r;
}

// x = ((float)qa - za) sa, y = ((float)qb - zb) sb (int8_to_float_base, source/nn2/utils.c:499-502), ONE fp32 sum, nothing
// contracted, sat8(rint(r / so) + zo) (float_to_int8_base, :550-560)
__device__ __forceinline__ int add_i8_step(int qa, int qb, const AddRec &m)
{
    const float x = __fmul_rn(__fsub_rn((float)qa, m.za), m.sa);
    const float y = __fmul_rn(__fsub_rn((float)qb, m.zb), m.sb);
    const float r = __fadd_rn(x, y);
    const float d = m.fma_div ? div_by_scale(r, m.so, m.inv_so) : __fdiv_rn(r, m.so);
    return sat8_from_float(__fadd_rn(rintf(d), m.zo));
}

// the sum of two binary16 values as the reference's x86 build gives it; h0 / h1: the layer's first / second input.  Only NaNs
// need care: float32_to_float16_base keeps a NaN's sign; the reference adds input0's element to input1's (add.c:23 as
// compiled, like mul.c:23), so of two NaN operands input1's goes through, with its own sign; inf + -inf makes the default NaN,
// whose sign bit is set on x86 (this device would clear it).  The genuine library's outputs on every pair of NaNs and
// infinities decide (tests/golden/add_bcast_cases.npz)
__device__ __forceinline__ uint16_t add_f16_step(uint16_t h0, uint16_t h1)
{
    if ((h1 & 0x7FFFu) > 0x7C00u) return (uint16_t)(0x7FFFu | (h1 & 0x8000u));
    if ((h0 & 0x7FFFu) > 0x7C00u) return (uint16_t)(0x7FFFu | (h0 & 0x8000u));
    const float r = __fadd_rn(f16_bits_to_float(h0), f16_bits_to_float(h1));
    if (r != r) return (uint16_t)0xFFFFu;
    return float_to_f16_bits_ref(r);
}

// The sum of two binary16 values as the SAME-SHAPE add gives it (shl_mi355x_add; a session runs it for a residual add,
// source/mi355x_opt/pooling.c:shl_mi355x_add_exec); h0 / h1: the layer's first / second input.  This is NOT add_f16_step: here
// the hardware's addition picks the NaN (of two NaN operands the one its operand order prefers, an inf + -inf its default one)
// and float_to_f16_bits_ref keeps that NaN's sign, where the broadcasting add follows the x86 reference's NaN rule.  For the two
// places that compute it: the stand-alone kernel (elementwise.hip) and the store of a binary16 convolution with a fused
// residual tail (residual_step.h), which must reproduce the stand-alone layer, not the broadcasting one.
__device__ __forceinline__ uint16_t add_same_f16_step(uint16_t h0, uint16_t h1)
{
    return float_to_f16_bits_ref(__fadd_rn(f16_bits_to_float(h0), f16_bits_to_float(h1)));
}

}  // namespace shl

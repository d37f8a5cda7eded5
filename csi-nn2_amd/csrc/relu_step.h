// relu_step.h -- the element function of CSINN_OP_RELU / CSINN_OP_RELU6 on int8 (shl_ref_relu_quant / shl_ref_relu6_quant,
// source/reference/relu.c:21-43, relu6.c:21-43), for the two places that compute it: the stand-alone kernel (elementwise.hip)
// and the store of a convolution with a fused residual tail (residual_step.h).  One definition, so that the fused launch
// equals the layers by construction.
#pragma once
#include "common.h"

namespace shl {

// the records of an int8 activation layer: its input dequantised, the clamped value requantised
struct ReluRec {
    float si, zi, so, zo;
    int32_t relu6;  // clamp at 6 too
};

static inline ReluRec relu_rec(float in_scale, int32_t in_zp, float out_scale, int32_t out_zp, int32_t relu6)
{
    ReluRec r;
    r.si = in_scale, r.zi = (float)in_zp, r.so = out_scale, r.zo = (float)out_zp, r.relu6 = relu6 ? 1 : 0;
    return r;
}

// x = ((float)q - zi) si (int8_to_float_base, source/nn2/utils.c:499-502), clamped at 0 and, for relu6, at 6,
// sat8(rint(x / so) + zo) (float_to_int8_base, :550-560): the hardware's division, nothing contracted
__device__ __forceinline__ int relu_i8_step(int q, float si, float zi, float so, float zo, int relu6)
{
    float x = __fmul_rn(__fsub_rn((float)q, zi), si);
    x = x > 0.0f ? x : 0.0f;
    if (relu6) x = fminf(x, 6.0f);
    return sat8_from_float(__fadd_rn(rintf(__fdiv_rn(x, so)), zo));
}

__device__ __forceinline__ int relu_i8_step(int q, const ReluRec &m) { return relu_i8_step(q, m.si, m.zi, m.so, m.zo, m.relu6); }

// binary16 (source/reference/relu.c:21-35, relu6.c:21-36 inside shl_ref_siso_callback_base): f16 -> f32 (exact), x > 0 ? x : 0
// (a NaN becomes 0), fmin(., 6) for relu6, f32 -> f16 with the reference's rounding.  For the stand-alone kernel
// (elementwise.hip) and the store of a binary16 convolution with a fused residual tail (residual_step.h)
__device__ __forceinline__ uint16_t relu_f16_step(uint16_t h, int relu6)
{
    float x = f16_bits_to_float(h);
    x = x > 0.0f ? x : 0.0f;
    if (relu6) x = fminf(x, 6.0f);
    return float_to_f16_bits_ref(x);
}

}  // namespace shl

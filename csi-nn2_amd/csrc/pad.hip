// pad.hip -- constant pad of a 4-d int8 / binary16 tensor (CSINN_OP_PAD): TensorFlow's asymmetric SAME padding in front of a
// stride-2 convolution, explicit pads of ONNX graphs.
//
// Restates shl_ref_pad_f32 behind shl_ref_siso_callback_base (source/reference/pad.c:21-140): the input is converted to
// float32, the float32 output is walked in memory order -- an element whose coordinate along any dim k lies in front of
// before[k] or behind before[k] + dim[k] receives pad_value, every other the next input element -- and the result is
// converted with the output's record.  NCHW and NHWC run the same loop nest with the dims named differently, so there is
// one routine over (dim, before, after)[4] in memory order.  Interior elements travel as requant_move.h says:
//   int8      q_out = sat8(rint(((q - zp_in) * s_in) / s_out) + zp_out); a byte copy when the records are equal and the
//             round trip was checked to be the identity on all 256 values
//   binary16  float32_to_float16_base(float16_to_float32_base(h))
// The pad element is computed ONCE on the host, as the reference's conversion of the float32 pad_value with the output's
// record (pad_element() below): int8 sat8(nearbyint(v / s_out) + zp_out), binary16 float32_to_float16_base(v).
//
// Arguments travel by value, calls enqueue only.  Two forms, chosen by pad_form() below, which also names them:
//   vec       16 bytes per thread in output order.  With j the innermost padded dim (0 when none is) and U the bytes of one
//             step along it, before[j] U, dim[j] U and after[j] U are multiples of 16 and both pointers 16-byte aligned: a
//             piece then is all pad or all interior, and an interior piece's source is aligned.  The dims behind j are
//             merged into it; the kernel sees at most four dims, the innermost in pieces.
//   generic   one output element per thread, any pads and alignment: the literal formula.
#include <stdlib.h>
#include <string.h>

#include "requant_move.h"

namespace shl {

enum { PAD_VEC = 0, PAD_GENERIC = 1 };

struct PadArgs {
    const void *in;
    void *out;
    int64_t oe[4], ie[4], bf[4];  // output extents, input extents, leading pads; the innermost in the form's unit
    int64_t items;
    uint32_t pad;  // the pad element, replicated over the dword
    MoveRec rec;
    int32_t small;  // the output has fewer than 2^32 elements: every index fits 32 bits
};

// the source unit of output unit i, or -1 where the output holds padding
__device__ __forceinline__ int64_t pad_source(int64_t i, const PadArgs &a)
{
    int64_t c3, c2, c1;
    int64_t rem = move_divmod(i, a.oe[3], a.small != 0, c3);
    rem = move_divmod(rem, a.oe[2], a.small != 0, c2);
    const int64_t c0 = move_divmod(rem, a.oe[1], a.small != 0, c1);
    const int64_t s0 = c0 - a.bf[0], s1 = c1 - a.bf[1], s2 = c2 - a.bf[2], s3 = c3 - a.bf[3];
    // (unsigned compares: a coordinate in front of the pad is negative)
    const bool inside = (uint64_t)s0 < (uint64_t)a.ie[0] && (uint64_t)s1 < (uint64_t)a.ie[1] && (uint64_t)s2 < (uint64_t)a.ie[2] &&
                        (uint64_t)s3 < (uint64_t)a.ie[3];
    return inside ? ((s0 * a.ie[1] + s1) * a.ie[2] + s2) * a.ie[3] + s3 : -1;
}

template <bool F16>
__global__ __launch_bounds__(256) void pad_vec_kernel(PadArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // piece of 16 bytes of the output
    if (i >= a.items) return;
    const int64_t src = pad_source(i, a);
    uint4 v = make_uint4(a.pad, a.pad, a.pad, a.pad);
    if (src >= 0) v = move_piece<uint4, F16>(static_cast<const uint4 *>(a.in)[src], a.rec);
    static_cast<uint4 *>(a.out)[i] = v;
}

template <bool F16>
__global__ __launch_bounds__(256) void pad_generic_kernel(PadArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // output element
    if (i >= a.items) return;
    const int64_t src = pad_source(i, a);
    if constexpr (F16) {
        static_cast<uint16_t *>(a.out)[i] =
            src >= 0 ? float_to_f16_bits_ref(f16_bits_to_float(static_cast<const uint16_t *>(a.in)[src])) : (uint16_t)a.pad;
    } else {
        static_cast<int8_t *>(a.out)[i] = src >= 0 ? (int8_t)move_rq<false>(static_cast<const int8_t *>(a.in)[src], a.rec) : (int8_t)a.pad;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------
// float32_to_float16_base (source/nn2/utils.c:576-620) on the host: common.h's float_to_f16_bits_literal, restated
static uint16_t host_f16_bits(float x)
{
    if (x > 65519.0f) return 0x7BFFu;
    if (x < -65519.0f) return 0xFBFFu;
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint32_t sign = u & 0x80000000u;
    u ^= sign;
    uint32_t h;
    if (u >= 0x7F800000u) {
        h = (u > 0x7F800000u) ? 0x7FFFu : 0x7C00u;
    } else {
        u &= 0xFFFFF000u;
        float f, scale;
        const uint32_t sbits = 15u << 23;  // 2^-112
        memcpy(&f, &u, 4), memcpy(&scale, &sbits, 4);
        volatile float s = f * scale;  // (fp32 subnormal results must survive)
        const float sv = s;
        memcpy(&u, &sv, 4);
        u += 0x1000u;
        if (u > (31u << 23)) u = 31u << 23;
        h = u >> 13;
    }
    return (uint16_t)(h | (sign >> 16));
}

// the pad element, in the low byte / half: the reference's conversion of the float32 pad_value with the output's record
static uint32_t pad_element(const shl_mi355x_pad_desc *d)
{
    if (d->dtype == SHL_MI355X_F16) return host_f16_bits(d->pad_value);
    // float_to_int8_base (source/nn2/utils.c:550-560): float ret = nearbyint(v / s) + zp -- the division in float, the
    // rounding and the sum in double, the result narrowed to float --, saturated, truncated
    const float q = d->pad_value / d->out_scale;
    const float ret = (float)(nearbyint((double)q) + (double)d->out_zp);
    int r;
    if (ret > 127.0f) r = 127;
    else if (ret < -128.0f) r = -128;
    else if (ret == ret) r = (int)ret;
    else r = 0;  // (NaN: the reference's conversion of it to int8 is undefined)
    return (uint32_t)r & 0xFFu;
}

// NULL when the arguments describe a pad, else what is wrong with them; *in_elems, *out_elems
static const char *pad_invalid(const void *in_dev, const void *out_dev, const shl_mi355x_pad_desc *d, int64_t *in_elems,
                               int64_t *out_elems)
{
    if (!d || !in_dev || !out_dev) return "NULL argument";
    if (d->dtype != SHL_MI355X_I8 && d->dtype != SHL_MI355X_F16) return "dtype is neither int8 nor binary16";
    int64_t ni = 1, no = 1;
    for (int k = 0; k < 4; ++k) {
        if (d->dim[k] < 0) return "a negative dim";
        if (d->before[k] < 0 || d->after[k] < 0) return "a negative pad";
        const int64_t o = (int64_t)d->dim[k] + d->before[k] + d->after[k];
        if (__builtin_mul_overflow(ni, (int64_t)d->dim[k], &ni) || __builtin_mul_overflow(no, o, &no)) return "tensor too large";
    }
    if (no > INT64_MAX / 2) return "tensor too large";
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    if (ranges_overlap(in_dev, ni * es, out_dev, no * es)) return "the output overlaps the input";
    *in_elems = ni, *out_elems = no;
    return NULL;
}

// The one place that chooses the form (launch and name).  SHL_MI355X_PAD_FORM=generic forces the literal form (A/B runs,
// tests); read per call.  *j: the innermost padded dim (vec)
static int pad_form(const void *in_dev, const void *out_dev, const shl_mi355x_pad_desc *d, int *j)
{
    *j = 0;
    for (int k = 3; k > 0; --k)
        if (d->before[k] != 0 || d->after[k] != 0) {
            *j = k;
            break;
        }
    const char *force = getenv("SHL_MI355X_PAD_FORM");
    if (force && strcmp(force, "generic") == 0) return PAD_GENERIC;
    if ((((uintptr_t)in_dev | (uintptr_t)out_dev) & 15) != 0) return PAD_GENERIC;
    int64_t unit = d->dtype == SHL_MI355X_F16 ? 2 : 1;  // bytes of one step along dim j
    for (int k = *j + 1; k < 4; ++k) unit *= d->dim[k];
    if ((d->before[*j] * unit) % 16 != 0 || (d->dim[*j] * unit) % 16 != 0 || (d->after[*j] * unit) % 16 != 0) return PAD_GENERIC;
    return PAD_VEC;
}

}  // namespace shl

extern "C" uint32_t shl_mi355x_pad_element(const struct shl_mi355x_pad_desc *d)
{
    if (!d || (d->dtype != SHL_MI355X_I8 && d->dtype != SHL_MI355X_F16)) return 0;
    return shl::pad_element(d);
}

extern "C" const char *shl_mi355x_pad_kernel_name(const void *in_dev, const void *out_dev, const struct shl_mi355x_pad_desc *d)
{
    int64_t ni, no;
    if (shl::pad_invalid(in_dev, out_dev, d, &ni, &no)) return "";
    int j;
    return shl::pad_form(in_dev, out_dev, d, &j) == shl::PAD_VEC ? "pad_vec" : "pad_generic";
}

extern "C" int shl_mi355x_pad(const void *in_dev, void *out_dev, const struct shl_mi355x_pad_desc *d, void *stream)
{
    using namespace shl;
    int64_t ni, no;
    const char *why = pad_invalid(in_dev, out_dev, d, &ni, &no);
    if (why) {
        set_error("pad: %s", why);
        return SHL_MI355X_EINVAL;
    }
    if (no == 0) return SHL_MI355X_OK;
    const bool f16 = d->dtype == SHL_MI355X_F16;
    int j;
    const int form = pad_form(in_dev, out_dev, d, &j);
    PadArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in_dev, a.out = out_dev;
    if (form == PAD_VEC) {
        // dims 0 .. j, right-aligned, the dims behind j merged into it and counted in 16-byte pieces
        int64_t unit = f16 ? 2 : 1;
        for (int k = j + 1; k < 4; ++k) unit *= d->dim[k];
        const int shift = 3 - j;
        for (int k = 0; k < 4; ++k) a.oe[k] = 1, a.ie[k] = 1, a.bf[k] = 0;
        for (int k = 0; k <= j; ++k) {
            a.ie[k + shift] = d->dim[k], a.bf[k + shift] = d->before[k];
            a.oe[k + shift] = (int64_t)d->dim[k] + d->before[k] + d->after[k];
        }
        a.ie[3] = a.ie[3] * unit / 16, a.bf[3] = a.bf[3] * unit / 16, a.oe[3] = a.oe[3] * unit / 16;
        a.items = no * (f16 ? 2 : 1) / 16;
    } else {
        for (int k = 0; k < 4; ++k) {
            a.ie[k] = d->dim[k], a.bf[k] = d->before[k];
            a.oe[k] = (int64_t)d->dim[k] + d->before[k] + d->after[k];
        }
        a.items = no;
    }
    const uint32_t e = pad_element(d);
    a.pad = f16 ? e * 0x00010001u : e * 0x01010101u;
    a.rec = move_rec(d->in_scale, d->in_zp, d->out_scale, d->out_zp, !f16 && form == PAD_VEC);
    a.small = no < (1ll << 32);
    const int64_t groups = (a.items + 255) / 256;
    if (grid_refused("pad", groups)) return SHL_MI355X_ENOTSUP;
    const dim3 grid((unsigned)groups), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (form == PAD_VEC) hipLaunchKernelGGL(f16 ? pad_vec_kernel<true> : pad_vec_kernel<false>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(f16 ? pad_generic_kernel<true> : pad_generic_kernel<false>, grid, block, 0, s, a);
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

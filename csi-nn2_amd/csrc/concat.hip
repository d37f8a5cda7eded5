// concat.hip -- concat of int8 / binary16 tensors along one axis (CSINN_OP_CONCAT).
//
// Restates shl_ref_concat_quant (source/reference/concat.c:21-76): every input is converted to float32 with its own
// record, slabs are copied -- for each of `outer` steps input i contributes len_i consecutive elements, in input order --
// and the float32 result is converted to the output's dtype with the output's record.  Per element:
//   int8      q_out = sat8(rint(((q - zp_i) * s_i) / s_out) + zp_out)     (int8_to_float_base, float_to_int8_base)
//   binary16  float32_to_float16_base(float16_to_float32_base(h)): every finite value and both zeros come back unchanged,
//             +-inf become +-65504 (0x7BFF / 0xFBFF), every NaN becomes 0x7FFF / 0xFFFF by its sign
// Nothing is summed: results are bit-identical to the reference for any records.
//
// The output is [outer][row], row = sum of len_i; input i is [outer][len_i] at column off_i.  Up to 8 inputs travel BY
// VALUE in the kernel arguments of one launch (pointer, len, off, record, raw flag): nothing is uploaded, the launch can be
// captured.  More inputs run as further launches over the next 8 (their output slices are disjoint).  Two forms, chosen
// by concat_form() below, which also names them:
//   vec       16 bytes per thread, indexed in OUTPUT order: stores are fully coalesced, loads coalesced within a slab; a
//             thread finds its input by comparing its column with the (at most 8) offsets.  Needs every len_i in bytes a
//             multiple of 16 (off_i and row then are too) and every pointer 16-byte aligned: NHWC channel concat of int8
//             channels in multiples of 16 / binary16 in multiples of 8, NCHW channel concat when C_i H W bytes % 16 == 0.
//             int8: an input whose record equals the output's is copied as bytes once the round trip was checked to be
//             the identity on all 256 values (requant_is_identity, pool2d.hip); the others take sixteen requantisations,
//             the division by div_by_scale (common.h) where the records admit it.  binary16: the two-rule fix-up above on
//             packed halves, in integer operations.
//   generic   one element per thread, any lengths and alignment: the literal formula (hardware division, the binary16
//             round trip through float32), raw copies included -- tests/test_concat.py runs every case through both.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"

namespace shl {

bool requant_is_identity(float s, int32_t zp);  // pool2d.hip

constexpr int CONCAT_MAX = 8;  // inputs per launch

enum { CONCAT_VEC = 0, CONCAT_GENERIC = 1 };

// len / off / row / base / width in the form's unit: 16-byte pieces (vec) or elements (generic)
struct ConcatIn {
    const void *p;
    int64_t len;  // per outer step
    int64_t off;  // first column INSIDE this launch's slice; unused entries: INT64_MAX
    float s, z;
    int32_t raw;  // int8 vec: copy the bytes
    int32_t pad;
};

struct ConcatArgs {
    ConcatIn in[CONCAT_MAX];
    void *out;
    int64_t row;    // the whole output row
    int64_t base;   // first column of this launch's slice
    int64_t width;  // columns of this launch's slice
    int64_t items;  // outer * width
    float so, zo, inv_so;
    int32_t fma_div;  // div_by_scale is exact for every non-raw input of this launch
};

// the input that owns column `col` of the slice: the last one whose offset is not behind it (offsets ascend).  Field by
// field: a select between whole entries made the compiler spill the argument block to scratch and index it
__device__ __forceinline__ ConcatIn concat_pick(const ConcatArgs &a, int64_t col)
{
    const void *p = a.in[0].p;
    int64_t len = a.in[0].len, off = a.in[0].off;
    float s = a.in[0].s, z = a.in[0].z;
    int32_t raw = a.in[0].raw;
#pragma unroll
    for (int j = 1; j < CONCAT_MAX; ++j) {
        const bool mine = col >= a.in[j].off;
        p = mine ? a.in[j].p : p;
        len = mine ? a.in[j].len : len, off = mine ? a.in[j].off : off;
        s = mine ? a.in[j].s : s, z = mine ? a.in[j].z : z;
        raw = mine ? a.in[j].raw : raw;
    }
    ConcatIn r;
    r.p = p, r.len = len, r.off = off, r.s = s, r.z = z, r.raw = raw, r.pad = 0;
    return r;
}

template <bool FMA>
__device__ __forceinline__ int concat_rq(int q, float s, float z, const ConcatArgs &a)
{
    const float x = __fmul_rn(__fsub_rn((float)q, z), s);  // int8_to_float_base (source/nn2/utils.c:499-502)
    const float d = FMA ? div_by_scale(x, a.so, a.inv_so) : __fdiv_rn(x, a.so);
    return sat8_from_float(__fadd_rn(rintf(d), a.zo));  // float_to_int8_base (:550-560)
}

template <bool FMA>
__device__ __forceinline__ uint32_t concat_rq4(uint32_t w, float s, float z, const ConcatArgs &a)
{
    return pack4_i8(concat_rq<FMA>((int8_t)w, s, z, a), concat_rq<FMA>((int8_t)(w >> 8), s, z, a),
                    concat_rq<FMA>((int8_t)(w >> 16), s, z, a), concat_rq<FMA>((int8_t)(w >> 24), s, z, a));
}

// two packed binary16 values through float16 -> float32 -> float32_to_float16_base: a half whose magnitude bits reach
// 0x7C00 is an infinity (-> 0x7BFF) or a NaN (-> 0x7FFF), the sign stays; everything below comes back unchanged
__device__ __forceinline__ uint32_t concat_fix_f16x2(uint32_t w)
{
    const uint32_t m = w & 0x7FFF7FFFu;
    const uint32_t special = (m + 0x04000400u) & 0x80008000u;  // per half: m >= 0x7C00 (no carry leaves a half)
    if (special == 0u) return w;
    const uint32_t mask = (special >> 15) * 0xFFFFu;
    const uint32_t nan = (((m + 0x03FF03FFu) & 0x80008000u) >> 15) * 0xFFFFu;  // per half: m > 0x7C00
    const uint32_t repl = 0x7BFF7BFFu | (nan & 0x04000400u) | (w & 0x80008000u);
    return (w & ~mask) | (repl & mask);
}

template <bool F16>
__global__ __launch_bounds__(256) void concat_vec_kernel(ConcatArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (outer step, piece of the slice), piece fastest
    if (i >= a.items) return;
    const int64_t k = i / a.width;
    const int64_t col = i - k * a.width;
    const ConcatIn in = concat_pick(a, col);
    uint4 v = static_cast<const uint4 *>(in.p)[k * in.len + (col - in.off)];
    if constexpr (F16) {
        v.x = concat_fix_f16x2(v.x), v.y = concat_fix_f16x2(v.y), v.z = concat_fix_f16x2(v.z), v.w = concat_fix_f16x2(v.w);
    } else if (!in.raw) {
        if (a.fma_div) {
            v.x = concat_rq4<true>(v.x, in.s, in.z, a), v.y = concat_rq4<true>(v.y, in.s, in.z, a);
            v.z = concat_rq4<true>(v.z, in.s, in.z, a), v.w = concat_rq4<true>(v.w, in.s, in.z, a);
        } else {
            v.x = concat_rq4<false>(v.x, in.s, in.z, a), v.y = concat_rq4<false>(v.y, in.s, in.z, a);
            v.z = concat_rq4<false>(v.z, in.s, in.z, a), v.w = concat_rq4<false>(v.w, in.s, in.z, a);
        }
    }
    static_cast<uint4 *>(a.out)[k * a.row + a.base + col] = v;
}

template <bool F16>
__global__ __launch_bounds__(256) void concat_generic_kernel(ConcatArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (outer step, element of the slice), element fastest
    if (i >= a.items) return;
    const int64_t k = i / a.width;
    const int64_t col = i - k * a.width;
    const ConcatIn in = concat_pick(a, col);
    const int64_t src = k * in.len + (col - in.off), dst = k * a.row + a.base + col;
    if constexpr (F16) {
        static_cast<uint16_t *>(a.out)[dst] = float_to_f16_bits_ref(f16_bits_to_float(static_cast<const uint16_t *>(in.p)[src]));
    } else {
        static_cast<int8_t *>(a.out)[dst] = (int8_t)concat_rq<false>(static_cast<const int8_t *>(in.p)[src], in.s, in.z, a);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------
// NULL when the arguments describe a concat, else what is wrong with them; *row: the output row in elements
static const char *concat_invalid(const void *const *in_dev, const int64_t *len, const float *in_scale, const int32_t *in_zp,
                                  const void *out_dev, const shl_mi355x_concat_desc *d, int64_t *row)
{
    if (!d || !in_dev || !len || !out_dev) return "NULL argument";
    if (d->dtype != SHL_MI355X_I8 && d->dtype != SHL_MI355X_F16) return "dtype is neither int8 nor binary16";
    if (d->dtype == SHL_MI355X_I8 && (!in_scale || !in_zp)) return "NULL argument";
    if (d->n_inputs < 1) return "n_inputs < 1";
    if (d->outer < 0) return "negative outer";
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    int64_t total = 0;
    for (int i = 0; i < d->n_inputs; ++i) {
        if (len[i] < 0) return "negative length";
        if (len[i] > 0 && !in_dev[i]) return "NULL input";
        if (__builtin_add_overflow(total, len[i], &total)) return "row too long";
    }
    int64_t bytes;
    if (__builtin_mul_overflow(total, d->outer, &bytes) || __builtin_mul_overflow(bytes, es, &bytes)) return "tensor too large";
    const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)bytes;
    for (int i = 0; i < d->n_inputs; ++i) {
        const uintptr_t p0 = (uintptr_t)in_dev[i], p1 = p0 + (uintptr_t)(len[i] * d->outer * es);
        if (p0 < p1 && p0 < o1 && o0 < p1) return "the output overlaps an input";
    }
    *row = total;
    return NULL;
}

// The one place that chooses the form (launch and name).  SHL_MI355X_CONCAT_FORM=generic forces the literal form
// (A/B runs, tests); read per call.
static int concat_form(const void *const *in_dev, const int64_t *len, const void *out_dev, const shl_mi355x_concat_desc *d)
{
    const char *force = getenv("SHL_MI355X_CONCAT_FORM");
    if (force && strcmp(force, "generic") == 0) return CONCAT_GENERIC;
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    if (((uintptr_t)out_dev & 15) != 0) return CONCAT_GENERIC;
    for (int i = 0; i < d->n_inputs; ++i) {
        if (len[i] == 0) continue;
        // every length a multiple of 16 bytes: every offset and the row then are too
        if ((len[i] * es) % 16 != 0 || ((uintptr_t)in_dev[i] & 15) != 0) return CONCAT_GENERIC;
    }
    return CONCAT_VEC;
}

// div_by_scale(x, so, RN(1 / so)) == x / so for every x = (q - zp) * s this input can produce (common.h; the range
// conv_plan.hip:fma_division_ok admits: 2^-40 <= so <= 2^40, |x| <= 2^60, x finite)
static bool concat_fma_ok(float s, int32_t zp, float so)
{
    if (!(so >= 0x1p-40f && so <= 0x1p40f)) return false;
    const double bound = (128.0 + fabs((double)zp)) * fabs((double)s);
    return bound <= 0x1p60;  // also NaN
}

}  // namespace shl

extern "C" const char *shl_mi355x_concat_kernel_name(const void *const *in_dev, const int64_t *len, const float *in_scale,
                                                     const int32_t *in_zp, const void *out_dev,
                                                     const struct shl_mi355x_concat_desc *d)
{
    int64_t row;
    if (shl::concat_invalid(in_dev, len, in_scale, in_zp, out_dev, d, &row)) return "";
    return shl::concat_form(in_dev, len, out_dev, d) == shl::CONCAT_VEC ? "concat_vec" : "concat_generic";
}

extern "C" int shl_mi355x_concat(const void *const *in_dev, const int64_t *len, const float *in_scale, const int32_t *in_zp,
                                 void *out_dev, const struct shl_mi355x_concat_desc *d, void *stream)
{
    using namespace shl;
    int64_t row;
    const char *why = concat_invalid(in_dev, len, in_scale, in_zp, out_dev, d, &row);
    if (why) {
        set_error("concat: %s", why);
        return SHL_MI355X_EINVAL;
    }
    if (d->outer == 0 || row == 0) return SHL_MI355X_OK;
    const bool f16 = d->dtype == SHL_MI355X_F16;
    const int form = concat_form(in_dev, len, out_dev, d);
    const int64_t unit = form == CONCAT_VEC ? (f16 ? 8 : 16) : 1;  // elements per column of the form
    // no launch has more workgroups than one over the whole row would: checked before anything is enqueued
    if ((row / unit * d->outer + 255) / 256 > 0x7FFFFFFFll) {
        set_error("concat: %lld workgroups exceed the grid", (long long)((row / unit * d->outer + 255) / 256));
        return SHL_MI355X_ENOTSUP;
    }
    int identity = -1;  // is requantising with the output's record the identity?  asked once, when first needed
    hipStream_t s = (hipStream_t)stream;
    int64_t base = 0;  // first column of the next launch, in elements
    int i = 0;
    while (i < d->n_inputs) {
        ConcatArgs a;
        memset(&a, 0, sizeof(a));
        a.out = out_dev;
        a.row = row / unit, a.base = base / unit;
        a.so = d->out_scale, a.zo = (float)d->out_zp, a.inv_so = 1.0f / d->out_scale;
        a.fma_div = 1;
        int64_t width = 0;
        int taken = 0;
        for (; i < d->n_inputs && taken < CONCAT_MAX; ++i) {
            if (len[i] == 0) continue;  // the reference's float loop skips it too
            ConcatIn &e = a.in[taken++];
            e.p = in_dev[i], e.len = len[i] / unit, e.off = width / unit;
            if (!f16) {
                e.s = in_scale[i], e.z = (float)in_zp[i];
                if (form == CONCAT_VEC && in_zp[i] == d->out_zp && memcmp(&in_scale[i], &d->out_scale, sizeof(float)) == 0) {
                    if (identity < 0) identity = requant_is_identity(d->out_scale, d->out_zp) ? 1 : 0;
                    e.raw = identity;
                }
                if (!e.raw && !concat_fma_ok(in_scale[i], in_zp[i], d->out_scale)) a.fma_div = 0;
            }
            width += len[i];
        }
        for (int j = taken; j < CONCAT_MAX; ++j) a.in[j] = a.in[0], a.in[j].off = INT64_MAX;
        base += width;
        if (taken == 0) break;  // only zero-length inputs were left
        a.width = width / unit;
        a.items = a.width * d->outer;
        const dim3 grid((unsigned)((a.items + 255) / 256)), block(256);
        if (form == CONCAT_VEC) hipLaunchKernelGGL(f16 ? concat_vec_kernel<true> : concat_vec_kernel<false>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(f16 ? concat_generic_kernel<true> : concat_generic_kernel<false>, grid, block, 0, s, a);
        SHL_HIP(hipGetLastError());
    }
    return SHL_MI355X_OK;
}

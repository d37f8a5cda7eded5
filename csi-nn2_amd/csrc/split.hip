// split.hip -- split of an int8 / binary16 tensor along one axis into several tensors (CSINN_OP_SPLIT): concat's mirror.
//
// Restates shl_ref_split_quant (source/reference/split.c:21-92): the input is converted to float32 with its record, for
// each of `outer` steps output i receives len_i consecutive elements, in output order, and every float32 output is
// converted to its dtype with ITS OWN record.  Per element (requant_move.h):
//   int8      q_out = sat8(rint(((q - zp_in) * s_in) / s_out_i) + zp_out_i)
//   binary16  float32_to_float16_base(float16_to_float32_base(h))
// Nothing is summed: results are bit-identical to the reference for any records.
//
// The input is [outer][row], row = sum of len_i; output i is [outer][len_i] and holds the columns from off_i on.  Up to 8
// outputs travel BY VALUE in the kernel arguments of one launch (pointer, len, off, record, how to move): nothing is
// uploaded, the launch can be captured.  More outputs run as further launches over the next 8, each indexing only its own
// slice of the row.  Two forms, chosen by split_form() below, which also names them:
//   vec       16 bytes per thread, indexed in INPUT order: loads are fully coalesced, stores coalesced within a slab; a
//             thread finds its output by comparing its column with the (at most 8) offsets.  Needs every len_i in bytes a
//             multiple of 16 (off_i and row then are too) and every pointer 16-byte aligned.  int8: an output whose record
//             equals the input's is copied as bytes once the round trip was checked to be the identity on all 256 values
//             (requant_is_identity, pool2d.hip); the others take sixteen requantisations, the division by div_by_scale
//             (common.h) where the records admit it.  binary16: the two-rule fix-up on packed halves.
//   generic   one element per thread, any lengths and alignment: the literal formula (hardware division, the binary16
//             round trip through float32), raw copies included.
#include <stdlib.h>
#include <string.h>

#include "requant_move.h"

namespace shl {

constexpr int SPLIT_MAX = 8;  // outputs per launch

enum { SPLIT_VEC = 0, SPLIT_GENERIC = 1 };

// len / off / row / base / width in the form's unit: 16-byte pieces (vec) or elements (generic)
struct SplitOut {
    void *p;
    int64_t len;  // per outer step
    int64_t off;  // first column INSIDE this launch's slice; unused entries: INT64_MAX
    float s, z, inv_s;
    int32_t mode;  // int8 vec: MOVE_RAW / MOVE_FMA / MOVE_DIV
};

struct SplitArgs {
    SplitOut out[SPLIT_MAX];
    const void *in;
    int64_t row;    // the whole input row
    int64_t base;   // first column of this launch's slice
    int64_t width;  // columns of this launch's slice
    int64_t items;  // outer * width
    float si, zi;
    int32_t small;  // outer * row < 2^32: every index fits 32 bits
};

// the output that owns column `col` of the slice: the last one whose offset is not behind it (offsets ascend).  Field by
// field, as concat_pick: a select between whole entries makes the compiler index the argument block in scratch
__device__ __forceinline__ SplitOut split_pick(const SplitArgs &a, int64_t col)
{
    void *p = a.out[0].p;
    int64_t len = a.out[0].len, off = a.out[0].off;
    float s = a.out[0].s, z = a.out[0].z, inv_s = a.out[0].inv_s;
    int32_t mode = a.out[0].mode;
#pragma unroll
    for (int j = 1; j < SPLIT_MAX; ++j) {
        const bool mine = col >= a.out[j].off;
        p = mine ? a.out[j].p : p;
        len = mine ? a.out[j].len : len, off = mine ? a.out[j].off : off;
        s = mine ? a.out[j].s : s, z = mine ? a.out[j].z : z, inv_s = mine ? a.out[j].inv_s : inv_s;
        mode = mine ? a.out[j].mode : mode;
    }
    SplitOut r;
    r.p = p, r.len = len, r.off = off, r.s = s, r.z = z, r.inv_s = inv_s, r.mode = mode;
    return r;
}

template <bool F16>
__global__ __launch_bounds__(256) void split_vec_kernel(SplitArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (outer step, piece of the slice), piece fastest
    if (i >= a.items) return;
    int64_t col;
    const int64_t k = move_divmod(i, a.width, a.small != 0, col);
    const SplitOut o = split_pick(a, col);
    uint4 v = static_cast<const uint4 *>(a.in)[k * a.row + a.base + col];
    v.x = move_word<F16>(v.x, o.mode, a.si, a.zi, o.s, o.z, o.inv_s), v.y = move_word<F16>(v.y, o.mode, a.si, a.zi, o.s, o.z, o.inv_s);
    v.z = move_word<F16>(v.z, o.mode, a.si, a.zi, o.s, o.z, o.inv_s), v.w = move_word<F16>(v.w, o.mode, a.si, a.zi, o.s, o.z, o.inv_s);
    static_cast<uint4 *>(o.p)[k * o.len + (col - o.off)] = v;
}

template <bool F16>
__global__ __launch_bounds__(256) void split_generic_kernel(SplitArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (outer step, element of the slice), element fastest
    if (i >= a.items) return;
    int64_t col;
    const int64_t k = move_divmod(i, a.width, a.small != 0, col);
    const SplitOut o = split_pick(a, col);
    const int64_t src = k * a.row + a.base + col, dst = k * o.len + (col - o.off);
    if constexpr (F16) {
        static_cast<uint16_t *>(o.p)[dst] = float_to_f16_bits_ref(f16_bits_to_float(static_cast<const uint16_t *>(a.in)[src]));
    } else {
        static_cast<int8_t *>(o.p)[dst] =
            (int8_t)move_rq<false>(static_cast<const int8_t *>(a.in)[src], a.si, a.zi, o.s, o.z, o.inv_s);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------
// NULL when the arguments describe a split, else what is wrong with them; *row: the input row in elements
static const char *split_invalid(const void *in_dev, void *const *out_dev, const int64_t *len, const float *out_scale,
                                 const int32_t *out_zp, const shl_mi355x_split_desc *d, int64_t *row)
{
    if (!d || !in_dev || !out_dev || !len) return "NULL argument";
    if (d->dtype != SHL_MI355X_I8 && d->dtype != SHL_MI355X_F16) return "dtype is neither int8 nor binary16";
    if (d->dtype == SHL_MI355X_I8 && (!out_scale || !out_zp)) return "NULL argument";
    if (d->n_outputs < 1) return "n_outputs < 1";
    if (d->outer < 0) return "negative outer";
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    int64_t total = 0;
    for (int i = 0; i < d->n_outputs; ++i) {
        if (len[i] <= 0) return "an output of length <= 0";
        if (!out_dev[i]) return "NULL output";
        if (__builtin_add_overflow(total, len[i], &total)) return "row too long";
    }
    int64_t bytes;
    if (__builtin_mul_overflow(total, d->outer, &bytes) || __builtin_mul_overflow(bytes, es, &bytes)) return "tensor too large";
    const uintptr_t i0 = (uintptr_t)in_dev, i1 = i0 + (uintptr_t)bytes;
    for (int i = 0; i < d->n_outputs; ++i) {
        const uintptr_t p0 = (uintptr_t)out_dev[i], p1 = p0 + (uintptr_t)(len[i] * d->outer * es);
        if (p0 < p1 && p0 < i1 && i0 < p1) return "an output overlaps the input";
        for (int j = 0; j < i; ++j) {
            const uintptr_t q0 = (uintptr_t)out_dev[j], q1 = q0 + (uintptr_t)(len[j] * d->outer * es);
            if (p0 < p1 && q0 < q1 && p0 < q1 && q0 < p1) return "two outputs overlap";
        }
    }
    *row = total;
    return NULL;
}

// The one place that chooses the form (launch and name).  SHL_MI355X_SPLIT_FORM=generic forces the literal form (A/B runs,
// tests); `vec` asks for the vector form, which the arguments must still admit; read per call.
static int split_form(const void *in_dev, void *const *out_dev, const int64_t *len, const shl_mi355x_split_desc *d)
{
    const char *force = getenv("SHL_MI355X_SPLIT_FORM");
    if (force && strcmp(force, "generic") == 0) return SPLIT_GENERIC;
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    if (((uintptr_t)in_dev & 15) != 0) return SPLIT_GENERIC;
    for (int i = 0; i < d->n_outputs; ++i) {
        // every length a multiple of 16 bytes: every offset and the row then are too
        if ((len[i] * es) % 16 != 0 || ((uintptr_t)out_dev[i] & 15) != 0) return SPLIT_GENERIC;
    }
    return SPLIT_VEC;
}

}  // namespace shl

extern "C" const char *shl_mi355x_split_kernel_name(const void *in_dev, void *const *out_dev, const int64_t *len,
                                                    const float *out_scale, const int32_t *out_zp,
                                                    const struct shl_mi355x_split_desc *d)
{
    int64_t row;
    if (shl::split_invalid(in_dev, out_dev, len, out_scale, out_zp, d, &row)) return "";
    return shl::split_form(in_dev, out_dev, len, d) == shl::SPLIT_VEC ? "split_vec" : "split_generic";
}

extern "C" int shl_mi355x_split(const void *in_dev, void *const *out_dev, const int64_t *len, const float *out_scale,
                                const int32_t *out_zp, const struct shl_mi355x_split_desc *d, void *stream)
{
    using namespace shl;
    int64_t row;
    const char *why = split_invalid(in_dev, out_dev, len, out_scale, out_zp, d, &row);
    if (why) {
        set_error("split: %s", why);
        return SHL_MI355X_EINVAL;
    }
    if (d->outer == 0) return SHL_MI355X_OK;
    const bool f16 = d->dtype == SHL_MI355X_F16;
    const int form = split_form(in_dev, out_dev, len, d);
    const int64_t unit = form == SPLIT_VEC ? (f16 ? 8 : 16) : 1;  // elements per column of the form
    // no launch has more workgroups than one over the whole row would: checked before anything is enqueued
    if ((row / unit * d->outer + 255) / 256 > 0x7FFFFFFFll) {
        set_error("split: %lld workgroups exceed the grid", (long long)((row / unit * d->outer + 255) / 256));
        return SHL_MI355X_ENOTSUP;
    }
    int identity = -1;  // is requantising with the input's record the identity?  asked once, when first needed
    hipStream_t s = (hipStream_t)stream;
    int64_t base = 0;  // first column of the next launch, in elements
    int i = 0;
    while (i < d->n_outputs) {
        SplitArgs a;
        memset(&a, 0, sizeof(a));
        a.in = in_dev;
        a.row = row / unit, a.base = base / unit;
        a.si = d->in_scale, a.zi = (float)d->in_zp;
        a.small = row * d->outer < (1ll << 32);  // (no overflow: split_invalid multiplied them)
        int64_t width = 0;
        int taken = 0;
        for (; i < d->n_outputs && taken < SPLIT_MAX; ++i) {
            SplitOut &e = a.out[taken++];
            e.p = out_dev[i], e.len = len[i] / unit, e.off = width / unit;
            if (!f16) {
                e.s = out_scale[i], e.z = (float)out_zp[i], e.inv_s = 1.0f / out_scale[i];
                e.mode = move_fma_ok(d->in_scale, d->in_zp, out_scale[i]) ? MOVE_FMA : MOVE_DIV;
                if (form == SPLIT_VEC && out_zp[i] == d->in_zp && memcmp(&out_scale[i], &d->in_scale, sizeof(float)) == 0) {
                    if (identity < 0) identity = requant_is_identity(d->in_scale, d->in_zp) ? 1 : 0;
                    if (identity) e.mode = MOVE_RAW;
                }
            }
            width += len[i];
        }
        for (int j = taken; j < SPLIT_MAX; ++j) a.out[j] = a.out[0], a.out[j].off = INT64_MAX;
        base += width;
        a.width = width / unit;
        a.items = a.width * d->outer;
        const dim3 grid((unsigned)((a.items + 255) / 256)), block(256);
        if (form == SPLIT_VEC) hipLaunchKernelGGL(f16 ? split_vec_kernel<true> : split_vec_kernel<false>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(f16 ? split_generic_kernel<true> : split_generic_kernel<false>, grid, block, 0, s, a);
        SHL_HIP(hipGetLastError());
    }
    return SHL_MI355X_OK;
}

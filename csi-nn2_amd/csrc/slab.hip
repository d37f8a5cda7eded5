// slab.hip -- concat of int8 / binary16 tensors along one axis (CSINN_OP_CONCAT) and its mirror, split of one tensor into
// several (CSINN_OP_SPLIT): one kernel pair that copies slabs between a WHOLE tensor and its PARTS, in either direction.
//
// Restates shl_ref_concat_quant (source/reference/concat.c:21-76) and shl_ref_split_quant (source/reference/split.c:21-92):
// every source is converted to float32 with its own record, slabs are copied -- for each of `outer` steps part i holds
// len_i consecutive elements of the whole's row, in part order -- and every float32 destination is converted to its dtype
// with ITS OWN record.  Per element (requant_move.h):
//   int8      q_out = sat8(rint(((q - zp_in) * s_in) / s_out) + zp_out)
//   binary16  float32_to_float16_base(float16_to_float32_base(h))
// Nothing is summed: results are bit-identical to the reference for any records.
//
// The whole is [outer][row], row = sum of len_i; part i is [outer][len_i] and holds the columns from off_i on.  GATHER
// (concat): the parts are the sources, the whole is the output and the common record is the output's.  Otherwise (split): the
// parts are the destinations and the common record is the input's.  Up to 8 parts travel BY VALUE in the kernel arguments of
// one launch (pointer, len, off, record, how to move): nothing is uploaded, the launch can be captured.  More parts run as
// further launches over the next 8, each indexing only its own slice of the row (the slices are disjoint).  Two forms, chosen
// by slab_form() below, which also names them:
//   vec       16 bytes per thread, indexed in the WHOLE's order: its side is fully coalesced, the parts' side coalesced
//             within a slab; a thread finds its part by comparing its column with the (at most 8) offsets.  Needs every len_i
//             in bytes a multiple of 16 (off_i and row then are too) and every pointer 16-byte aligned: NHWC channel concat of
//             int8 channels in multiples of 16 / binary16 in multiples of 8, NCHW channel concat when C_i H W bytes % 16 == 0.
//             int8: a part whose record equals the whole's is copied as bytes once the round trip was checked to be the
//             identity on all 256 values (requant_is_identity, pool2d.hip); the others take sixteen requantisations, the
//             division by div_by_scale (common.h) where that part's records admit it.  binary16: the two-rule fix-up on
//             packed halves, in integer operations.
//   generic   one element per thread, any lengths and alignment: the literal formula (hardware division, the binary16
//             round trip through float32), raw copies included -- tests/test_concat.py and tests/test_split_shuffle.py run
//             every case through both.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "requant_move.h"

namespace shl {

constexpr int SLAB_MAX = 8;  // parts per launch

enum { SLAB_VEC = 0, SLAB_GENERIC = 1 };

// len / off / row / width in the form's unit: 16-byte pieces (vec) or elements (generic)
struct SlabPart {
    void *p;
    int64_t len;  // per outer step
    int64_t off;  // first column INSIDE this launch's slice; unused entries: INT64_MAX
    float s, z, inv_s;
    int32_t mode;  // int8 vec: MOVE_RAW / MOVE_FMA / MOVE_DIV
};

struct SlabArgs {
    SlabPart part[SLAB_MAX];
    void *whole;    // at the first column of this launch's slice
    int64_t row;    // the whole's row
    int64_t width;  // columns of this launch's slice
    int64_t items;  // outer * width
    float s, z, inv_s;  // the whole's record
    int32_t small;      // outer * row < 2^32: every index fits 32 bits (read by the scatter kernels)
};

// the part that owns column `col` of the slice: the last one whose offset is not behind it (offsets ascend).  Field by
// field: a select between whole entries made the compiler copy the argument block to scratch (256 bytes) and index it there
// (profiles/concat_notes.md).  The first part starts the slice, so its offset is 0: saying so, and keeping the slice's first
// column in the `whole` pointer rather than in a field, spares four scalar registers in kernels that hold the whole table
// in them (the figures per kernel: profiles/concat_notes.md).
// Where the part is and how it travels (the result's record fields stay unset) ...
__device__ __forceinline__ SlabPart slab_pick(const SlabArgs &a, int64_t col)
{
    SlabPart r;
    r.p = a.part[0].p, r.len = a.part[0].len, r.off = 0, r.mode = a.part[0].mode;
#pragma unroll
    for (int j = 1; j < SLAB_MAX; ++j) {
        const bool mine = col >= a.part[j].off;
        r.p = mine ? a.part[j].p : r.p;
        r.len = mine ? a.part[j].len : r.len, r.off = mine ? a.part[j].off : r.off;
        r.mode = mine ? a.part[j].mode : r.mode;
    }
    return r;
}

// ... and, picked apart from it so that a raw copy never pays for them, the records of the move between that part and the whole
template <bool GATHER>
__device__ __forceinline__ MoveRec slab_rec(const SlabArgs &a, int64_t col, int32_t mode)
{
    float s = a.part[0].s, z = a.part[0].z, inv_s = a.part[0].inv_s;
#pragma unroll
    for (int j = 1; j < SLAB_MAX; ++j) {
        const bool mine = col >= a.part[j].off;
        s = mine ? a.part[j].s : s, z = mine ? a.part[j].z : z, inv_s = mine ? a.part[j].inv_s : inv_s;
    }
    MoveRec r;
    if constexpr (GATHER) r.si = s, r.zi = z, r.so = a.s, r.zo = a.z, r.inv_so = a.inv_s;
    else r.si = a.s, r.zi = a.z, r.so = s, r.zo = z, r.inv_so = inv_s;
    r.mode = mode;
    return r;
}

// thread i owns unit i of the slice, (outer step, column) with the column fastest, on both sides: W = uint4 is the vec form,
// W = the element the generic one
template <bool GATHER, bool F16, typename W>
__device__ __forceinline__ void slab_move(const SlabArgs &a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.items) return;
    int64_t k, col;
    if constexpr (GATHER) {
        // A gather's load waits for the part it reads from, so for the whole table of pointers, lengths and offsets: ask for
        // it HERE, in one batch of scalar loads.  Left alone, the compiler fetches a third of it behind the division, and a
        // wave of raw copies waits for a second and a third round trip (10 % of a concat of raw copies, measured:
        // profiles/move_refactor_notes.md).  For the same reason the division stays the 64-bit one, whose expansion has
        // its own 32-bit path: move_divmod's switch costs the registers that keep the table in one batch at 8 waves
#pragma unroll
        for (int j = 0; j < SLAB_MAX; ++j) asm volatile("" ::"s"(a.part[j].p), "s"(a.part[j].len), "s"(a.part[j ? j : 1].off));
        k = i / a.width, col = i - k * a.width;
    } else {
        k = move_divmod(i, a.width, a.small != 0, col);  // (a scatter's load needs no part: nothing waits for the table)
    }
    const SlabPart t = slab_pick(a, col);
    W *part = static_cast<W *>(t.p) + (k * t.len + (col - t.off)), *whole = static_cast<W *>(a.whole) + (k * a.row + col);
    W v = GATHER ? *part : *whole;
    // (one look at the mode lets a raw copy pass the records and the four dwords' decisions by)
    if constexpr (sizeof(W) != 16) v = (W)move_literal<F16>(v, slab_rec<GATHER>(a, col, t.mode));
    else if (F16 || t.mode != MOVE_RAW) v = move_piece<W, F16>(v, slab_rec<GATHER>(a, col, t.mode));
    *(GATHER ? whole : part) = v;
}

template <bool GATHER, bool F16>
__global__ __launch_bounds__(256) void slab_vec_kernel(SlabArgs a)
{
    slab_move<GATHER, F16, uint4>(a);
}

template <bool GATHER, bool F16>
__global__ __launch_bounds__(256) void slab_generic_kernel(SlabArgs a)
{
    slab_move<GATHER, F16, typename std::conditional<F16, uint16_t, uint8_t>::type>(a);
}

// ---- host side ---------------------------------------------------------------------------------------------
// The two checks stay apart: concat skips a zero-length input where split refuses such an output, and split compares its
// outputs pairwise.
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
    for (int i = 0; i < d->n_inputs; ++i)
        if (ranges_overlap(in_dev[i], len[i] * d->outer * es, out_dev, bytes)) return "the output overlaps an input";
    *row = total;
    return NULL;
}

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
    for (int i = 0; i < d->n_outputs; ++i) {
        if (ranges_overlap(out_dev[i], len[i] * d->outer * es, in_dev, bytes)) return "an output overlaps the input";
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(out_dev[i], len[i] * d->outer * es, out_dev[j], len[j] * d->outer * es)) return "two outputs overlap";
    }
    *row = total;
    return NULL;
}

// The one place that chooses the form (launch and name).  <env>=generic forces the literal form (A/B runs, tests); any other
// value means nothing -- the vector form is taken only where the arguments admit it; read per call.
static int slab_form(const char *env, int dtype, const void *whole, const void *const *part, const int64_t *len, int n)
{
    const char *force = getenv(env);
    if (force && strcmp(force, "generic") == 0) return SLAB_GENERIC;
    const int64_t es = dtype == SHL_MI355X_F16 ? 2 : 1;
    if (((uintptr_t)whole & 15) != 0) return SLAB_GENERIC;
    for (int i = 0; i < n; ++i) {
        if (len[i] == 0) continue;  // (concat only)
        // every length a multiple of 16 bytes: every offset and the row then are too
        if ((len[i] * es) % 16 != 0 || ((uintptr_t)part[i] & 15) != 0) return SLAB_GENERIC;
    }
    return SLAB_VEC;
}

// one operator call: its parts (pointer, length, int8 record each), the whole and its record
struct SlabJob {
    const char *op;
    bool gather;
    int dtype, form, n;
    int64_t outer, row;
    void *whole;
    void *const *part;
    const int64_t *len;
    const float *scale;
    const int32_t *zp;
    float s;
    int32_t z;
};

static int slab_launch(const SlabJob &j, hipStream_t s)
{
    if (j.outer == 0 || j.row == 0) return SHL_MI355X_OK;
    const bool f16 = j.dtype == SHL_MI355X_F16;
    const int64_t unit = j.form == SLAB_VEC ? (f16 ? 8 : 16) : 1;  // elements per column of the form
    // no launch has more workgroups than one over the whole row would: checked before anything is enqueued
    if (grid_refused(j.op, (j.row / unit * j.outer + 255) / 256)) return SHL_MI355X_ENOTSUP;
    void (*kernel)(SlabArgs);  // (a template-id with a comma cannot be a macro argument)
    if (j.form == SLAB_VEC) {
        if (j.gather) kernel = f16 ? slab_vec_kernel<true, true> : slab_vec_kernel<true, false>;
        else kernel = f16 ? slab_vec_kernel<false, true> : slab_vec_kernel<false, false>;
    } else {
        if (j.gather) kernel = f16 ? slab_generic_kernel<true, true> : slab_generic_kernel<true, false>;
        else kernel = f16 ? slab_generic_kernel<false, true> : slab_generic_kernel<false, false>;
    }
    int64_t base = 0;  // first column of the next launch, in elements
    int i = 0;
    while (i < j.n) {
        SlabArgs a;
        memset(&a, 0, sizeof(a));
        a.whole = static_cast<char *>(j.whole) + base * (f16 ? 2 : 1);
        a.row = j.row / unit;
        a.s = j.s, a.z = (float)j.z, a.inv_s = 1.0f / j.s;
        a.small = j.row * j.outer < (1ll << 32);  // (no overflow: *_invalid multiplied them)
        int64_t width = 0;
        int taken = 0;
        for (; i < j.n && taken < SLAB_MAX; ++i) {
            if (j.len[i] == 0) continue;  // (concat only: the reference's float loop skips it too)
            SlabPart &e = a.part[taken++];
            e.p = j.part[i], e.len = j.len[i] / unit, e.off = width / unit;
            if (!f16) {
                e.s = j.scale[i], e.z = (float)j.zp[i], e.inv_s = 1.0f / j.scale[i];
                const bool copy = j.form == SLAB_VEC;
                e.mode = (j.gather ? move_rec(j.scale[i], j.zp[i], j.s, j.z, copy) : move_rec(j.s, j.z, j.scale[i], j.zp[i], copy)).mode;
            }
            width += j.len[i];
        }
        for (int k = taken; k < SLAB_MAX; ++k) a.part[k] = a.part[0], a.part[k].off = INT64_MAX;
        base += width;
        if (taken == 0) break;  // only zero-length parts were left
        a.width = width / unit;
        a.items = a.width * j.outer;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((a.items + 255) / 256)), dim3(256), 0, s, a);
        SHL_HIP(hipGetLastError());
    }
    return SHL_MI355X_OK;
}

}  // namespace shl

extern "C" const char *shl_mi355x_concat_kernel_name(const void *const *in_dev, const int64_t *len, const float *in_scale,
                                                     const int32_t *in_zp, const void *out_dev,
                                                     const struct shl_mi355x_concat_desc *d)
{
    using namespace shl;
    int64_t row;
    if (concat_invalid(in_dev, len, in_scale, in_zp, out_dev, d, &row)) return "";
    return slab_form("SHL_MI355X_CONCAT_FORM", d->dtype, out_dev, in_dev, len, d->n_inputs) == SLAB_VEC ? "concat_vec" : "concat_generic";
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
    SlabJob j;
    j.op = "concat", j.gather = true, j.dtype = d->dtype, j.n = d->n_inputs, j.outer = d->outer, j.row = row;
    j.form = slab_form("SHL_MI355X_CONCAT_FORM", d->dtype, out_dev, in_dev, len, d->n_inputs);
    j.whole = out_dev, j.s = d->out_scale, j.z = d->out_zp;
    j.part = (void *const *)in_dev, j.len = len, j.scale = in_scale, j.zp = in_zp;  // (gather only reads the parts)
    return slab_launch(j, (hipStream_t)stream);
}

extern "C" const char *shl_mi355x_split_kernel_name(const void *in_dev, void *const *out_dev, const int64_t *len,
                                                    const float *out_scale, const int32_t *out_zp,
                                                    const struct shl_mi355x_split_desc *d)
{
    using namespace shl;
    int64_t row;
    if (split_invalid(in_dev, out_dev, len, out_scale, out_zp, d, &row)) return "";
    return slab_form("SHL_MI355X_SPLIT_FORM", d->dtype, in_dev, out_dev, len, d->n_outputs) == SLAB_VEC ? "split_vec" : "split_generic";
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
    SlabJob j;
    j.op = "split", j.gather = false, j.dtype = d->dtype, j.n = d->n_outputs, j.outer = d->outer, j.row = row;
    j.form = slab_form("SHL_MI355X_SPLIT_FORM", d->dtype, in_dev, out_dev, len, d->n_outputs);
    j.whole = const_cast<void *>(in_dev), j.s = d->in_scale, j.z = d->in_zp;  // (scatter only reads the whole)
    j.part = out_dev, j.len = len, j.scale = out_scale, j.zp = out_zp;
    return slab_launch(j, (hipStream_t)stream);
}

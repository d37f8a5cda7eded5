// attention_canon.h -- the host side of attention.hip: what is wrong with a descriptor, the two products as matmul descriptors,
// the rule that decides whether the fused kernel exists for a shape, and its LDS layout.  Pure host code that touches no device
// and includes no HIP header, so that a stand-alone program can compile it with the sanitizers (tests/test_attention_cpu.py).
#pragma once
#include <stdint.h>
#include <string.h>

#include "matmul_canon.h"

namespace shl {

constexpr int ATT_ROWS = 32;     // query rows per workgroup
constexpr int ATT_KEYS = 128;    // keys (Q K^T) / output columns (P V) per pass: 32 per wave
constexpr int ATT_TABLE_ABOVE = 256;  // int8 rows longer than this take the exponentials from a per-row table of 256

// Q K^T: a = q [batches][s][d], b = k [batches][t][d] read with swapped strides (trans_b), stored under the s record
static inline void att_qk_desc(const shl_mi355x_attention_desc *d, shl_mi355x_matmul_desc *m)
{
    memset(m, 0, sizeof(*m));
    m->dtype = d->dtype, m->batches = d->batches, m->m = d->s, m->n = d->t, m->k = d->d;
    m->a_batch_stride = (int64_t)d->s * d->d, m->a_row_stride = d->d, m->a_k_stride = 1;
    m->b_batch_stride = (int64_t)d->t * d->d, m->b_col_stride = d->d, m->b_k_stride = 1;
    m->a_elems = (int64_t)d->batches * d->s * d->d, m->b_elems = (int64_t)d->batches * d->t * d->d;
    m->out_elems = (int64_t)d->batches * d->s * d->t;
    m->a_scale = d->q_scale, m->a_zp = d->q_zp, m->b_scale = d->k_scale, m->b_zp = d->k_zp;
    m->out_scale = d->s_scale, m->out_zp = d->s_zp;
}

// P V: a = p [batches][s][t], b = v [batches][t][dv], no transposes, stored under the output's record
static inline void att_pv_desc(const shl_mi355x_attention_desc *d, shl_mi355x_matmul_desc *m)
{
    memset(m, 0, sizeof(*m));
    m->dtype = d->dtype, m->batches = d->batches, m->m = d->s, m->n = d->dv, m->k = d->t;
    m->a_batch_stride = (int64_t)d->s * d->t, m->a_row_stride = d->t, m->a_k_stride = 1;
    m->b_batch_stride = (int64_t)d->t * d->dv, m->b_col_stride = 1, m->b_k_stride = d->dv;
    m->a_elems = (int64_t)d->batches * d->s * d->t, m->b_elems = (int64_t)d->batches * d->t * d->dv;
    m->out_elems = (int64_t)d->batches * d->s * d->dv;
    m->a_scale = d->p_scale, m->a_zp = d->p_zp, m->b_scale = d->v_scale, m->b_zp = d->v_zp;
    m->out_scale = d->out_scale, m->out_zp = d->out_zp;
}

// NULL, or what is wrong with the descriptor alone (the part of att_validate that no pointer enters: the layout form, whose
// operands are no dense ranges, shares it)
static inline const char *att_desc_check(const shl_mi355x_attention_desc *d)
{
    if (d->dtype != SHL_MI355X_I8 && d->dtype != SHL_MI355X_F16) return "dtype is neither int8 nor binary16";
    if (d->batches < 1 || d->s < 1 || d->t < 1 || d->d < 1 || d->dv < 1) return "batches, s, t, d or dv below 1";
    if (d->t > SHL_MI355X_ATTENTION_MAX_KEYS) return "t exceeds SHL_MI355X_ATTENTION_MAX_KEYS";
    if (d->reserved0 != 0 || d->reserved[0] != 0 || d->reserved[1] != 0 || d->reserved[2] != 0 || d->reserved[3] != 0)
        return "a reserved field that is not zero";
    if ((d->has_scale != 0 && d->has_scale != 1) || (d->scale_is_first != 0 && d->scale_is_first != 1))
        return "has_scale or scale_is_first is neither 0 nor 1";
    if (d->has_scale && (d->dtype == SHL_MI355X_I8 ? (d->scale_raw < -128 || d->scale_raw > 127) : (d->scale_raw < 0 || d->scale_raw > 0xFFFF)))
        return "scale_raw is no element of the dtype";
    // (three factors below 2^31 each: the first product fits 64 bits, the second is taken only when the first is below 2^31)
    const int64_t lim = 0x7FFFFFFFll;
    const int64_t ext[5][2] = {{d->s, d->d}, {d->t, d->d}, {d->t, d->dv}, {d->s, d->dv}, {d->s, d->t}};
    for (int i = 0; i < 5; ++i) {
        const int64_t first = (int64_t)d->batches * ext[i][0];
        if (first > lim || first * ext[i][1] > lim) return "a tensor of 2^31 or more elements";
    }
    return NULL;
}

// NULL, or what is wrong with the call (SHL_MI355X_EINVAL).  Nothing is enqueued and no device is touched
static inline const char *att_validate(const void *q_dev, const void *k_dev, const void *v_dev, const void *out_dev,
                                       const shl_mi355x_attention_desc *d)
{
    if (!d || !q_dev || !k_dev || !v_dev || !out_dev) return "NULL argument";
    const char *why = att_desc_check(d);
    if (why) return why;
    // (att_desc_check: every count is below 2^31)
    const int64_t elems[4] = {(int64_t)d->batches * d->s * d->d, (int64_t)d->batches * d->t * d->d, (int64_t)d->batches * d->t * d->dv,
                              (int64_t)d->batches * d->s * d->dv};
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)(elems[3] * es);
    const uintptr_t in0[3] = {(uintptr_t)q_dev, (uintptr_t)k_dev, (uintptr_t)v_dev};
    if ((in0[0] | in0[1] | in0[2] | o0) & (uintptr_t)(es - 1)) return "a pointer that is not aligned to its elements";
    if (o1 < o0) return "a buffer that wraps around the address space";
    for (int i = 0; i < 3; ++i) {
        const uintptr_t i1 = in0[i] + (uintptr_t)(elems[i] * es);
        if (i1 < in0[i]) return "a buffer that wraps around the address space";
        if (in0[i] < o1 && o0 < i1) return "the output overlaps an operand";
    }
    return NULL;
}

// The fused kernel exists where shl_mi355x_matmul would run BOTH products in its mfma form: only against that form does the
// fused launch equal the unfused calls.  NULL, or why not (SHL_MI355X_ENOTSUP); for a descriptor att_validate has passed.
// (The form does not depend on the pointers: they decide the width of the loads only.)
// (What a session fuses WITHOUT being asked is narrower: att_default below.)
static inline const char *att_unsupported(const shl_mi355x_attention_desc *d)
{
    shl_mi355x_matmul_desc m;
    MmPlan p;
    att_qk_desc(d, &m);
    mm_plan(NULL, NULL, &m, &p);
    if (mm_form(&m, &p) != MM_MFMA) return "the matmul form rule gives Q K^T the chain form: the fused kernel equals the mfma form only";
    att_pv_desc(d, &m);
    mm_plan(NULL, NULL, &m, &p);
    if (mm_form(&m, &p) != MM_MFMA) return "the matmul form rule gives P V the chain form: the fused kernel equals the mfma form only";
    return NULL;
}

// The shape classes a session fuses by default: those where the fused launch was MEASURED faster than the four launches it
// replaces by more than the run-to-run spread (profiles/attention_notes.md; fused / unfused, int8 and binary16):
//   heads of 64 and more are excluded:  197 keys 1.19 / 1.13 (12 heads), 1.40 / 1.35 (3 heads), 1.01 / 1.01 at batch 8;
//                                        64 keys 1.38 / 1.39; 384 keys 1.39 / 1.39; 512 keys 1.47 / 1.35; 640 keys 1.33 / 1.39
//   heads of 32 on 850 keys are in:     0.81 / 0.87 (spread 0 - 2 %)
// Heads below 64 on fewer keys were not measured and stay out.  SHL_MI355X_ATTENTION=1 fuses every shape the kernel takes
constexpr int ATT_DEFAULT_MAX_D = 32;
constexpr int ATT_DEFAULT_MIN_KEYS = 768;

static inline bool att_default(const shl_mi355x_attention_desc *d) { return d->d <= ATT_DEFAULT_MAX_D && d->t >= ATT_DEFAULT_MIN_KEYS; }

// ---- the biased launch (shl_mi355x_attention_bias) ---------------------------------------------------------------------------
// the largest index the kernel forms in the bias, or -1 when it is 2^31 or more; for a descriptor whose strides are not negative
// and whose b_ext1 divides batches.  (A stride along an extent of 1 is never multiplied by anything but 0)
static inline int64_t att_bias_last(const shl_mi355x_attention_desc *d, const shl_mi355x_attention_bias_desc *b)
{
    const int64_t lim = 0x7FFFFFFFll;
    const int64_t ext[4] = {d->batches / b->b_ext1, b->b_ext1, d->s, d->t};
    const int64_t stride[4] = {b->b_stride[0], b->b_stride[1], b->row_stride, b->key_stride};
    int64_t last = 0;
    for (int i = 0; i < 4; ++i) {
        if (ext[i] == 1) continue;
        // (an extent below 2^31 times a stride below 2^31 fits 64 bits; so does the sum of four terms below 2^31)
        if (stride[i] > lim || (ext[i] - 1) * stride[i] > lim) return -1;
        last += (ext[i] - 1) * stride[i];
    }
    return last > lim ? -1 : last;
}

// NULL, or what is wrong with the bias and its descriptor, for a descriptor att_desc_check has passed; [*b0, *b1) the bytes the
// kernel reads of it.  (The layout form shares it)
static inline const char *att_bias_check(const void *bias_dev, const shl_mi355x_attention_desc *d, const shl_mi355x_attention_bias_desc *b,
                                         uintptr_t *b0, uintptr_t *b1)
{
    if (!bias_dev || !b) return "NULL argument";
    if (b->reserved[0] != 0 || b->reserved[1] != 0 || b->reserved[2] != 0 || b->reserved[3] != 0) return "a reserved field that is not zero";
    if (b->bias_is_first != 0 && b->bias_is_first != 1) return "bias_is_first is neither 0 nor 1";
    if (b->b_stride[0] < 0 || b->b_stride[1] < 0 || b->row_stride < 0 || b->key_stride < 0) return "a negative bias stride";
    if (b->b_ext1 < 1 || d->batches % b->b_ext1 != 0) return "b_ext1 is below 1 or does not divide batches";
    const int64_t last = att_bias_last(d, b);
    if (last < 0) return "a bias index of 2^31 or more";
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    *b0 = (uintptr_t)bias_dev, *b1 = *b0 + (uintptr_t)((last + 1) * es);
    if (*b0 & (uintptr_t)(es - 1)) return "a pointer that is not aligned to its elements";
    if (*b1 < *b0) return "a buffer that wraps around the address space";
    return NULL;
}

// NULL, or what is wrong with the call (SHL_MI355X_EINVAL): everything att_validate refuses, and the bias's own defects
static inline const char *att_bias_validate(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev,
                                            const void *out_dev, const shl_mi355x_attention_desc *d,
                                            const shl_mi355x_attention_bias_desc *b)
{
    const char *why = att_validate(q_dev, k_dev, v_dev, out_dev, d);
    if (why) return why;
    uintptr_t b0, b1;
    why = att_bias_check(bias_dev, d, b, &b0, &b1);
    if (why) return why;
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)((int64_t)d->batches * d->s * d->dv * es);  // (att_validate: below 2^31)
    if (b0 < o1 && o0 < b1) return "the output overlaps the bias";
    return NULL;
}

// The strides of the biased launch from the add's collapsed groups (eltwise.c:shl_mi355x_bcast_prepare: groups of neighbouring
// dims of the scores along which the bias varies or is broadcast, outermost first).  The groups are cut where they cross the
// borders of [batches][s][t]; pieces that continue each other (the outer one's stride is the inner one's times its extent) are
// one piece again.  The keys and the rows must come out as one piece each, the batches as at most two: i0 (outer) and i1.
// 0: done; 1: the groups are not those of [batches][s][t]; 2: a bias the four strides cannot express
static inline int att_bias_geometry(const shl_mi355x_mul_desc *m, int32_t batches, int32_t s, int32_t t, shl_mi355x_attention_bias_desc *b)
{
    if (!m || !b || m->ngroups < 1 || m->ngroups > 4 || batches < 1 || s < 1 || t < 1) return 1;
    int64_t count = 1;
    for (int g = 0; g < m->ngroups; ++g) {
        if (m->dim[g] < 1 || m->b_stride[g] < 0 || m->dim[g] > 0x7FFFFFFFll) return 1;
        count *= m->dim[g];
        if (count > 0x7FFFFFFFll) return 1;
    }
    if (count != (int64_t)batches * s * t) return 1;
    // pieces, innermost first: seg 0 the keys, 1 the rows, 2 the batches
    struct Piece {
        int seg;
        int64_t ext, stride;
    } piece[12];
    int np = 0;
    const int64_t seg_ext[3] = {t, s, batches};
    int g = m->ngroups - 1, seg = 0;
    int64_t grem = m->dim[g], gst = m->b_stride[g], srem = seg_ext[0];
    for (;;) {
        while (grem == 1 && g > 0) --g, grem = m->dim[g], gst = m->b_stride[g];
        while (srem == 1 && seg < 2) ++seg, srem = seg_ext[seg];
        if (grem == 1 || srem == 1) break;  // (the counts are equal: both are used up together)
        int64_t take;
        if (grem % srem == 0) take = srem;
        else if (srem % grem == 0) take = grem;
        else return 2;
        // a piece that continues the one before it joins it
        if (np > 0 && piece[np - 1].seg == seg && gst == piece[np - 1].stride * piece[np - 1].ext) piece[np - 1].ext *= take;
        else {
            if (np == 12) return 2;
            piece[np].seg = seg, piece[np].ext = take, piece[np].stride = gst, ++np;
        }
        grem /= take, srem /= take, gst *= take;
    }
    if (grem != 1 || srem != 1) return 1;
    int64_t stride[3][2] = {{0, 0}, {0, 0}, {0, 0}}, ext[3][2] = {{1, 1}, {1, 1}, {1, 1}};
    int n[3] = {0, 0, 0};
    for (int i = 0; i < np; ++i) {
        const int sg = piece[i].seg;
        if (n[sg] == (sg == 2 ? 2 : 1)) return 2;
        stride[sg][n[sg]] = piece[i].stride, ext[sg][n[sg]] = piece[i].ext, ++n[sg];
    }
    b->key_stride = stride[0][0], b->row_stride = stride[1][0];
    // one batch piece: all of the batch index is i1
    b->b_ext1 = (int32_t)(n[2] == 2 ? ext[2][0] : batches);
    b->b_stride[1] = stride[2][0], b->b_stride[0] = n[2] == 2 ? stride[2][1] : 0;
    return 0;
}

// The shape classes a session fuses by default when the chain carries a bias: those where the biased launch was MEASURED
// faster than the five launches it replaces, in int8 and in binary16, by more than the spread between windows on both sides
// (profiles/attention_bias_notes.md; fused / unfused, int8 and binary16; a workgroup is 32 query rows of one batch):
//   long rows on one round of the chip   heads of 32 on 850 keys, 216 workgroups: 0.82 / 0.93 -- but 1.64 / 1.84 on the 1728
//                                        workgroups of batch 8, which hold a CU each for their 850 keys' LDS
//   windows, many of them                heads of 32 on 49 keys, 3072 workgroups: 0.85 / 0.94 -- on 384 workgroups a tie
// Heads of 64 on 128 keys (384 workgroups: 0.91 / 0.95) and on 197 keys (672: 0.98 / 0.96) win too, but by little, and lose
// 17 to 38 % at batch 1 and on 384 keys: they stay behind the switch.  SHL_MI355X_ATTENTION=1 fuses every shape the kernel takes
constexpr int ATT_BIAS_LONG_MAX_GROUPS = 256;    // (the chip's CUs)
constexpr int ATT_BIAS_WINDOW_MAX_KEYS = 64;
constexpr int ATT_BIAS_WINDOW_MIN_GROUPS = 3072;

static inline bool att_bias_default(const shl_mi355x_attention_desc *d)
{
    const int64_t groups = (int64_t)d->batches * ((d->s + ATT_ROWS - 1) / ATT_ROWS);
    if (d->d > ATT_DEFAULT_MAX_D) return false;
    return (d->t >= ATT_DEFAULT_MIN_KEYS && groups <= ATT_BIAS_LONG_MAX_GROUPS) ||
           (d->t <= ATT_BIAS_WINDOW_MAX_KEYS && groups >= ATT_BIAS_WINDOW_MIN_GROUPS);
}

// 16-byte global loads stay aligned for every batch, row and piece of a dense [..][rows][inner] operand
static inline int att_vec(const void *p, int64_t inner, int64_t es) { return ((uintptr_t)p & 15) == 0 && (inner * es) % 16 == 0; }

// ---- the layout form (shl_mi355x_attention_layout): operands where the projections left them ---------------------------------
// ... and the layout form's rule: the operand's base (i0 * outer + i1 * head elements in), every row and every piece of it stay
// on the 16-byte grid.  ext: the extents {batches / heads, heads, rows} the three strides run along; a stride along an extent of
// 1 is never multiplied by anything but 0 and does not count (as for the validator)
static inline int att_vec_layout(const void *p, const int32_t stride[3], const int64_t ext[3], int64_t inner, int64_t es)
{
    if (!att_vec(p, inner, es)) return 0;
    for (int i = 0; i < 3; ++i)
        if (ext[i] > 1 && (stride[i] * es) % 16 != 0) return 0;
    return 1;
}

constexpr int ATT_MOVED_Q = 1, ATT_MOVED_K = 2, ATT_MOVED_V = 4, ATT_MOVED_OUT = 8;

// the four (extent, stride) pairs of an operand [batches / heads][heads][rows][inner]
struct AttView {
    int64_t ext[4], stride[4];
};

static inline AttView att_view(const shl_mi355x_attention_desc *d, int32_t heads, const int32_t stride[3], int32_t rows, int32_t inner)
{
    AttView v = {{d->batches / heads, heads, rows, inner}, {stride[0], stride[1], stride[2], 1}};
    return v;
}

// the largest index the kernel forms in the operand, or -1 when it is 2^31 or more; strides not negative.  (A stride along an
// extent of 1 is never multiplied by anything but 0; an extent and a stride below 2^31 each: the product fits 64 bits)
static inline int64_t att_view_last(const AttView &v)
{
    int64_t last = 0;
    for (int i = 0; i < 4; ++i)
        if (v.ext[i] > 1) last += (v.ext[i] - 1) * v.stride[i];
    return last > 0x7FFFFFFFll ? -1 : last;
}

// no two index tuples of the view name one element: the pairs sorted by stride, each stride at least the extent times the
// stride of the pair below it (the innermost at least 1).  Pairs of extent 1 are dropped; gaps are allowed
static inline bool att_view_injective(const AttView &v)
{
    int64_t e[4], s[4];
    int n = 0;
    for (int i = 0; i < 4; ++i) {
        if (v.ext[i] == 1) continue;
        int at = n++;
        for (; at > 0 && s[at - 1] > v.stride[i]; --at) e[at] = e[at - 1], s[at] = s[at - 1];
        e[at] = v.ext[i], s[at] = v.stride[i];
    }
    int64_t need = 1;
    for (int i = 0; i < n; ++i) {
        if (s[i] < need) return false;
        need = e[i] * s[i];  // (both below 2^31)
    }
    return true;
}

// NULL, or what is wrong with the layout call (SHL_MI355X_EINVAL): the descriptor's own defects as att_validate and
// att_bias_validate name them (bias_dev NULL: the launch without a bias, and bd is not looked at), then the layout's.  The
// operands' ranges are those of their strides, not of dense tensors.  Inputs may have any strides that are not negative -- 0,
// rows that overlap, q, k and v inside one packed projection --; the output's elements must be distinct and its range apart
// from every input's.  Nothing is enqueued and no device is touched
static inline const char *att_layout_validate(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev,
                                              const void *out_dev, const shl_mi355x_attention_desc *d,
                                              const shl_mi355x_attention_bias_desc *bd, const shl_mi355x_attention_layout_desc *l)
{
    if (!d || !l || !q_dev || !k_dev || !v_dev || !out_dev) return "NULL argument";
    const char *why = att_desc_check(d);
    if (why) return why;
    uintptr_t b0 = 0, b1 = 0;
    if (bias_dev || bd) {
        why = att_bias_check(bias_dev, d, bd, &b0, &b1);
        if (why) return why;
    }
    if (l->heads < 1 || d->batches % l->heads != 0) return "heads is below 1 or does not divide batches";
    if ((uint32_t)l->moved > 15u) return "moved bits beyond the four";
    if (l->reserved[0] != 0 || l->reserved[1] != 0) return "a reserved field that is not zero";
    const int32_t *const stride[4] = {l->q_stride, l->k_stride, l->v_stride, l->out_stride};
    for (int i = 0; i < 4; ++i)
        if (stride[i][0] < 0 || stride[i][1] < 0 || stride[i][2] < 0) return "a negative stride";
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    const int32_t rows[4] = {d->s, d->t, d->t, d->s}, inner[4] = {d->d, d->d, d->dv, d->dv};
    const uintptr_t p0[4] = {(uintptr_t)q_dev, (uintptr_t)k_dev, (uintptr_t)v_dev, (uintptr_t)out_dev};
    uintptr_t p1[4];
    if ((p0[0] | p0[1] | p0[2] | p0[3]) & (uintptr_t)(es - 1)) return "a pointer that is not aligned to its elements";
    for (int i = 0; i < 4; ++i) {
        const AttView v = att_view(d, l->heads, stride[i], rows[i], inner[i]);
        const int64_t last = att_view_last(v);
        if (last < 0) return "an operand index of 2^31 or more";
        p1[i] = p0[i] + (uintptr_t)((last + 1) * es);
        if (p1[i] < p0[i]) return "a buffer that wraps around the address space";
        if (i == 3 && !att_view_injective(v)) return "output elements that overlap each other";
    }
    for (int i = 0; i < 3; ++i)
        if (p0[i] < p1[3] && p0[3] < p1[i]) return "the output overlaps an operand";
    if (bias_dev && b0 < p1[3] && p0[3] < b1) return "the output overlaps the bias";
    return NULL;
}

// The strides of a [batches][rows][cols] view over a dense source, as a chain of movers would have copied it: the source's dims,
// then steps in order -- a reshape (its target dims) or, at most once, a transpose (perm: output dim k is input dim perm[k]) --
// and, swap_last2, the last two dims exchanged once more (a K that reaches Q K^T as [..][d][t], read without trans_b).  The last
// two dims of the result are the rows and the columns, the product of the others is the batches; their pieces that continue each
// other are one piece, and at most two may remain: heads is the inner one's extent.  For the OUTPUT the same function is called
// on the destination: its dims, the chain behind the core inverted, give where the core's [batches][s][dv] lands.
// 0: done; 1: arguments that describe no view (counts that differ, no permutation, a second transpose, rank below 2 or above
// SHL_MI355X_MAX_DIM); 2: a view the three strides cannot express (inner stride other than 1, rows or columns in more than one
// piece, batch dims in more than two, a reshape whose dims divide neither way into the dims it regroups, an index of 2^31 or more)
struct AttViewStep {
    int32_t is_transpose, rank;
    int32_t v[SHL_MI355X_MAX_DIM];  // the reshape's target dims / the permutation
};

static inline int att_layout_strides(const int32_t *src_dim, int32_t src_rank, const AttViewStep *step, int32_t nsteps, int32_t swap_last2,
                                     int32_t *batches, int32_t *rows, int32_t *cols, int32_t *heads, int32_t stride[3])
{
    constexpr int R = SHL_MI355X_MAX_DIM, A = 4 * SHL_MI355X_MAX_DIM;
    if (!src_dim || (nsteps > 0 && !step) || nsteps < 0 || !batches || !rows || !cols || !heads || !stride) return 1;
    if (src_rank < 1 || src_rank > R) return 1;
    // The view as atoms -- (extent, stride) pairs, outermost first, none of extent 1 -- and the dims as runs of atoms: a reshape
    // regroups the atoms (splitting one where a new dim ends inside it), a transpose permutes the runs.  A dim made of atoms that
    // do not continue each other (the merged [B H] behind a transpose) is what the movers would have copied, and still a view
    int64_t ae[A], as[A], count = 1;
    int na = 0, rank = src_rank, len[R];  // len: the atoms of each dim
    for (int i = 0; i < rank; ++i) {
        if (src_dim[i] < 1) return 1;
        count *= src_dim[i];
        if (count > 0x7FFFFFFFll) return 2;
    }
    for (int64_t i = 0, run = count; i < rank; ++i) {
        run /= src_dim[i];
        len[i] = src_dim[i] > 1 ? 1 : 0;
        if (src_dim[i] > 1) ae[na] = src_dim[i], as[na] = run, ++na;
    }
    int transposes = 0;
    for (int n = 0; n < nsteps; ++n) {
        const AttViewStep &s = step[n];
        if (s.rank < 1 || s.rank > R) return 1;
        int64_t ne[A], ns[A];
        int nn = 0, nlen[R];
        if (s.is_transpose) {
            if (++transposes > 1 || s.rank != rank) return 1;
            uint32_t seen = 0;
            int first[R];
            for (int i = 0, at = 0; i < rank; ++i) first[i] = at, at += len[i];
            for (int i = 0; i < rank; ++i) {
                if (s.v[i] < 0 || s.v[i] >= rank || (seen >> s.v[i] & 1u)) return 1;
                seen |= 1u << s.v[i];
                nlen[i] = len[s.v[i]];
                for (int k = 0; k < nlen[i]; ++k) ne[nn] = ae[first[s.v[i]] + k], ns[nn] = as[first[s.v[i]] + k], ++nn;
            }
        } else {
            int64_t c = 1;
            for (int i = 0; i < s.rank; ++i) {
                if (s.v[i] < 1) return 1;
                c *= s.v[i];
                if (c > 0x7FFFFFFFll) return 1;
            }
            if (c != count) return 1;
            int at = 0;
            int64_t e = 1, st = 0;  // what is left of the atom under the cursor
            for (int i = 0; i < s.rank; ++i) {
                int64_t need = s.v[i];
                nlen[i] = 0;
                while (need > 1) {
                    if (e == 1) e = ae[at], st = as[at], ++at;  // (the counts are equal: an atom is left)
                    if (nn == A) return 2;
                    if (need % e == 0) ne[nn] = e, ns[nn] = st, need /= e, e = 1;
                    else if (e % need == 0) e /= need, ne[nn] = need, ns[nn] = st * e, need = 1;  // the atom's outer part
                    else return 2;
                    ++nn, ++nlen[i];
                }
            }
        }
        rank = s.rank, na = nn;
        for (int i = 0; i < rank; ++i) len[i] = nlen[i];
        for (int i = 0; i < na; ++i) ae[i] = ne[i], as[i] = ns[i];
    }
    if (rank < 2) return 1;
    // the rows' and the columns' atoms, swapped where the consumer reads the last two dims the other way round
    int first[R + 1];
    first[0] = 0;
    for (int i = 0; i < rank; ++i) first[i + 1] = first[i] + len[i];
    const int dr = swap_last2 ? rank - 1 : rank - 2, dc = swap_last2 ? rank - 2 : rank - 1;
    // a dim is one piece when its atoms continue each other
    int64_t ext2[2] = {1, 1}, st2[2] = {0, 0};
    const int dd[2] = {dr, dc};
    for (int w = 0; w < 2; ++w)
        for (int k = first[dd[w]]; k < first[dd[w] + 1]; ++k) {
            if (k > first[dd[w]] && as[k - 1] != ae[k] * as[k]) return 2;
            ext2[w] *= ae[k], st2[w] = as[k];
        }
    if (ext2[1] != 1 && st2[1] != 1) return 2;
    // the batch dims' pieces, outermost first
    int64_t pe[A], ps[A];
    int np = 0;
    for (int k = 0; k < first[rank - 2]; ++k) {
        if (np > 0 && ps[np - 1] == ae[k] * as[k]) pe[np - 1] *= ae[k], ps[np - 1] = as[k];
        else pe[np] = ae[k], ps[np] = as[k], ++np;
    }
    if (np > 2) return 2;
    int64_t last = 0, b = 1;
    for (int k = 0; k < na; ++k) last += (ae[k] - 1) * as[k];
    for (int k = 0; k < first[rank - 2]; ++k) b *= ae[k];
    if (last > 0x7FFFFFFFll) return 2;
    *batches = (int32_t)b, *rows = (int32_t)ext2[0], *cols = (int32_t)ext2[1];
    *heads = (int32_t)(np == 0 ? 1 : pe[np - 1]);
    stride[0] = (int32_t)(np == 2 ? ps[0] : 0), stride[1] = (int32_t)(np >= 1 ? ps[np - 1] : 0);
    stride[2] = (int32_t)st2[0];
    return 0;
}

// The classes a session folds the head moves of WITHOUT being asked: those where one layout launch was MEASURED faster than the
// mover launches plus the core it replaces, in int8 and in binary16, by more than the spread between windows on both sides
// (the project's standing rule; tools/attention_layout_bench.py is the method, profiles/attention_layout_notes.md the record).
// A is the eight movers plus the core by the dense forms' own default rules; layout / A, int8 and binary16, with and without a bias:
//   short rows, heads of 32 to 64     49 keys (d 32) 0.67 / 0.69 and 0.88 / 0.86 at batch 8; 64 keys 0.74 / 0.76; 128 keys
//                                     0.77 / 0.86 and 0.66 / 0.71; 197 keys 0.78 / 0.79, 0.87 / 0.95 (3 heads), 0.80 / 0.84
//                                     and 0.63 / 0.67 at batch 8
//   long rows on one round of the chip   heads of 32 on 850 keys, 216 workgroups: 0.82 / 0.89, with a mask 0.84 / 0.93
// Heads of 64 on 384 keys win by too little in binary16 (0.87 / 0.98) and lose there on 512 and 640 keys (0.98 / 1.03,
// 0.94 / 1.13): they stay out, and so does what was not measured: fewer than 49 keys, 198 to 383 keys, heads below 32 on
// short rows, a dv other than d, long rows on more than 256 workgroups.  The short class is bounded by the extremes of the
// measured rows (49 and 197 keys, heads of 32 and 64, dv = d, grids from 21 workgroups on -- smaller grids were not measured,
// larger ones than the 3072 measured only add rounds of the chip); between them it interpolates over 64 and 128 keys.  The spread
// between windows was below 1 % on every row
constexpr int ATT_LAYOUT_SHORT_MIN_KEYS = 49;
constexpr int ATT_LAYOUT_SHORT_MAX_KEYS = 197;
constexpr int ATT_LAYOUT_SHORT_MIN_D = 32;
constexpr int ATT_LAYOUT_SHORT_MAX_D = 64;
constexpr int ATT_LAYOUT_SHORT_MIN_GROUPS = 21;  // (DeiT-tiny at batch 1, the smallest grid measured: 3 heads x 7 row tiles)

static inline bool att_layout_default(const shl_mi355x_attention_desc *d, const shl_mi355x_attention_layout_desc *)
{
    const int64_t groups = (int64_t)d->batches * ((d->s + ATT_ROWS - 1) / ATT_ROWS);
    if (d->dv != d->d) return false;
    return (d->t >= ATT_LAYOUT_SHORT_MIN_KEYS && d->t <= ATT_LAYOUT_SHORT_MAX_KEYS && d->d >= ATT_LAYOUT_SHORT_MIN_D &&
            d->d <= ATT_LAYOUT_SHORT_MAX_D && groups >= ATT_LAYOUT_SHORT_MIN_GROUPS) ||
           (d->d <= ATT_DEFAULT_MAX_D && d->t >= ATT_DEFAULT_MIN_KEYS && groups <= ATT_BIAS_LONG_MAX_GROUPS);
}

// the LDS image, in bytes from the start: e rows | exponential tables (int8) | score tile | q slab | k / v slab | row sums |
// requantised tables (int8), the rows and tables one per wave.  Every offset is a multiple of 16
struct AttLds {
    int32_t tile_pitch;  // bytes per row of the 32 x t score tile: whole 64-byte slabs of k + 16 (the 32 rows of a fragment read
                         // fall on different banks)
    int32_t e, lut_e, tile, slab_q, slab_kv, row_sum, lut_q, bytes;
};

static inline AttLds att_lds(const shl_mi355x_attention_desc *d, int waves)
{
    const int32_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1, i8 = d->dtype == SHL_MI355X_I8;
    AttLds l;
    l.tile_pitch = (d->t * es + 63) / 64 * 64 + 16;
    int32_t at = 0;
    l.e = at, at += waves * (d->t + 256) * 8;
    l.lut_e = at, at += i8 ? waves * 256 * 8 : 0;
    l.tile = at, at += ATT_ROWS * l.tile_pitch;
    l.slab_q = at, at += ATT_ROWS * 80;
    l.slab_kv = at, at += ATT_KEYS * 80;
    l.row_sum = at, at += 4 * 32 * 4;
    l.lut_q = at, at += i8 ? waves * 256 : 0;
    l.bytes = at;
    return l;
}

// The waves of a workgroup: four run the products, and all of them the softmax, a row each at a time.  The softmax's f64 work
// (exp, the running sum, the quotient) is a chain per row, so a grid that leaves the chip's SIMDs idle -- batch 1: 84 workgroups
// for ViT-B's 12 heads on 256 CUs -- brings more waves per workgroup: as many of 16, 8, 4 as keep the whole grid at or under four
// waves per SIMD (256 CUs x 16) and fit the LDS (an e row and, int8, two tables per wave)
constexpr int ATT_LDS_BYTES = 160 * 1024;
constexpr int64_t ATT_CHIP_WAVES = 256 * 16;

static inline int att_waves(const shl_mi355x_attention_desc *d)
{
    const int64_t groups = (int64_t)d->batches * ((d->s + ATT_ROWS - 1) / ATT_ROWS);
    for (int waves = 16; waves > 4; waves /= 2)
        if (groups * waves <= ATT_CHIP_WAVES && att_lds(d, waves).bytes <= ATT_LDS_BYTES) return waves;
    return 4;
}

}  // namespace shl

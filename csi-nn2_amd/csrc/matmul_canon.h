// matmul_canon.h -- the host side of matmul.hip: what is wrong with a descriptor, the plan-time proof that the int8 mfma form
// equals the reference's chain, and the form rule.  Pure host code that touches no device and includes no HIP header, so that a
// stand-alone program can compile it with the sanitizers (tests/test_matmul_cpu.py).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "fma_div_ok.h"
#include "shl_mi355x.h"

namespace shl {

enum { MM_CHAIN = 0, MM_MFMA = 1 };

// the default rule's threshold (profiles/matmul_notes.md): the mfma form pays about 5 us for its first slab whatever the
// shape, the chain one dependent multiply-add per k.  Measured: the chain wins P V at S = 49 (K = 49: 4.0 against 6.3 us) and
// loses everywhere from K = 64 on, M = 1 included (K = 768: 25 against 10 us).  So the chain runs problems of less than one
// slab of k whose outputs fit the chip's lanes in one go (256 CUs x 256 lanes); past that its time grows with the output
// count as well
constexpr int MM_CHAIN_BELOW_K = 64;
constexpr int64_t MM_CHAIN_MAX_OUTPUTS = 65536;

// what the launch needs beyond the descriptor
struct MmPlan {
    int a_kcontig, b_kcontig;  // the operand's k stride is 1 (else its row / column stride is)
    int a_vec, b_vec;          // 16-byte global loads stay aligned for every batch, row and piece
    int mfma_fits;
};

// NULL, or what is wrong with the call.  Nothing is enqueued and no device is touched
static inline const char *mm_validate(const void *a_dev, const void *b_dev, const void *out_dev, const shl_mi355x_matmul_desc *d)
{
    if (!d || !a_dev || !b_dev || !out_dev) return "NULL argument";
    if (d->dtype != SHL_MI355X_I8 && d->dtype != SHL_MI355X_F16) return "dtype is neither int8 nor binary16";
    if (d->batches < 1 || d->m < 1 || d->n < 1 || d->k < 1) return "batches, m, n or k below 1";
    if (d->a_elems < 1 || d->b_elems < 1 || d->out_elems < 1) return "a tensor without elements";
    if (d->a_elems > 0x7FFFFFFFll || d->b_elems > 0x7FFFFFFFll || d->out_elems > 0x7FFFFFFFll) return "a tensor of 2^31 or more elements";
    if (d->a_batch_stride < 0 || d->a_row_stride < 0 || d->a_k_stride < 0 || d->b_batch_stride < 0 || d->b_col_stride < 0 ||
        d->b_k_stride < 0)
        return "a negative stride";
    // (three factors below 2^31: the first product fits 64 bits, the second is taken only when the first is below 2^31)
    const int64_t bm = (int64_t)d->batches * d->m;
    if (bm > 0x7FFFFFFFll || bm * d->n != d->out_elems) return "the output tensor does not hold batches x m x n elements";
    const int64_t lim = 0x7FFFFFFFll;  // a stride at or past it reaches past any admissible tensor unless its extent is 1
    const int64_t ext[6] = {d->batches, d->m, d->k, d->batches, d->n, d->k};
    const int64_t str[6] = {d->a_batch_stride, d->a_row_stride, d->a_k_stride, d->b_batch_stride, d->b_col_stride, d->b_k_stride};
    for (int side = 0; side < 2; ++side) {
        const int64_t elems = side == 0 ? d->a_elems : d->b_elems;
        int64_t reach = 0;
        for (int j = 0; j < 3; ++j) {
            const int64_t e = ext[3 * side + j], s = str[3 * side + j];
            if (e > 1 && s > lim) return side == 0 ? "an index reaches past the first operand" : "an index reaches past the second operand";
            reach += (e - 1) * s;  // (below 2^62 per term)
        }
        if (reach >= elems) return side == 0 ? "an index reaches past the first operand" : "an index reaches past the second operand";
    }
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    const uintptr_t a0 = (uintptr_t)a_dev, a1 = a0 + (uintptr_t)(d->a_elems * es), b0 = (uintptr_t)b_dev, b1 = b0 + (uintptr_t)(d->b_elems * es);
    const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)(d->out_elems * es);
    if ((a0 | b0 | o0) & (uintptr_t)(es - 1)) return "a pointer that is not aligned to its elements";
    if (a1 < a0 || b1 < b0 || o1 < o0) return "a buffer that wraps around the address space";
    if ((a0 < o1 && o0 < a1) || (b0 < o1 && o0 < b1)) return "the output overlaps an operand";
    return NULL;
}

// the bias of shl_mi355x_matmul_bias, for a descriptor mm_validate has passed: n elements of the descriptor's dtype
static inline const char *mm_validate_bias(const void *bias_dev, const void *out_dev, const shl_mi355x_matmul_desc *d)
{
    if (!bias_dev) return "NULL argument";
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    const uintptr_t c0 = (uintptr_t)bias_dev, c1 = c0 + (uintptr_t)(d->n * es), o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)(d->out_elems * es);
    if (c0 & (uintptr_t)(es - 1)) return "a pointer that is not aligned to its elements";
    if (c1 < c0) return "a buffer that wraps around the address space";
    if (c0 < o1 && o0 < c1) return "the output overlaps the bias";
    return NULL;
}

// a float32 scale as m 2^e with m odd: false for zero, NaN and infinities
static inline bool mm_odd_mantissa(float s, int64_t *m, int *e)
{
    if (!(fabsf(s) > 0.0f) || isinf(s)) return false;
    int ex;
    const double f = frexp(fabs((double)s), &ex);  // s = f 2^ex, 0.5 <= f < 1: f 2^24 is an integer for a normal float32
    int64_t mm = (int64_t)ldexp(f, 53);            // (also for a subnormal one: at most 53 bits either way)
    ex -= 53;
    while ((mm & 1) == 0) mm >>= 1, ++ex;
    *m = mm, *e = ex;
    return true;
}

// the proof of DESIGN: k Aa Ab ma mb < 2^24 and exponents far from under- and overflow
static inline bool mm_is_exact(const shl_mi355x_matmul_desc *d)
{
    if (!d || d->dtype != SHL_MI355X_I8 || d->k < 1) return false;
    if (d->a_zp < -128 || d->a_zp > 127 || d->b_zp < -128 || d->b_zp > 127) return false;
    int64_t ma, mb;
    int ea, eb;
    if (!mm_odd_mantissa(d->a_scale, &ma, &ea) || !mm_odd_mantissa(d->b_scale, &mb, &eb)) return false;
    if (ea < -120 || eb < -120 || ea + eb < -120 || ea > 60 || eb > 60 || ea + eb > 60) return false;
    const int64_t aa = d->a_zp + 128 > 127 - d->a_zp ? d->a_zp + 128 : 127 - d->a_zp;
    const int64_t ab = d->b_zp + 128 > 127 - d->b_zp ? d->b_zp + 128 : 127 - d->b_zp;
    const int64_t cap = (int64_t)1 << 24;
    int64_t p = (int64_t)d->k;  // every factor is at least 1: the product only grows, so it is cut off once it reaches the cap
    const int64_t f[4] = {aa, ab, ma, mb};
    for (int j = 0; j < 4; ++j) {
        if (f[j] >= cap || p >= cap) return false;
        p *= f[j];  // (both below 2^24)
    }
    return p < cap;
}

// div_by_scale(f, so, RN(1 / so)) == f / so for every f the int8 forms can end with (common.h: 2^-40 <= so <= 2^40,
// |f| <= 2^60, f finite): |f| is at most k 255 255 |sa sb|, with a factor of two for the chain's roundings
static inline bool mm_fma_ok(const shl_mi355x_matmul_desc *d)
{
    return fma_div_ok(2.0 * (double)d->k * 65025.0 * fabs((double)d->a_scale) * fabs((double)d->b_scale), d->out_scale);
}

static inline void mm_plan(const void *a_dev, const void *b_dev, const shl_mi355x_matmul_desc *d, MmPlan *p)
{
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    memset(p, 0, sizeof(*p));
    p->a_kcontig = d->a_k_stride == 1 || d->k == 1;
    p->b_kcontig = d->b_k_stride == 1 || d->k == 1;
    const bool a_unit = p->a_kcontig || d->a_row_stride == 1 || d->m == 1;
    const bool b_unit = p->b_kcontig || d->b_col_stride == 1 || d->n == 1;
    // the stride that is NOT walked by a 16-byte piece, and the batch stride, must keep every piece on the 16-byte grid
    const int64_t a_other = p->a_kcontig ? (d->m == 1 ? 0 : d->a_row_stride) : (d->k == 1 ? 0 : d->a_k_stride);
    const int64_t b_other = p->b_kcontig ? (d->n == 1 ? 0 : d->b_col_stride) : (d->k == 1 ? 0 : d->b_k_stride);
    const int64_t a_batch = d->batches == 1 ? 0 : d->a_batch_stride, b_batch = d->batches == 1 ? 0 : d->b_batch_stride;
    p->a_vec = ((uintptr_t)a_dev & 15) == 0 && (a_other * es) % 16 == 0 && (a_batch * es) % 16 == 0;
    p->b_vec = ((uintptr_t)b_dev & 15) == 0 && (b_other * es) % 16 == 0 && (b_batch * es) % 16 == 0;
    p->mfma_fits = a_unit && b_unit && (d->dtype == SHL_MI355X_F16 || d->k <= SHL_MI355X_MATMUL_MFMA_MAX_K);
    if (d->dtype == SHL_MI355X_I8 && (d->a_zp < -128 || d->a_zp > 127 || d->b_zp < -128 || d->b_zp > 127)) p->mfma_fits = 0;
}

// The one place that chooses the form (launch and name).  SHL_MI355X_MATMUL_FORM=chain|mfma forces one; read per call
static inline int mm_form(const shl_mi355x_matmul_desc *d, const MmPlan *p)
{
    const char *force = getenv("SHL_MI355X_MATMUL_FORM");
    if (force && strcmp(force, "chain") == 0) return MM_CHAIN;
    if (!p->mfma_fits) return MM_CHAIN;
    if (force && strcmp(force, "mfma") == 0) return MM_MFMA;
    return d->k < MM_CHAIN_BELOW_K && d->out_elems <= MM_CHAIN_MAX_OUTPUTS ? MM_CHAIN : MM_MFMA;
}

static inline const char *mm_form_name(int form) { return form == MM_MFMA ? SHL_MI355X_MATMUL_MFMA : SHL_MI355X_MATMUL_CHAIN; }

}  // namespace shl

// reduce_canon.h -- the host side of reduce.hip: what is wrong with a descriptor, its canonical form, the form rule and the
// rows form's plan.  Pure host code that touches no device and includes no HIP header, so that a stand-alone program can
// compile it with the sanitizers (tests/test_reduce_cpu.py).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "fma_div_ok.h"
#include "shl_mi355x.h"

namespace shl {

enum { RD_ROWS = 0, RD_COLS = 1, RD_GENERIC = 2 };

constexpr int RD_G = SHL_MI355X_REDUCE_GROUPS;

// the layer after canonicalisation: groups with their extents and input strides in elements, the outermost first
struct RdCanon {
    int n_out, n_in;
    int64_t oext[SHL_MI355X_MAX_DIM], ostr[SHL_MI355X_MAX_DIM], iext[SHL_MI355X_MAX_DIM], istr[SHL_MI355X_MAX_DIM];
    int64_t out_count, inner_size;
};

// one list: extent-1 groups dropped, a group merged into the one before it when that one's stride is this one's extent times
// its stride (the pair then is one run of the mixed-radix index).  Returns the count
static inline int rd_canon_list(int n, const int32_t *ext, const int32_t *str, int64_t *cext, int64_t *cstr)
{
    int m = 0;
    for (int k = 0; k < n; ++k) {
        if (ext[k] == 1) continue;
        if (m > 0 && cstr[m - 1] == (int64_t)ext[k] * str[k]) {
            cext[m - 1] *= ext[k], cstr[m - 1] = str[k];
            continue;
        }
        cext[m] = ext[k], cstr[m] = str[k], ++m;
    }
    return m;
}

// NULL and the canonical layer, or what is wrong with the call.  Nothing is enqueued and no device is touched
static inline const char *rd_canonicalise(const void *in_dev, const void *out_dev, const shl_mi355x_reduce_desc *d, RdCanon *c)
{
    if (!d || !in_dev || !out_dev) return "NULL argument";
    if (d->dtype != SHL_MI355X_I8 && d->dtype != SHL_MI355X_F16) return "dtype is neither int8 nor binary16";
    if (d->kind < SHL_MI355X_REDUCE_SUM || d->kind > SHL_MI355X_REDUCE_MIN) return "kind is none of sum, mean, max, min";
    if (d->init != SHL_MI355X_REDUCE_INIT_FLT_MAX && d->init != SHL_MI355X_REDUCE_INIT_FIRST) return "unknown initial-value rule";
    if (d->n_out < 0 || d->n_out > SHL_MI355X_MAX_DIM || d->n_inner < 0 || d->n_inner > SHL_MI355X_MAX_DIM) return "group count outside 0 .. 8";
    if (d->in_elems < 1) return "the input has no elements";
    if (d->in_elems > 0x7FFFFFFFll) return "the input has 2^31 or more elements";
    int64_t outs = 1, inner = 1, reach = 0;  // reach: the largest index, held at in_elems once it is past the input
    for (int k = 0; k < d->n_out; ++k) {
        if (d->out_extent[k] < 0 || d->out_stride[k] < 0) return "a negative outer extent or stride";
        outs *= d->out_extent[k];  // (below 2^31 before this step: no overflow)
        if (outs > 0x7FFFFFFFll) return "2^31 or more outputs";
        if (d->out_extent[k] > 0) reach += (int64_t)(d->out_extent[k] - 1) * d->out_stride[k];  // (below 2^62 per term)
        if (reach > d->in_elems) reach = d->in_elems;
    }
    for (int k = 0; k < d->n_inner; ++k) {
        if (d->inner_extent[k] < 1 || d->inner_stride[k] < 0) return "an inner extent below 1 or a negative stride";
        inner *= d->inner_extent[k];
        if (inner > 0x7FFFFFFFll) return "2^31 or more elements per output";
        reach += (int64_t)(d->inner_extent[k] - 1) * d->inner_stride[k];
        if (reach > d->in_elems) reach = d->in_elems;
    }
    memset(c, 0, sizeof(*c));
    c->out_count = outs, c->inner_size = inner;
    if (outs > 0 && reach >= d->in_elems) return "an index reaches past the input";
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    const uintptr_t i0 = (uintptr_t)in_dev, i1 = i0 + (uintptr_t)(d->in_elems * es), o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)(outs * es);
    if ((i0 | o0) & (uintptr_t)(es - 1)) return "a pointer that is not aligned to its elements";
    if (i1 < i0 || o1 < o0) return "a buffer that wraps around the address space";
    if (o0 < o1 && i0 < o1 && o0 < i1) return "the output overlaps the input";
    c->n_out = outs == 0 ? 0 : rd_canon_list(d->n_out, d->out_extent, d->out_stride, c->oext, c->ostr);
    c->n_in = rd_canon_list(d->n_inner, d->inner_extent, d->inner_stride, c->iext, c->istr);
    if (c->n_out > RD_G || c->n_in > RD_G) return "more than 4 groups remain on one side after canonicalisation";
    return NULL;
}

// The one place that chooses the form (launch and name).  SHL_MI355X_REDUCE_FORM=generic forces the literal form; read per
// call
static inline int rd_form(const RdCanon *c)
{
    const char *force = getenv("SHL_MI355X_REDUCE_FORM");
    if (force && strcmp(force, "generic") == 0) return RD_GENERIC;
    if (c->n_in > 0 && c->istr[c->n_in - 1] == 1) return RD_ROWS;
    if (c->n_out > 0 && c->ostr[c->n_out - 1] == 1) return RD_COLS;
    return RD_GENERIC;
}

static inline const char *rd_form_name(int form)
{
    return form == RD_ROWS ? SHL_MI355X_REDUCE_ROWS : form == RD_COLS ? SHL_MI355X_REDUCE_COLS : SHL_MI355X_REDUCE_GENERIC;
}

// the rows form: a run is the innermost inner group; a window of np 16-byte pieces on the 16-byte grid holds it from its
// first byte's offset on that grid (up to 15) on, in `passes` windows
struct RdRows {
    int32_t run, segs, np, rows, passes;
};

static inline void rd_rows_plan(const RdCanon *c, int64_t es, RdRows *r)
{
    const int64_t run = c->iext[c->n_in - 1], span = 15 + run * es;  // bytes from the grid point below the run to its end
    int np = 1;
    while (np < SHL_MI355X_REDUCE_CHUNK_BYTES / 16 && (int64_t)np * 16 < span) np *= 2;
    r->run = (int32_t)run, r->segs = (int32_t)(c->inner_size / run);
    r->np = np, r->rows = np == 16 ? 64 : np == 8 ? 128 : 256;
    r->passes = (int32_t)((span + (int64_t)np * 16 - 1) / ((int64_t)np * 16));
}

// div_by_scale(x, so, RN(1 / so)) == x / so for every x the chain can end with (common.h; the range
// conv_plan.hip:fma_division_ok admits: 2^-40 <= so <= 2^40, |x| <= 2^60, x finite): |x| is at most inner_size times the
// largest element, with a factor of two for the chain's roundings
static inline bool reduce_fma_ok(const shl_mi355x_reduce_desc *d, const RdCanon *c)
{
    return fma_div_ok(2.0 * (double)c->inner_size * (128.0 + fabs((double)d->in_zp)) * fabs((double)d->in_scale), d->out_scale);
}

}  // namespace shl

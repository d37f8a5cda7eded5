/*
 * attention.c -- the core of an attention block as one launch, for session.c: the chain matmul(q, k, trans_b) -> [mul by a
 * one-element constant] -> softmax over the last axis -> matmul(p, v) as ONE descriptor of include/shl_mi355x.h
 * (shl_mi355x_attention).  No operator of its own: the four layers keep their callbacks, and a session whose planner does not
 * merge them runs them as before.
 */
#include <string.h>

#include "mi355x_internal.h"

/* a tensor the fused kernel can stand for: the chain's dtype, one quantisation record, 2 .. MAX_DIM dims of at least 1 */
static int plain(const struct csinn_tensor *t, int dtype)
{
    if (t == NULL || shl_mi355x_dtype_code(t) != dtype || t->qinfo == NULL || t->quant_channel > 1) return 0;
    if (t->dim_count < 2 || t->dim_count > MAX_DIM) return 0;
    if (dtype == SHL_MI355X_F16 && t->qinfo->scale != 1.0f) return 0;
    for (int i = 0; i < t->dim_count; i++)
        if (t->dim[i] < 1) return 0;
    return 1;
}

/* [batches][rows][cols] of a tensor whose leading dims are one batch count; 0 when it has another shape */
static int is_shape(const struct csinn_tensor *t, int64_t batches, int32_t rows, int32_t cols)
{
    int64_t b = 1;
    for (int i = 0; i < t->dim_count - 2; i++) b *= t->dim[i]; /* (each below 2^31, at most MAX_DIM of them: no overflow of note) */
    return b == batches && t->dim[t->dim_count - 2] == rows && t->dim[t->dim_count - 1] == cols;
}

/* The chain as a descriptor.  s: the scores q k^T stores; c / sc: the constant and the scaled scores, both NULL without the
 * multiply; const_first: the constant is the mul layer's first input; p: the softmax's output, axis its params' axis.
 * CSINN_TRUE when shl_mi355x_attention takes the chain (asked with made-up addresses that do not overlap) and -- unless `force` --
 * the shape is one a session fuses by default; CSINN_FALSE -- without a message: the planner only asks -- when the layers then
 * run one by one */
int shl_mi355x_attention_prepare(struct csinn_tensor *q, struct csinn_tensor *k, struct csinn_tensor *s,
                                 struct csinn_matmul_params *qk_params, struct csinn_tensor *c, struct csinn_tensor *sc,
                                 int const_first, struct csinn_tensor *p, int axis, struct csinn_tensor *v,
                                 struct csinn_tensor *out, struct csinn_matmul_params *pv_params, int force,
                                 struct shl_mi355x_attention_desc *d)
{
    if (q == NULL || qk_params == NULL || pv_params == NULL) return CSINN_FALSE;
    const int dtype = shl_mi355x_dtype_code(q);
    if (dtype < 0 || !plain(q, dtype) || !plain(k, dtype) || !plain(s, dtype) || !plain(p, dtype) || !plain(v, dtype) || !plain(out, dtype))
        return CSINN_FALSE;
    if (qk_params->trans_a || !qk_params->trans_b || pv_params->trans_a || pv_params->trans_b) return CSINN_FALSE;
    int64_t batches = 1;
    for (int i = 0; i < q->dim_count - 2; i++) batches *= q->dim[i];
    const int32_t S = q->dim[q->dim_count - 2], D = q->dim[q->dim_count - 1];
    const int32_t T = k->dim[k->dim_count - 2], DV = v->dim[v->dim_count - 1];
    /* equal batch counts everywhere: the "dense" broadcast of one k or v for every batch is not fused */
    if (batches > 0x7FFFFFFFll || !is_shape(k, batches, T, D) || !is_shape(s, batches, S, T) || !is_shape(p, batches, S, T) ||
        !is_shape(v, batches, T, DV) || !is_shape(out, batches, S, DV))
        return CSINN_FALSE;
    if (axis != p->dim_count - 1) return CSINN_FALSE;
    memset(d, 0, sizeof(*d));
    d->dtype = dtype, d->batches = (int32_t)batches, d->s = S, d->t = T, d->d = D, d->dv = DV;
    d->q_scale = q->qinfo->scale, d->q_zp = q->qinfo->zero_point;
    d->k_scale = k->qinfo->scale, d->k_zp = k->qinfo->zero_point;
    d->v_scale = v->qinfo->scale, d->v_zp = v->qinfo->zero_point;
    d->s_scale = s->qinfo->scale, d->s_zp = s->qinfo->zero_point;
    d->p_scale = p->qinfo->scale, d->p_zp = p->qinfo->zero_point;
    d->out_scale = out->qinfo->scale, d->out_zp = out->qinfo->zero_point;
    d->c_scale = d->sc_scale = 1.0f;
    if (c != NULL) {
        if (sc == NULL || !plain(sc, dtype) || !is_shape(sc, batches, S, T)) return CSINN_FALSE;
        if (shl_mi355x_dtype_code(c) != dtype || c->qinfo == NULL || c->quant_channel > 1 || !c->is_const || c->data == NULL ||
            shl_mi355x_tensor_elems(c) != 1 || (dtype == SHL_MI355X_F16 && c->qinfo->scale != 1.0f))
            return CSINN_FALSE;
        d->has_scale = 1, d->scale_is_first = const_first ? 1 : 0;
        d->scale_raw = dtype == SHL_MI355X_I8 ? (int32_t) * (const int8_t *)c->data : (int32_t) * (const uint16_t *)c->data;
        d->c_scale = c->qinfo->scale, d->c_zp = c->qinfo->zero_point;
        d->sc_scale = sc->qinfo->scale, d->sc_zp = sc->qinfo->zero_point;
    }
    /* the last word belongs to the kernel's own rules (the idiom of matmul.c) */
    const void *a0 = (const void *)((uintptr_t)1 << 56), *a1 = (const void *)((uintptr_t)1 << 57), *a2 = (const void *)((uintptr_t)1 << 58),
               *a3 = (const void *)((uintptr_t)1 << 59);
    if (shl_mi355x_attention_kernel_name(a0, a1, a2, a3, d)[0] == '\0') return CSINN_FALSE;
    return force || shl_mi355x_attention_by_default(a0, a1, a2, a3, d) ? CSINN_TRUE : CSINN_FALSE;
}

/* The add between the (scaled) scores and the softmax of a chain whose other layers shl_mi355x_attention_prepare has put into
 * *d (asked with `force`: whether the biased chain is fused by default is decided here).  in0 / in1 / sum: the add layer's
 * tensors; x: the chain's own tensor among its inputs, the other one is the bias (a mask, a relative position bias).
 * CSINN_TRUE with *bd filled when shl_mi355x_attention_bias takes the chain and -- unless `force` -- fuses the shape by default.
 * The add must be one shl_mi355x_add_exec hands to shl_mi355x_add_bcast with the bias as its broadcast operand: that is the
 * launch the fused kernel equals.  Two operands of equal shape go to shl_mi355x_add there, whose binary16 NaN rule is another
 * (csrc/add_step.h), so they stay apart.  A bias that varies along more than two groups of the batch dims, or whose groups cut
 * through the rows or the keys, has no descriptor and stays apart as well */
int shl_mi355x_attention_bias_prepare(struct csinn_tensor *in0, struct csinn_tensor *in1, struct csinn_tensor *sum,
                                      struct csinn_tensor *x, const struct shl_mi355x_attention_desc *d, int force,
                                      struct shl_mi355x_attention_bias_desc *bd)
{
    if (in0 == NULL || in1 == NULL || d == NULL || (x != in0 && x != in1) || in0 == in1) return CSINN_FALSE;
    struct csinn_tensor *bias = x == in0 ? in1 : in0;
    if (!plain(sum, d->dtype) || !is_shape(sum, d->batches, d->s, d->t) || sum->dim_count != x->dim_count) return CSINN_FALSE;
    if (shl_mi355x_dtype_code(bias) != d->dtype || bias->qinfo == NULL || bias->quant_channel > 1 || bias->dim_count < 1 ||
        bias->dim_count > sum->dim_count || (d->dtype == SHL_MI355X_F16 && bias->qinfo->scale != 1.0f))
        return CSINN_FALSE;
    int same = bias->dim_count == sum->dim_count;
    for (int i = 0; i < sum->dim_count; i++) {
        if (x->dim[i] != sum->dim[i]) return CSINN_FALSE;
        const int j = i - (sum->dim_count - bias->dim_count);
        const int32_t b = j >= 0 ? bias->dim[j] : 1;
        if (b != sum->dim[i] && b != 1) return CSINN_FALSE; /* (asked here, so that bcast_prepare has nothing to complain about) */
        if (j >= 0 && b != sum->dim[i]) same = 0;
    }
    if (same) return CSINN_FALSE;
    struct csinn_tensor *full, *small;
    struct shl_mi355x_mul_desc md;
    if (shl_mi355x_bcast_prepare("add", in0, in1, sum, &full, &small, &md) != CSINN_TRUE || small != bias || full != x) return CSINN_FALSE;
    memset(bd, 0, sizeof(*bd));
    if (shl_mi355x_attention_bias_geometry(&md, d->batches, d->s, d->t, bd) != SHL_MI355X_OK) return CSINN_FALSE;
    bd->bias_is_first = bias == in0;
    bd->b_scale = bias->qinfo->scale, bd->b_zp = bias->qinfo->zero_point;
    bd->sb_scale = sum->qinfo->scale, bd->sb_zp = sum->qinfo->zero_point;
    const void *a0 = (const void *)((uintptr_t)1 << 56), *a1 = (const void *)((uintptr_t)1 << 57), *a2 = (const void *)((uintptr_t)1 << 58),
               *a3 = (const void *)((uintptr_t)1 << 59), *a4 = (const void *)((uintptr_t)1 << 60);
    if (shl_mi355x_attention_bias_kernel_name(a0, a1, a2, a4, a3, d, bd)[0] == '\0') return CSINN_FALSE;
    return force || shl_mi355x_attention_bias_by_default(a0, a1, a2, a4, a3, d, bd) ? CSINN_TRUE : CSINN_FALSE;
}

int shl_mi355x_attention_bias_forward(const struct shl_mi355x_attention_desc *d, const struct shl_mi355x_attention_bias_desc *bd,
                                      const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev, void *out_dev,
                                      void *stream)
{
    int st = shl_mi355x_attention_bias(q_dev, k_dev, v_dev, bias_dev, out_dev, d, bd, stream);
    if (st != SHL_MI355X_OK) {
        shl_debug_error("mi355x: attention with a bias failed (%d): %s\n", st, shl_mi355x_last_error());
        return CSINN_FALSE;
    }
    return CSINN_TRUE;
}

int shl_mi355x_attention_forward(const struct shl_mi355x_attention_desc *d, const void *q_dev, const void *k_dev, const void *v_dev,
                                 void *out_dev, void *stream)
{
    int st = shl_mi355x_attention(q_dev, k_dev, v_dev, out_dev, d, stream);
    if (st != SHL_MI355X_OK) {
        shl_debug_error("mi355x: attention failed (%d): %s\n", st, shl_mi355x_last_error());
        return CSINN_FALSE;
    }
    return CSINN_TRUE;
}

/* the same chains on operands where the projections left them (bd NULL: without a bias) */
int shl_mi355x_attention_layout_forward(const struct shl_mi355x_attention_desc *d, const struct shl_mi355x_attention_bias_desc *bd,
                                        const struct shl_mi355x_attention_layout_desc *ld, const void *q_dev, const void *k_dev,
                                        const void *v_dev, const void *bias_dev, void *out_dev, void *stream)
{
    int st = shl_mi355x_attention_layout(q_dev, k_dev, v_dev, bd ? bias_dev : NULL, out_dev, d, bd, ld, stream);
    if (st != SHL_MI355X_OK) {
        shl_debug_error("mi355x: attention through strides failed (%d): %s\n", st, shl_mi355x_last_error());
        return CSINN_FALSE;
    }
    return CSINN_TRUE;
}

/*
 * matmul.c -- the matmul callbacks of the MI355X backend: CSINN_OP_MATMUL, batched, both transposes and the reference's
 * "dense" broadcast.  It is what makes an attention block of the transposes, reshapes, softmax, mul and add a session already
 * runs (QK^T, PV, and every linear layer a converter exports as MatMul against a constant): with it a MobileViT stage, a ViT
 * encoder layer or a DETR head stays inside a session's single hipGraph.
 *
 * exec(mat0, mat1, output, params) with the reference's signature (source/reference/matmul.c:134-138).  The layer's dims,
 * transposes and broadcast become ONE descriptor of include/shl_mi355x.h: batches, M, N, K and three strides per operand.
 * The reference multiplies the leading dims of each operand into a batch count and accepts equal counts (any transposes) or
 * mat1's count of 1 with no transposes; everything else it refuses, and so does this file -- before anything is staged or
 * written; next to the genuine library such a layer then runs on the reference's kernel.  The reference trusts the output
 * tensor's size and that both operands agree on K; here both are checked.
 */
#include <string.h>

#include "mi355x_internal.h"

static int check_one(const char *what, struct csinn_tensor *t, int *dtype)
{
    if (t == NULL || t->qinfo == NULL) {
        shl_debug_error("mi355x: matmul: the %s is missing or has no quantisation record\n", what);
        return CSINN_FALSE;
    }
    const int dt = t->dtype == CSINN_DTYPE_INT8 ? SHL_MI355X_I8 : t->dtype == CSINN_DTYPE_FLOAT16 ? SHL_MI355X_F16 : -1;
    if (dt < 0 || (*dtype >= 0 && dt != *dtype)) {
        shl_debug_error("mi355x: matmul: dtype %d of the %s is unsupported or differs from the other tensors'\n", t->dtype, what);
        return CSINN_UNSUPPORT_DTYPE;
    }
    *dtype = dt;
    if (t->quant_channel > 1) {
        shl_debug_error("mi355x: matmul: per-channel quantised tensors are not supported\n");
        return CSINN_UNSUPPORT_DTYPE;
    }
    if (dt == SHL_MI355X_F16 && t->qinfo->scale != 1.0f) {
        /* f16_to_float / float_to_f16 scale by qinfo->scale when it differs from 1 (source/nn2/utils.c:1175-1205) */
        shl_debug_error("mi355x: matmul fp16 with qinfo scale != 1 is not supported\n");
        return CSINN_FALSE;
    }
    if (t->dim_count < 2 || t->dim_count > MAX_DIM) {
        shl_debug_error("mi355x: matmul: the %s has %d dims (2 .. %d)\n", what, t->dim_count, MAX_DIM);
        return CSINN_FALSE;
    }
    int64_t n = 1;
    for (int k = 0; k < t->dim_count; k++) {
        if (t->dim[k] < 1) {
            shl_debug_error("mi355x: matmul: dim %d of the %s is %d\n", k, what, t->dim[k]);
            return CSINN_FALSE;
        }
        n *= t->dim[k];
        if (n > 0x7FFFFFFFll) {
            shl_debug_error("mi355x: matmul: the %s has 2^31 or more elements\n", what);
            return CSINN_FALSE;
        }
    }
    return CSINN_TRUE;
}

static int64_t elems_of(const struct csinn_tensor *t)
{
    int64_t n = 1;
    for (int k = 0; k < t->dim_count; k++) n *= t->dim[k];
    return n;
}

/* the layer as a descriptor; CSINN_TRUE, or why not */
static int matmul_prepare(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
                          struct csinn_matmul_params *params, struct shl_mi355x_matmul_desc *d)
{
    int dtype = -1;
    int rc = check_one("first input", mat0, &dtype);
    if (rc == CSINN_TRUE) rc = check_one("second input", mat1, &dtype);
    if (rc == CSINN_TRUE) rc = check_one("output", output, &dtype);
    if (rc != CSINN_TRUE) return rc;
    if (params == NULL) return CSINN_FALSE;
    const int ta = params->trans_a ? 1 : 0, tb = params->trans_b ? 1 : 0;
    int64_t batches_a = 1, batches_b = 1; /* (each below 2^31: check_one) */
    for (int k = 0; k < mat0->dim_count - 2; k++) batches_a *= mat0->dim[k];
    for (int k = 0; k < mat1->dim_count - 2; k++) batches_b *= mat1->dim[k];
    /* matmul.c:41-43 */
    const int32_t m = mat0->dim[mat0->dim_count - (ta ? 1 : 2)], k = mat0->dim[mat0->dim_count - (ta ? 2 : 1)];
    const int32_t n = mat1->dim[mat1->dim_count - (tb ? 2 : 1)], k1 = mat1->dim[mat1->dim_count - (tb ? 1 : 2)];
    if (k1 != k) {
        shl_debug_error("mi355x: matmul: the operands disagree on K (%d and %d)\n", k, k1);
        return CSINN_FALSE;
    }
    if (!(batches_a == batches_b || (batches_a > 1 && batches_b == 1 && !ta && !tb))) {
        shl_debug_error("mi355x: matmul: batches %lld and %lld with trans_a %d, trans_b %d: a broadcast the reference refuses\n",
                        (long long)batches_a, (long long)batches_b, ta, tb);
        return CSINN_FALSE;
    }
    memset(d, 0, sizeof(*d));
    d->dtype = dtype, d->batches = (int32_t)batches_a, d->m = m, d->n = n, d->k = k;
    d->a_batch_stride = (int64_t)m * k, d->a_row_stride = ta ? 1 : k, d->a_k_stride = ta ? m : 1;
    d->b_batch_stride = batches_b == 1 && batches_a > 1 ? 0 : (int64_t)k * n, d->b_col_stride = tb ? k : 1, d->b_k_stride = tb ? 1 : n;
    d->a_elems = elems_of(mat0), d->b_elems = elems_of(mat1), d->out_elems = elems_of(output);
    d->a_scale = mat0->qinfo->scale, d->a_zp = mat0->qinfo->zero_point;
    d->b_scale = mat1->qinfo->scale, d->b_zp = mat1->qinfo->zero_point;
    d->out_scale = output->qinfo->scale, d->out_zp = output->qinfo->zero_point;
    /* the last word belongs to the kernels' own rules: with made-up addresses that do not overlap, the descriptor must name a
     * form (this is where an output tensor of another size is caught) */
    const void *a = (const void *)((uintptr_t)1 << 56), *b = (const void *)((uintptr_t)1 << 57), *o = (const void *)((uintptr_t)1 << 58);
    if (shl_mi355x_matmul_kernel_name(a, b, o, d)[0] == '\0') {
        shl_mi355x_matmul(a, b, (void *)o, d, NULL); /* (refused before anything is enqueued: only the message is wanted) */
        shl_debug_error("mi355x: matmul: %s\n", shl_mi355x_last_error());
        return CSINN_FALSE;
    }
    return CSINN_TRUE;
}

int shl_mi355x_matmul_init(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
                           struct csinn_matmul_params *params)
{
    struct shl_mi355x_matmul_desc d;
    if (matmul_prepare(mat0, mat1, output, params, &d) != CSINN_TRUE)
        shl_mi355x_fall_through(&params->base, CSINN_OP_MATMUL, mat0 ? mat0->dtype : -1);
    return CSINN_TRUE;
}

int shl_mi355x_matmul_exec(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
                           struct csinn_matmul_params *params)
{
    struct shl_mi355x_matmul_desc d;
    int rc = matmul_prepare(mat0, mat1, output, params, &d);
    if (rc != CSINN_TRUE) return rc;
    struct shl_mi355x_ctx *ctx = shl_mi355x_ctx_of(params->base.sess);
    const void *a_dev = shl_mi355x_stage_in(ctx, mat0, 0);
    const void *b_dev = shl_mi355x_stage_in(ctx, mat1, 2);
    void *out_dev = shl_mi355x_stage_out_begin(ctx, output, 1);
    if (a_dev == NULL || b_dev == NULL || out_dev == NULL) return CSINN_FALSE;
    int st = shl_mi355x_matmul(a_dev, b_dev, out_dev, &d, shl_mi355x_ctx_stream(ctx));
    if (st != SHL_MI355X_OK) {
        shl_debug_error("mi355x: matmul failed (%d): %s\n", st, shl_mi355x_last_error());
        return CSINN_FALSE;
    }
    return shl_mi355x_stage_out_end(ctx, output, out_dev);
}

int shl_mi355x_matmul_perf(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
                           struct csinn_matmul_params *params, struct csinn_perf_info *info)
{
    struct shl_mi355x_matmul_desc d;
    int rc = matmul_prepare(mat0, mat1, output, params, &d);
    if (rc != CSINN_TRUE) return rc;
    uintptr_t at = (uintptr_t)1 << 56;
    const void *a = (const void *)shl_mi355x_perf_address(mat0, &at);
    const void *b = (const void *)shl_mi355x_perf_address(mat1, &at);
    const void *o = (const void *)shl_mi355x_perf_address(output, &at);
    info->kernel_name = (char *)shl_mi355x_matmul_kernel_name(a, b, o, &d);
    return CSINN_TRUE;
}

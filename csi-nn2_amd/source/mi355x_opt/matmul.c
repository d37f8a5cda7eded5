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

/* one tensor: what the device carries, 2 .. MAX_DIM dims of at least 1, fewer than 2^31 elements */
static int check_one(const char *what, struct csinn_tensor *t, int *dtype)
{
    int rc = shl_mi355x_check_tensor("matmul", what, t, dtype);
    return rc == CSINN_TRUE ? shl_mi355x_check_dims("matmul", what, t, 2, 1, SHL_MI355X_INT32_ELEMS) : rc;
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
    d->a_elems = shl_mi355x_tensor_elems(mat0), d->b_elems = shl_mi355x_tensor_elems(mat1);
    d->out_elems = shl_mi355x_tensor_elems(output);
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
    struct shl_mi355x_staged s;
    if (shl_mi355x_staged_begin(&params->base, mat0, mat1, output, &s) != CSINN_TRUE) return CSINN_FALSE;
    int st = shl_mi355x_matmul(s.in[0], s.in[1], s.out, &d, s.stream);
    return shl_mi355x_staged_end("matmul", &s, output, st);
}

/* session.c: the matmul layer (mat0, mat1, params; `mid` its output tensor) and the add of the constant `bias` behind it
 * (`output` the add's output) as ONE launch on device buffers; bias_is_first: the bias is the add's first input */
int shl_mi355x_matmul_bias_forward(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *mid,
                                   struct csinn_tensor *bias, struct csinn_tensor *output, struct csinn_matmul_params *params,
                                   int bias_is_first, const void *a_dev, const void *b_dev, const void *bias_dev, void *out_dev,
                                   void *stream)
{
    struct shl_mi355x_matmul_desc d;
    int rc = matmul_prepare(mat0, mat1, mid, params, &d);
    if (rc != CSINN_TRUE) return rc;
    d.out_scale = output->qinfo->scale, d.out_zp = output->qinfo->zero_point;
    int st = shl_mi355x_matmul_bias(a_dev, b_dev, bias_dev, out_dev, &d, bias->qinfo->scale, bias->qinfo->zero_point,
                                    mid->qinfo->scale, mid->qinfo->zero_point, bias_is_first, stream);
    if (st != SHL_MI355X_OK) {
        shl_debug_error("mi355x: matmul + bias failed (%d): %s\n", st, shl_mi355x_last_error());
        return CSINN_FALSE;
    }
    return CSINN_TRUE;
}

int shl_mi355x_matmul_perf(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
                           struct csinn_matmul_params *params, struct csinn_perf_info *info)
{
    struct shl_mi355x_matmul_desc d;
    int rc = matmul_prepare(mat0, mat1, output, params, &d);
    if (rc != CSINN_TRUE) return rc;
    uintptr_t at = SHL_MI355X_PERF_BASE;
    const void *a = (const void *)shl_mi355x_perf_address(mat0, &at);
    const void *b = (const void *)shl_mi355x_perf_address(mat1, &at);
    const void *o = (const void *)shl_mi355x_perf_address(output, &at);
    info->kernel_name = (char *)shl_mi355x_matmul_kernel_name(a, b, o, &d);
    return CSINN_TRUE;
}

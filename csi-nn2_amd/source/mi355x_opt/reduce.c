/*
 * reduce.c -- the reduction callbacks of the MI355X backend: mean, sum, max, min (the stride family), reduce_mean, reduce_sum,
 * reduce_max, reduce_min (the axis family) and global_maxpool2d.  TensorFlow exports global pooling as a mean over H and W
 * (every MobileNetV2 / V3 and EfficientNet tail, every squeeze-and-excite block), CBAM takes a global max pool next to the
 * average one and max / mean over the channel axis, detection and segmentation heads reduce over one axis.  With them such
 * a model stays inside a session's single hipGraph.
 *
 * exec(input, output, params) with the reference's signatures (source/reference/mean.c:55-59, reduce_max.c:65-69,
 * global_maxpool.c:46-50).  All nine become ONE descriptor of include/shl_mi355x.h: two lists of (extent, input stride)
 * groups, the kind and the initial-value rule.  The reference trusts the lists and the axis -- an index past the input, an
 * output tensor of another size, axis_count != 1 (an assert) -- here such a layer is refused before anything is staged or
 * written; next to the genuine library it then runs on the reference's kernel.
 */
#include <string.h>

#include "mi355x_internal.h"

/* what every family asks of the pair: dtypes, records, dims that fit; *d gets the dtype, the records and in_elems */
static int reduce_io(const char *op, struct csinn_tensor *input, struct csinn_tensor *output, struct shl_mi355x_reduce_desc *d)
{
    int dtype;
    int rc = shl_mi355x_check_io(op, input, output, &dtype);
    if (rc == CSINN_TRUE) rc = shl_mi355x_check_dims(op, "input", input, 1, 1, SHL_MI355X_INT32_ELEMS);
    if (rc == CSINN_TRUE) rc = shl_mi355x_check_dims(op, "output", output, 0, 0, 0);
    if (rc != CSINN_TRUE) return rc;
    memset(d, 0, sizeof(*d));
    d->dtype = dtype, d->in_elems = shl_mi355x_tensor_elems(input);
    d->in_scale = input->qinfo->scale, d->in_zp = input->qinfo->zero_point;
    d->out_scale = output->qinfo->scale, d->out_zp = output->qinfo->zero_point;
    return CSINN_TRUE;
}

/* the last word belongs to the kernels' own rules: with made-up addresses that do not overlap, the descriptor must name a
 * form; and the output tensor must hold exactly the outputs */
static int reduce_settle(const char *op, struct csinn_tensor *output, const struct shl_mi355x_reduce_desc *d)
{
    int64_t outs = 1;
    for (int k = 0; k < d->n_out; k++) outs *= d->out_extent[k];
    if (outs != shl_mi355x_tensor_elems(output)) {
        shl_debug_error("mi355x: %s: the layer gives %lld outputs, the output tensor holds %lld\n", op, (long long)outs,
                        (long long)shl_mi355x_tensor_elems(output));
        return CSINN_FALSE;
    }
    const void *in = (const void *)((uintptr_t)1 << 56), *out = (const void *)((uintptr_t)1 << 57);
    if (outs > 0 && shl_mi355x_reduce_kernel_name(in, out, d)[0] == '\0') {
        struct shl_mi355x_reduce_desc copy = *d;
        shl_mi355x_reduce(in, (void *)out, &copy, NULL); /* (refused before anything is enqueued: only the message is wanted) */
        shl_debug_error("mi355x: %s: %s\n", op, shl_mi355x_last_error());
        return CSINN_FALSE;
    }
    return CSINN_TRUE;
}

/* ------------------------------------------------------------------------ mean, sum, max, min */
static int stride_prepare(const char *op, int kind, struct csinn_tensor *input, struct csinn_tensor *output,
                          struct csinn_reduce_params *params, struct shl_mi355x_reduce_desc *d)
{
    int rc = reduce_io(op, input, output, d);
    if (rc != CSINN_TRUE) return rc;
    if (params->n < 0 || params->n > SHL_MI355X_MAX_DIM || params->m < 0 || params->m > SHL_MI355X_MAX_DIM ||
        (params->n > 0 && (params->out_extents == NULL || params->out_strides == NULL)) ||
        (params->m > 0 && (params->inner_extents == NULL || params->inner_strides == NULL))) {
        shl_debug_error("mi355x: %s: %d outer and %d inner groups (at most %d each, with their arrays)\n", op, params->n, params->m,
                        SHL_MI355X_MAX_DIM);
        return CSINN_FALSE;
    }
    d->kind = kind, d->init = SHL_MI355X_REDUCE_INIT_FLT_MAX;
    d->n_out = params->n, d->n_inner = params->m;
    for (int k = 0; k < params->n; k++) d->out_extent[k] = params->out_extents[k], d->out_stride[k] = params->out_strides[k];
    for (int k = 0; k < params->m; k++) d->inner_extent[k] = params->inner_extents[k], d->inner_stride[k] = params->inner_strides[k];
    return reduce_settle(op, output, d);
}

/* ------------------------------------------------------------------------ reduce_mean, reduce_sum, reduce_max, reduce_min */
static int axis_prepare(const char *op, int kind, struct csinn_tensor *input, struct csinn_tensor *output,
                        struct csinn_reduce_params *params, struct shl_mi355x_reduce_desc *d)
{
    int rc = reduce_io(op, input, output, d);
    if (rc != CSINN_TRUE) return rc;
    if (params->axis_count != 1 || params->axis == NULL) {
        shl_debug_error("mi355x: %s: axis_count %d (the reference defines one axis only)\n", op, params->axis_count);
        return CSINN_FALSE;
    }
    const int axis = params->axis[0];
    d->kind = kind, d->init = SHL_MI355X_REDUCE_INIT_FIRST;
    if (axis == -1) { /* the whole tensor to one value */
        d->n_out = 0, d->n_inner = 1;
        d->inner_extent[0] = (int32_t)d->in_elems, d->inner_stride[0] = 1;
        return reduce_settle(op, output, d);
    }
    if (axis < 0 || axis >= input->dim_count) {
        shl_debug_error("mi355x: %s: axis %d of a %d-d tensor\n", op, axis, input->dim_count);
        return CSINN_FALSE;
    }
    int64_t outer = 1, inner = 1;
    for (int k = 0; k < axis; k++) outer *= input->dim[k];
    for (int k = axis + 1; k < input->dim_count; k++) inner *= input->dim[k];
    const int64_t cnt = input->dim[axis];
    d->n_out = 2, d->n_inner = 1;
    d->out_extent[0] = (int32_t)outer, d->out_stride[0] = (int32_t)(cnt * inner); /* (at most in_elems: below 2^31) */
    d->out_extent[1] = (int32_t)inner, d->out_stride[1] = 1;
    d->inner_extent[0] = (int32_t)cnt, d->inner_stride[0] = (int32_t)inner;
    return reduce_settle(op, output, d);
}

/* ------------------------------------------------------------------------ global_maxpool2d */
static int gmp_prepare(const char *op, int kind, struct csinn_tensor *input, struct csinn_tensor *output,
                       struct csinn_pool_params *params, struct shl_mi355x_reduce_desc *d)
{
    (void)kind;
    int rc = reduce_io(op, input, output, d);
    if (rc != CSINN_TRUE) return rc;
    const int nchw = params->base.layout == CSINN_LAYOUT_NCHW;
    if (!nchw && params->base.layout != CSINN_LAYOUT_NHWC) return CSINN_UNSUPPORT_LAYOUT;
    if (input->dim_count != 4 || output->dim_count != 4) {
        shl_debug_error("mi355x: %s expects 4-d tensors (input %d-d, output %d-d)\n", op, input->dim_count, output->dim_count);
        return CSINN_FALSE;
    }
    const int32_t n = input->dim[0], c = input->dim[nchw ? 1 : 3], h = input->dim[nchw ? 2 : 1], w = input->dim[nchw ? 3 : 2];
    if (output->dim[0] != n || output->dim[nchw ? 1 : 3] != c) {
        shl_debug_error("mi355x: %s: the output is not [N, C, 1, 1] / [N, 1, 1, C] of the input\n", op);
        return CSINN_FALSE;
    }
    d->kind = SHL_MI355X_REDUCE_MAX, d->init = SHL_MI355X_REDUCE_INIT_FLT_MAX; /* maxpool.c:47, :90 */
    d->n_out = 2, d->n_inner = 2;
    d->out_extent[0] = n, d->out_stride[0] = c * h * w;
    d->out_extent[1] = c, d->out_stride[1] = nchw ? h * w : 1;
    d->inner_extent[0] = h, d->inner_stride[0] = nchw ? w : w * c;
    d->inner_extent[1] = w, d->inner_stride[1] = nchw ? 1 : c;
    return reduce_settle(op, output, d);
}

/* what the nine ops have in common once their descriptor exists: stage, run, fetch */
static int reduce_run(const char *op, struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_params_base *base,
                      const struct shl_mi355x_reduce_desc *d)
{
    if (csinn_tensor_size(output) == 0) return CSINN_TRUE;
    struct shl_mi355x_staged s;
    if (shl_mi355x_staged_begin(base, input, NULL, output, &s) != CSINN_TRUE) return CSINN_FALSE;
    int st = shl_mi355x_reduce(s.in[0], s.out, d, s.stream);
    return shl_mi355x_staged_end(op, &s, output, st);
}

static int reduce_perf(struct csinn_tensor *input, struct csinn_tensor *output, const struct shl_mi355x_reduce_desc *d,
                       struct csinn_perf_info *info)
{
    uintptr_t at = SHL_MI355X_PERF_BASE;
    const void *in = (const void *)shl_mi355x_perf_address(input, &at);
    const void *out = (const void *)shl_mi355x_perf_address(output, &at);
    info->kernel_name = (char *)shl_mi355x_reduce_kernel_name(in, out, d);
    return CSINN_TRUE;
}

#define REDUCE_OP(name, OP, KIND, PARAMS, prepare)                                                                             \
    int shl_mi355x_##name##_init(struct csinn_tensor *input, struct csinn_tensor *output, struct PARAMS *params)               \
    {                                                                                                                          \
        struct shl_mi355x_reduce_desc d;                                                                                       \
        if (prepare(#name, KIND, input, output, params, &d) != CSINN_TRUE)                                                     \
            shl_mi355x_fall_through(&params->base, OP, input ? input->dtype : -1);                                             \
        return CSINN_TRUE;                                                                                                     \
    }                                                                                                                          \
    int shl_mi355x_##name##_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct PARAMS *params)               \
    {                                                                                                                          \
        struct shl_mi355x_reduce_desc d;                                                                                       \
        int rc = prepare(#name, KIND, input, output, params, &d);                                                              \
        if (rc != CSINN_TRUE) return rc;                                                                                       \
        return reduce_run(#name, input, output, &params->base, &d);                                                            \
    }                                                                                                                          \
    int shl_mi355x_##name##_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct PARAMS *params,               \
                                 struct csinn_perf_info *info)                                                                 \
    {                                                                                                                          \
        struct shl_mi355x_reduce_desc d;                                                                                       \
        int rc = prepare(#name, KIND, input, output, params, &d);                                                              \
        if (rc != CSINN_TRUE) return rc;                                                                                       \
        return reduce_perf(input, output, &d, info);                                                                           \
    }

REDUCE_OP(mean, CSINN_OP_MEAN, SHL_MI355X_REDUCE_MEAN, csinn_reduce_params, stride_prepare)
REDUCE_OP(sum, CSINN_OP_SUM, SHL_MI355X_REDUCE_SUM, csinn_reduce_params, stride_prepare)
REDUCE_OP(max, CSINN_OP_MAX, SHL_MI355X_REDUCE_MAX, csinn_reduce_params, stride_prepare)
REDUCE_OP(min, CSINN_OP_MIN, SHL_MI355X_REDUCE_MIN, csinn_reduce_params, stride_prepare)
REDUCE_OP(reduce_mean, CSINN_OP_REDUCE_MEAN, SHL_MI355X_REDUCE_MEAN, csinn_reduce_params, axis_prepare)
REDUCE_OP(reduce_sum, CSINN_OP_REDUCE_SUM, SHL_MI355X_REDUCE_SUM, csinn_reduce_params, axis_prepare)
REDUCE_OP(reduce_max, CSINN_OP_REDUCE_MAX, SHL_MI355X_REDUCE_MAX, csinn_reduce_params, axis_prepare)
REDUCE_OP(reduce_min, CSINN_OP_REDUCE_MIN, SHL_MI355X_REDUCE_MIN, csinn_reduce_params, axis_prepare)
REDUCE_OP(global_maxpool2d, CSINN_OP_GLOBAL_MAXPOOL2D, SHL_MI355X_REDUCE_MAX, csinn_pool_params, gmp_prepare)

/*
 * pooling.c -- global_avgpool2d and softmax callbacks of the MI355X backend: the two operators
 * between MobileNetV1's last pointwise convolution and its output (SURVEY 8f1;
 * example/c906_mobilenetv1_f16.c:1805-1886 of the reference); the windowed maxpool2d / avgpool2d (ResNet's stem
 * pool, Inception-style average pools); add (residual, and with one operand broadcast); concat (the end of every Fire module and Inception block).
 *
 * exec(input, output, params) with the reference's signatures
 * (source/reference/global_averagepool.c:46-50, maxpool.c:113-124, averagepool.c:127-138, softmax.c:68-72,
 * concat.c:51-76).
 */
#include <stdlib.h>
#include <string.h>

#include "mi355x_internal.h"

int shl_mi355x_global_avgpool2d_exec(struct csinn_tensor *input, struct csinn_tensor *output,
                                     struct csinn_pool_params *params)
{
    int dtype;
    int rc = shl_mi355x_check_io("global_avgpool2d", input, output, &dtype);
    if (rc != CSINN_TRUE) return rc;
    if (input->dim_count != 4) {
        shl_debug_error("mi355x: global_avgpool2d expects a 4-d tensor\n");
        return CSINN_FALSE;
    }
    int layout, c, hw;
    if (params->base.layout == CSINN_LAYOUT_NCHW) {
        layout = SHL_MI355X_NCHW;
        c = input->dim[1];
        hw = input->dim[2] * input->dim[3];
    } else if (params->base.layout == CSINN_LAYOUT_NHWC) {
        layout = SHL_MI355X_NHWC;
        c = input->dim[3];
        hw = input->dim[1] * input->dim[2];
    } else {
        return CSINN_UNSUPPORT_LAYOUT;
    }
    struct shl_mi355x_staged s;
    if (shl_mi355x_staged_begin(&params->base, input, NULL, output, &s) != CSINN_TRUE) return CSINN_FALSE;
    int st = shl_mi355x_global_avgpool2d(s.in[0], s.out, dtype, layout, input->dim[0], c, hw, input->qinfo->scale,
                                         input->qinfo->zero_point, output->qinfo->scale, output->qinfo->zero_point, s.stream);
    return shl_mi355x_staged_end("global_avgpool2d", &s, output, st);
}

/* maxpool2d / avgpool2d (source/reference/maxpool.c:113-124, averagepool.c:127-138): the window geometry comes
 * from params, the output size from the OUTPUT tensor's dims (ceil_mode, pad_down and pad_right act through it) */
static int pool2d_desc(const char *op, int kind, struct csinn_tensor *input, struct csinn_tensor *output,
                       struct csinn_pool_params *params, struct shl_mi355x_pool_desc *desc)
{
    int dtype;
    int rc = shl_mi355x_check_io(op, input, output, &dtype);
    if (rc != CSINN_TRUE) return rc;
    if (input->dim_count != 4 || output->dim_count != 4) {
        shl_debug_error("mi355x: %s expects a 4-d tensor\n", op);
        return CSINN_FALSE;
    }
    struct shl_mi355x_pool_desc d;
    memset(&d, 0, sizeof(d));
    int out_c;
    if (params->base.layout == CSINN_LAYOUT_NCHW) {
        d.layout = SHL_MI355X_NCHW;
        d.c = input->dim[1], d.in_h = input->dim[2], d.in_w = input->dim[3];
        out_c = output->dim[1], d.out_h = output->dim[2], d.out_w = output->dim[3];
    } else if (params->base.layout == CSINN_LAYOUT_NHWC) {
        d.layout = SHL_MI355X_NHWC;
        d.in_h = input->dim[1], d.in_w = input->dim[2], d.c = input->dim[3];
        d.out_h = output->dim[1], d.out_w = output->dim[2], out_c = output->dim[3];
    } else {
        return CSINN_UNSUPPORT_LAYOUT;
    }
    if (output->dim[0] != input->dim[0] || out_c != d.c) {
        shl_debug_error("mi355x: %s: batch / channels of input and output differ\n", op);
        return CSINN_FALSE;
    }
    d.kind = kind;
    d.dtype = dtype;
    d.batch = input->dim[0];
    d.kernel_h = params->filter_height, d.kernel_w = params->filter_width;
    d.stride_h = params->stride_height, d.stride_w = params->stride_width;
    d.pad_top = params->pad_top, d.pad_left = params->pad_left;
    d.count_include_pad = params->count_include_pad ? 1 : 0;
    d.in_scale = input->qinfo->scale, d.in_zp = input->qinfo->zero_point;
    d.out_scale = output->qinfo->scale, d.out_zp = output->qinfo->zero_point;
    *desc = d;
    return CSINN_TRUE;
}

static int pool2d_exec(const char *op, int kind, struct csinn_tensor *input, struct csinn_tensor *output,
                       struct csinn_pool_params *params)
{
    struct shl_mi355x_pool_desc d;
    int rc = pool2d_desc(op, kind, input, output, params, &d);
    if (rc != CSINN_TRUE) return rc;
    struct shl_mi355x_staged s;
    if (shl_mi355x_staged_begin(&params->base, input, NULL, output, &s) != CSINN_TRUE) return CSINN_FALSE;
    int st = shl_mi355x_pool2d(s.in[0], s.out, &d, s.stream);
    return shl_mi355x_staged_end(op, &s, output, st);
}

int shl_mi355x_maxpool2d_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pool_params *params)
{
    return pool2d_exec("maxpool2d", SHL_MI355X_POOL_MAX, input, output, params);
}

int shl_mi355x_avgpool2d_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pool_params *params)
{
    return pool2d_exec("avgpool2d", SHL_MI355X_POOL_AVG, input, output, params);
}

/* perf callbacks (single-input signature): the kernel form the rules choose for this layer */
static int pool2d_perf(const char *op, int kind, struct csinn_tensor *input, struct csinn_tensor *output,
                       struct csinn_pool_params *params, struct csinn_perf_info *info)
{
    struct shl_mi355x_pool_desc d;
    int rc = pool2d_desc(op, kind, input, output, params, &d);
    if (rc != CSINN_TRUE) return rc;
    info->kernel_name = (char *)shl_mi355x_pool2d_kernel_name(&d);
    return CSINN_TRUE;
}

int shl_mi355x_maxpool2d_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pool_params *params,
                              struct csinn_perf_info *info)
{
    return pool2d_perf("maxpool2d", SHL_MI355X_POOL_MAX, input, output, params, info);
}

int shl_mi355x_avgpool2d_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pool_params *params,
                              struct csinn_perf_info *info)
{
    return pool2d_perf("avgpool2d", SHL_MI355X_POOL_AVG, input, output, params, info);
}

int shl_mi355x_softmax_exec(struct csinn_tensor *input, struct csinn_tensor *output,
                            struct csinn_softmax_params *params)
{
    int dtype;
    int rc = shl_mi355x_check_io("softmax", input, output, &dtype);
    if (rc != CSINN_TRUE) return rc;
    const int axis = params->axis;
    if (axis < 0 || axis >= input->dim_count) {
        shl_debug_error("mi355x: softmax axis %d out of range\n", axis);
        return CSINN_FALSE;
    }
    int64_t outer = 1, inner = 1;
    for (int i = 0; i < axis; i++) outer *= input->dim[i];
    for (int i = axis + 1; i < input->dim_count; i++) inner *= input->dim[i];
    struct shl_mi355x_staged s;
    if (shl_mi355x_staged_begin(&params->base, input, NULL, output, &s) != CSINN_TRUE) return CSINN_FALSE;
    int st = shl_mi355x_softmax(s.in[0], s.out, dtype, outer, input->dim[axis], inner, input->qinfo->scale,
                                input->qinfo->zero_point, output->qinfo->scale, output->qinfo->zero_point, s.stream);
    return shl_mi355x_staged_end("softmax", &s, output, st);
}

/* add (source/reference/add.c:21-41).  Two same-shape inputs (the residual add) go to shl_mi355x_add; a layer with one
 * operand broadcast to the other (a bias, a mask, a positional embedding) to shl_mi355x_add_bcast, by mul's geometry rule
 * (eltwise.c).  add_check: CSINN_TRUE with *same_shape set, or the status to return */
static int add_check(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output, int *dtype,
                     int *same_shape)
{
    int rc = shl_mi355x_check_io("add", input0, output, dtype);
    if (rc != CSINN_TRUE) return rc;
    /* (every defect of the second input is CSINN_UNSUPPORT_DTYPE, unlike shl_mi355x_check_tensor's statuses) */
    if (shl_mi355x_dtype_code(input1) != *dtype || input1->qinfo == NULL || input1->quant_channel > 1 ||
        (*dtype == SHL_MI355X_F16 && input1->qinfo->scale != 1.0f)) {
        shl_debug_error("mi355x: add: second input dtype / quantisation unsupported\n");
        return CSINN_UNSUPPORT_DTYPE;
    }
    *same_shape = input0->dim_count == input1->dim_count && input0->dim_count == output->dim_count;
    for (int i = 0; *same_shape && i < input0->dim_count; i++)
        *same_shape = input0->dim[i] == input1->dim[i] && input0->dim[i] == output->dim[i];
    return CSINN_TRUE;
}

int shl_mi355x_add_exec(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                        struct csinn_diso_params *params)
{
    int dtype, same_shape;
    int rc = add_check(input0, input1, output, &dtype, &same_shape);
    if (rc != CSINN_TRUE) return rc;
    struct shl_mi355x_staged s;
    if (same_shape) {
        if (shl_mi355x_staged_begin(&params->base, input0, input1, output, &s) != CSINN_TRUE) return CSINN_FALSE;
        int st = shl_mi355x_add(s.in[0], s.in[1], s.out, (size_t)csinn_tensor_size(output), dtype, input0->qinfo->scale,
                                input0->qinfo->zero_point, input1->qinfo->scale, input1->qinfo->zero_point,
                                output->qinfo->scale, output->qinfo->zero_point, s.stream);
        return shl_mi355x_staged_end("add", &s, output, st);
    }
    struct csinn_tensor *full, *small;
    struct shl_mi355x_mul_desc d;
    rc = shl_mi355x_bcast_prepare("add", input0, input1, output, &full, &small, &d);
    if (rc != CSINN_TRUE) return rc;
    if (csinn_tensor_size(output) == 0) return CSINN_TRUE;
    /* the inputs are staged in their own order, whichever of them is the broadcast one */
    if (shl_mi355x_staged_begin(&params->base, input0, input1, output, &s) != CSINN_TRUE) return CSINN_FALSE;
    const int a = full == input0 ? 0 : 1;
    int st = shl_mi355x_add_bcast(s.in[a], s.in[1 - a], s.out, &d, s.stream);
    return shl_mi355x_staged_end("add", &s, output, st);
}

/* a broadcasting layer: the form the rule chooses; a same-shape one: the name under its params block (there is none: "") */
int shl_mi355x_add_perf(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                        struct csinn_diso_params *params, struct csinn_perf_info *info)
{
    int dtype, same_shape;
    int rc = add_check(input0, input1, output, &dtype, &same_shape);
    if (rc != CSINN_TRUE) return rc;
    if (same_shape) {
        info->kernel_name = (char *)shl_mi355x_params_kernel_name(params);
        return CSINN_TRUE;
    }
    struct csinn_tensor *full, *small;
    struct shl_mi355x_mul_desc d;
    rc = shl_mi355x_bcast_prepare("add", input0, input1, output, &full, &small, &d);
    if (rc != CSINN_TRUE) return rc;
    uintptr_t at = SHL_MI355X_PERF_BASE;
    const void *in[2];
    in[0] = (const void *)shl_mi355x_perf_address(input0, &at), in[1] = (const void *)shl_mi355x_perf_address(input1, &at);
    const int a = full == input0 ? 0 : 1;
    info->kernel_name =
        (char *)shl_mi355x_add_bcast_kernel_name(&d, in[a], in[1 - a], (const void *)shl_mi355x_perf_address(output, &at));
    return CSINN_TRUE;
}

/* concat (source/reference/concat.c:21-76): a variable number of inputs.  The reference trusts the shapes; here a
 * mismatch is an error, where it would read past a buffer. */
struct concat_call {
    struct shl_mi355x_concat_desc desc;
    int64_t *len;
    float *scale;
    int32_t *zp;
    const void **dev;
};

static void concat_release(struct concat_call *c)
{
    free(c->len);
    free(c->scale);
    free(c->zp);
    free(c->dev);
}

static int concat_prepare(struct csinn_tensor **input, struct csinn_tensor *output, struct csinn_concat_params *params,
                          struct concat_call *c)
{
    memset(c, 0, sizeof(*c));
    const int n = params->inputs_count;
    if (input == NULL || n < 1) {
        shl_debug_error("mi355x: concat needs at least one input\n");
        return CSINN_FALSE;
    }
    const int dims = output->dim_count;
    /* axis == -1 is the last axis; the reference rewrites params->axis, which a params block shared between threads
     * or replayed by a graph has no need of */
    const int axis = params->axis == -1 ? dims - 1 : params->axis;
    if (dims < 1 || dims > MAX_DIM || axis < 0 || axis >= dims) {
        shl_debug_error("mi355x: concat: axis %d of a %d-d tensor\n", params->axis, dims);
        return CSINN_FALSE;
    }
    int64_t outer = 1, inner = 1, along = 0;
    for (int k = 0; k < axis; k++) outer *= output->dim[k];
    for (int k = axis + 1; k < dims; k++) inner *= output->dim[k];
    int dtype = -1;
    for (int i = 0; i < n; i++) {
        if (input[i] == NULL) {
            shl_debug_error("mi355x: concat: input %d is NULL\n", i);
            return CSINN_FALSE;
        }
        int rc = shl_mi355x_check_io("concat", input[i], output, &dtype);
        if (rc != CSINN_TRUE) return rc;
        if (input[i]->dim_count != dims) {
            shl_debug_error("mi355x: concat: input %d is %d-d, the output %d-d\n", i, input[i]->dim_count, dims);
            return CSINN_FALSE;
        }
        for (int k = 0; k < dims; k++)
            if (input[i]->dim[k] < 0 || (k != axis && input[i]->dim[k] != output->dim[k])) {
                shl_debug_error("mi355x: concat: dim %d of input %d is %d, the output's %d\n", k, i, input[i]->dim[k],
                                output->dim[k]);
                return CSINN_FALSE;
            }
        along += input[i]->dim[axis];
    }
    if (along != output->dim[axis]) {
        shl_debug_error("mi355x: concat: the inputs hold %lld along axis %d, the output %d\n", (long long)along, axis,
                        output->dim[axis]);
        return CSINN_FALSE;
    }
    c->len = calloc((size_t)n, sizeof(*c->len));
    c->scale = calloc((size_t)n, sizeof(*c->scale));
    c->zp = calloc((size_t)n, sizeof(*c->zp));
    c->dev = calloc((size_t)n, sizeof(*c->dev));
    if (!c->len || !c->scale || !c->zp || !c->dev) {
        concat_release(c);
        return CSINN_FALSE;
    }
    for (int i = 0; i < n; i++) {
        c->len[i] = input[i]->dim[axis] * inner;
        c->scale[i] = input[i]->qinfo->scale;
        c->zp[i] = input[i]->qinfo->zero_point;
    }
    c->desc.dtype = dtype;
    c->desc.n_inputs = n;
    c->desc.outer = outer;
    c->desc.out_scale = output->qinfo->scale;
    c->desc.out_zp = output->qinfo->zero_point;
    return CSINN_TRUE;
}

int shl_mi355x_concat_exec(struct csinn_tensor **input, struct csinn_tensor *output, struct csinn_concat_params *params)
{
    struct concat_call c;
    int rc = concat_prepare(input, output, params, &c);
    if (rc != CSINN_TRUE) return rc;
    if (csinn_tensor_size(output) == 0) {
        concat_release(&c);
        return CSINN_TRUE;
    }
    struct shl_mi355x_ctx *ctx = shl_mi355x_ctx_of(params->base.sess);
    void *out_dev = NULL;
    if (shl_mi355x_stage_in_many(ctx, input, c.desc.n_inputs, c.dev) == CSINN_TRUE)
        out_dev = shl_mi355x_stage_out_begin(ctx, output, 1);
    if (out_dev == NULL) {
        concat_release(&c);
        return CSINN_FALSE;
    }
    int st = shl_mi355x_concat(c.dev, c.len, c.scale, c.zp, out_dev, &c.desc, shl_mi355x_ctx_stream(ctx));
    concat_release(&c);
    if (st != SHL_MI355X_OK) {
        shl_debug_error("mi355x: concat failed (%d): %s\n", st, shl_mi355x_last_error());
        return CSINN_FALSE;
    }
    return shl_mi355x_stage_out_end(ctx, output, out_dev);
}

/* the form the rules choose for this layer.  They look at addresses: a DMABUF tensor has its own; host tensors are given
 * the alignment the staging path will give them (made-up, disjoint addresses: nothing is staged here) */
int shl_mi355x_concat_perf(struct csinn_tensor **input, struct csinn_tensor *output, struct csinn_concat_params *params,
                           struct csinn_perf_info *info)
{
    struct concat_call c;
    int rc = concat_prepare(input, output, params, &c);
    if (rc != CSINN_TRUE) return rc;
    uintptr_t at = SHL_MI355X_PERF_BASE;
    for (int i = 0; i < c.desc.n_inputs; i++) c.dev[i] = (const void *)shl_mi355x_perf_address(input[i], &at);
    const void *out = (const void *)shl_mi355x_perf_address(output, &at);
    info->kernel_name = (char *)shl_mi355x_concat_kernel_name(c.dev, c.len, c.scale, c.zp, out, &c.desc);
    concat_release(&c);
    return CSINN_TRUE;
}

/*
 * split.c -- the split and shuffle_channel callbacks of the MI355X backend: the operators that DIVIDE a tensor, so that
 * ShuffleNetV2 units (split -> branch -> concat -> shuffle_channel) and the CSP / C2f blocks of YOLO backbones
 * (conv -> split -> bottlenecks -> concat) stay inside a session's single hipGraph.
 *
 * exec(input, output[], params) / exec(input, output, params) with the reference's signatures
 * (source/reference/split.c:74-92, shuffle_channel.c:78-82).  The reference trusts the shapes -- a split of dim 5 into 4
 * gives chunks of 2 and a last one of -1, and it runs off the end; with output_num == 1 and a split_index it reads
 * split_index[-1] -- here such a layer is refused before anything is staged or written.
 */
#include <stdlib.h>
#include <string.h>

#include "mi355x_internal.h"

/* ------------------------------------------------------------------------ split */
struct split_call {
    struct shl_mi355x_split_desc desc;
    int64_t *len;
    float *scale;
    int32_t *zp;
    void **dev;
};

static void split_release(struct split_call *c)
{
    free(c->len);
    free(c->scale);
    free(c->zp);
    free(c->dev);
}

/* the descriptor of the layer, or why there is none; looks at dims, dtypes and records only (never at `data`: in graph
 * mode that is a node while the graph is built) */
static int split_prepare(struct csinn_tensor *input, struct csinn_tensor **output, struct csinn_split_params *params,
                         struct split_call *c)
{
    memset(c, 0, sizeof(*c));
    const int n = params->output_num;
    if (input == NULL || output == NULL || n < 1) {
        shl_debug_error("mi355x: split needs at least one output\n");
        return CSINN_FALSE;
    }
    const int dims = input->dim_count;
    /* a negative axis counts from the back (split.c:26); params is left alone */
    const int axis = params->axis < 0 ? dims + params->axis : params->axis;
    if (dims < 1 || dims > MAX_DIM || axis < 0 || axis >= dims) {
        shl_debug_error("mi355x: split: axis %d of a %d-d tensor\n", params->axis, dims);
        return CSINN_FALSE;
    }
    const int64_t along = input->dim[axis];
    const int64_t avg = (along + n - 1) / n;
    int64_t outer = 1, inner = 1;
    for (int k = 0; k < axis; k++) outer *= input->dim[k];
    for (int k = axis + 1; k < dims; k++) inner *= input->dim[k];
    if (outer < 0 || inner < 0) {
        shl_debug_error("mi355x: split: a negative dim\n");
        return CSINN_FALSE;
    }
    int dtype = -1;
    int64_t begin = 0;
    for (int i = 0; i < n; i++) {
        if (output[i] == NULL) {
            shl_debug_error("mi355x: split: output %d is NULL\n", i);
            return CSINN_FALSE;
        }
        int rc = shl_mi355x_check_io("split", input, output[i], &dtype);
        if (rc != CSINN_TRUE) return rc;
        /* where output i ends: split_index[i], or i + 1 chunks; the last output ends where the axis does
         * (output_num == 1: the whole tensor, split_index is not read) */
        int64_t end;
        if (i == n - 1) end = along;
        else if (params->split_index != NULL) end = params->split_index[i];
        else end = (i + 1) * avg;
        if (end <= begin || end > along) {
            shl_debug_error("mi355x: split: output %d would hold [%lld, %lld) of %lld along axis %d\n", i, (long long)begin,
                            (long long)end, (long long)along, axis);
            return CSINN_FALSE;
        }
        if (output[i]->dim_count != dims) {
            shl_debug_error("mi355x: split: output %d is %d-d, the input %d-d\n", i, output[i]->dim_count, dims);
            return CSINN_FALSE;
        }
        for (int k = 0; k < dims; k++)
            if (output[i]->dim[k] != (k == axis ? end - begin : input->dim[k])) {
                shl_debug_error("mi355x: split: dim %d of output %d is %d, expected %lld\n", k, i, output[i]->dim[k],
                                (long long)(k == axis ? end - begin : input->dim[k]));
                return CSINN_FALSE;
            }
        for (int j = 0; j < i; j++)
            if (output[j] == output[i]) {
                shl_debug_error("mi355x: split: outputs %d and %d are the same tensor\n", j, i);
                return CSINN_FALSE;
            }
        begin = end;
    }
    c->len = calloc((size_t)n, sizeof(*c->len));
    c->scale = calloc((size_t)n, sizeof(*c->scale));
    c->zp = calloc((size_t)n, sizeof(*c->zp));
    c->dev = calloc((size_t)n, sizeof(*c->dev));
    if (!c->len || !c->scale || !c->zp || !c->dev) {
        split_release(c);
        return CSINN_FALSE;
    }
    for (int i = 0; i < n; i++) {
        c->len[i] = output[i]->dim[axis] * inner;
        c->scale[i] = output[i]->qinfo->scale;
        c->zp[i] = output[i]->qinfo->zero_point;
    }
    c->desc.dtype = dtype;
    c->desc.n_outputs = n;
    c->desc.outer = outer;
    c->desc.in_scale = input->qinfo->scale;
    c->desc.in_zp = input->qinfo->zero_point;
    return CSINN_TRUE;
}

int shl_mi355x_split_init(struct csinn_tensor *input, struct csinn_tensor **output, struct csinn_split_params *params)
{
    struct split_call c;
    if (split_prepare(input, output, params, &c) == CSINN_TRUE) split_release(&c);
    else shl_mi355x_fall_through(&params->base, CSINN_OP_SPLIT, input ? input->dtype : -1);
    return CSINN_TRUE;
}

int shl_mi355x_split_exec(struct csinn_tensor *input, struct csinn_tensor **output, struct csinn_split_params *params)
{
    struct split_call c;
    int rc = split_prepare(input, output, params, &c);
    if (rc != CSINN_TRUE) return rc;
    if (csinn_tensor_size(input) == 0) {
        split_release(&c);
        return CSINN_TRUE;
    }
    struct shl_mi355x_ctx *ctx = shl_mi355x_ctx_of(params->base.sess);
    const int n = c.desc.n_outputs;
    const void *in_dev = shl_mi355x_stage_in(ctx, input, 0);
    if (in_dev == NULL || shl_mi355x_stage_out_many_begin(ctx, output, n, c.dev) != CSINN_TRUE) {
        split_release(&c);
        return CSINN_FALSE;
    }
    int st = shl_mi355x_split(in_dev, c.dev, c.len, c.scale, c.zp, &c.desc, shl_mi355x_ctx_stream(ctx));
    if (st != SHL_MI355X_OK) {
        shl_debug_error("mi355x: split failed (%d): %s\n", st, shl_mi355x_last_error());
        split_release(&c);
        return CSINN_FALSE;
    }
    rc = shl_mi355x_stage_out_many_end(ctx, output, n, c.dev);
    split_release(&c);
    return rc;
}

/* the form the rules choose for this layer */
int shl_mi355x_split_perf(struct csinn_tensor *input, struct csinn_tensor **output, struct csinn_split_params *params,
                          struct csinn_perf_info *info)
{
    struct split_call c;
    int rc = split_prepare(input, output, params, &c);
    if (rc != CSINN_TRUE) return rc;
    uintptr_t at = SHL_MI355X_PERF_BASE;
    const void *in = (const void *)shl_mi355x_perf_address(input, &at);
    for (int i = 0; i < c.desc.n_outputs; i++) c.dev[i] = (void *)shl_mi355x_perf_address(output[i], &at);
    info->kernel_name = (char *)shl_mi355x_split_kernel_name(in, c.dev, c.len, c.scale, c.zp, &c.desc);
    split_release(&c);
    return CSINN_TRUE;
}

/* ------------------------------------------------------------------------ shuffle_channel */
static int shuffle_desc(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_shuffle_channel_params *params,
                        struct shl_mi355x_shuffle_desc *desc)
{
    int dtype;
    int rc = shl_mi355x_check_io("shuffle_channel", input, output, &dtype);
    if (rc != CSINN_TRUE) return rc;
    if (input->dim_count != 4 || output->dim_count != 4) {
        shl_debug_error("mi355x: shuffle_channel expects 4-d tensors\n");
        return CSINN_FALSE;
    }
    for (int k = 0; k < 4; k++)
        if (input->dim[k] < 0 || output->dim[k] != input->dim[k]) {
            shl_debug_error("mi355x: shuffle_channel: dim %d of the input is %d, of the output %d\n", k, input->dim[k],
                            output->dim[k]);
            return CSINN_FALSE;
        }
    struct shl_mi355x_shuffle_desc d;
    memset(&d, 0, sizeof(d));
    if (params->base.layout == CSINN_LAYOUT_NCHW) {
        d.outer = input->dim[0], d.c = input->dim[1], d.inner = (int64_t)input->dim[2] * input->dim[3];
    } else if (params->base.layout == CSINN_LAYOUT_NHWC) {
        d.outer = (int64_t)input->dim[0] * input->dim[1] * input->dim[2], d.c = input->dim[3], d.inner = 1;
    } else {
        return CSINN_UNSUPPORT_LAYOUT;
    }
    if (params->group < 1 || d.c < 1 || d.c % params->group != 0) {
        shl_debug_error("mi355x: shuffle_channel: %lld channels in %d groups\n", (long long)d.c, params->group);
        return CSINN_FALSE;
    }
    if (d.inner == 0) d.inner = 1, d.outer = 0; /* a tensor without pixels: nothing to do */
    d.dtype = dtype;
    d.group = params->group;
    d.in_scale = input->qinfo->scale, d.in_zp = input->qinfo->zero_point;
    d.out_scale = output->qinfo->scale, d.out_zp = output->qinfo->zero_point;
    *desc = d;
    return CSINN_TRUE;
}

int shl_mi355x_shuffle_channel_init(struct csinn_tensor *input, struct csinn_tensor *output,
                                    struct csinn_shuffle_channel_params *params)
{
    struct shl_mi355x_shuffle_desc d;
    if (shuffle_desc(input, output, params, &d) != CSINN_TRUE)
        shl_mi355x_fall_through(&params->base, CSINN_OP_SHUFFLE_CHANNEL, input ? input->dtype : -1);
    return CSINN_TRUE;
}

int shl_mi355x_shuffle_channel_exec(struct csinn_tensor *input, struct csinn_tensor *output,
                                    struct csinn_shuffle_channel_params *params)
{
    struct shl_mi355x_shuffle_desc d;
    int rc = shuffle_desc(input, output, params, &d);
    if (rc != CSINN_TRUE) return rc;
    if (csinn_tensor_size(output) == 0) return CSINN_TRUE;
    struct shl_mi355x_staged s;
    if (shl_mi355x_staged_begin(&params->base, input, NULL, output, &s) != CSINN_TRUE) return CSINN_FALSE;
    int st = shl_mi355x_shuffle_channel(s.in[0], s.out, &d, s.stream);
    return shl_mi355x_staged_end("shuffle_channel", &s, output, st);
}

int shl_mi355x_shuffle_channel_perf(struct csinn_tensor *input, struct csinn_tensor *output,
                                    struct csinn_shuffle_channel_params *params, struct csinn_perf_info *info)
{
    struct shl_mi355x_shuffle_desc d;
    int rc = shuffle_desc(input, output, params, &d);
    if (rc != CSINN_TRUE) return rc;
    uintptr_t at = SHL_MI355X_PERF_BASE;
    const void *in = (const void *)shl_mi355x_perf_address(input, &at);
    info->kernel_name = (char *)shl_mi355x_shuffle_channel_kernel_name(in, (const void *)shl_mi355x_perf_address(output, &at), &d);
    return CSINN_TRUE;
}

/*
 * move.c -- the transpose, reshape, flatten and pad callbacks of the MI355X backend: the operators that only change a
 * tensor's order or shape, which a converter emits around every kernel -- flatten / reshape between global_avgpool2d and
 * fullyconnected, a pad for TensorFlow's asymmetric SAME padding in front of a stride-2 convolution, reshape -> transpose in
 * every detection head and attention block.  With them such a model stays inside a session's single hipGraph.
 *
 * exec(input, output, params) with the reference's signatures (source/reference/transpose.c:96-100, reshape.c:49-53,
 * flatten.c:54-58, pad.c:136-140).  The reference trusts the shapes -- a transpose whose output dims are not the permuted
 * input dims, a reshape into fewer elements, a pad whose output is too small all run off the end of a buffer, EDGE and
 * REFLECT pads hit an assert -- here such a layer is refused before anything is staged or written.
 */
#include <string.h>

#include "mi355x_internal.h"

/* dtypes and records of the pair, and what tensors of any rank add: dims that fit (a tensor may hold 2^31 elements or more:
 * the kernels count in 64 bits) */
static int check_io(const char *op, struct csinn_tensor *input, struct csinn_tensor *output, int *dtype)
{
    int rc = shl_mi355x_check_io(op, input, output, dtype);
    if (rc == CSINN_TRUE) rc = shl_mi355x_check_dims(op, "input", input, 0, 0, 0);
    if (rc == CSINN_TRUE) rc = shl_mi355x_check_dims(op, "output", output, 0, 0, 0);
    return rc;
}

/* what the three ops have in common once their descriptor exists: stage, run, fetch */
enum move_kind { MOVE_TRANSPOSE, MOVE_FLAT, MOVE_PAD };
struct move_call {
    enum move_kind kind;
    int64_t elems; /* MOVE_FLAT */
    union {
        struct shl_mi355x_transpose_desc transpose;
        struct shl_mi355x_move_desc flat;
        struct shl_mi355x_pad_desc pad;
    } d;
};

static int move_run(const char *op, struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_params_base *base,
                    const struct move_call *c)
{
    if (csinn_tensor_size(output) == 0) return CSINN_TRUE;
    struct shl_mi355x_staged s;
    if (shl_mi355x_staged_begin(base, input, NULL, output, &s) != CSINN_TRUE) return CSINN_FALSE;
    int st;
    if (c->kind == MOVE_TRANSPOSE) st = shl_mi355x_transpose(s.in[0], s.out, &c->d.transpose, s.stream);
    else if (c->kind == MOVE_PAD) st = shl_mi355x_pad(s.in[0], s.out, &c->d.pad, s.stream);
    else st = shl_mi355x_move(s.in[0], s.out, c->elems, &c->d.flat, s.stream);
    return shl_mi355x_staged_end(op, &s, output, st);
}

static int move_perf(struct csinn_tensor *input, struct csinn_tensor *output, const struct move_call *c,
                     struct csinn_perf_info *info)
{
    uintptr_t at = SHL_MI355X_PERF_BASE;
    const void *in = (const void *)shl_mi355x_perf_address(input, &at);
    const void *out = (const void *)shl_mi355x_perf_address(output, &at);
    if (c->kind == MOVE_TRANSPOSE) info->kernel_name = (char *)shl_mi355x_transpose_kernel_name(in, out, &c->d.transpose);
    else if (c->kind == MOVE_PAD) info->kernel_name = (char *)shl_mi355x_pad_kernel_name(in, out, &c->d.pad);
    else info->kernel_name = (char *)shl_mi355x_move_kernel_name(in, out, c->elems, &c->d.flat);
    return CSINN_TRUE;
}

/* ------------------------------------------------------------------------ transpose */
/* the descriptor of the layer, or why there is none; looks at dims, dtypes and records only (never at `data`: in graph
 * mode that is a node while the graph is built) */
static int transpose_prepare(const char *op, struct csinn_tensor *input, struct csinn_tensor *output,
                             struct csinn_transpose_params *params, struct move_call *c)
{
    int dtype;
    int rc = check_io(op, input, output, &dtype);
    if (rc != CSINN_TRUE) return rc;
    const int rank = input->dim_count;
    if (rank < 1 || params->permute_num != rank || output->dim_count != rank || params->permute == NULL) {
        shl_debug_error("mi355x: transpose: permute_num %d, input %d-d, output %d-d\n", params->permute_num, input->dim_count,
                        output->dim_count);
        return CSINN_FALSE;
    }
    memset(c, 0, sizeof(*c));
    c->kind = MOVE_TRANSPOSE;
    struct shl_mi355x_transpose_desc *d = &c->d.transpose;
    unsigned seen = 0;
    for (int k = 0; k < rank; k++) {
        const int p = params->permute[k];
        if (p < 0 || p >= rank || (seen & (1u << p))) {
            shl_debug_error("mi355x: transpose: permute[%d] = %d is out of range or repeated\n", k, p);
            return CSINN_FALSE;
        }
        seen |= 1u << p;
        if (output->dim[k] != input->dim[p]) {
            shl_debug_error("mi355x: transpose: dim %d of the output is %d, dim %d of the input %d\n", k, output->dim[k], p,
                            input->dim[p]);
            return CSINN_FALSE;
        }
        d->dim[k] = input->dim[k], d->perm[k] = p;
    }
    d->dtype = dtype, d->rank = rank;
    d->in_scale = input->qinfo->scale, d->in_zp = input->qinfo->zero_point;
    d->out_scale = output->qinfo->scale, d->out_zp = output->qinfo->zero_point;
    return CSINN_TRUE;
}

/* ------------------------------------------------------------------------ reshape, flatten */
/* a flat requantised copy of the input's elements: the output must hold as many (the reference copies
 * csinn_tensor_byte_size(input) bytes whatever the output's size) */
static int flat_prepare(const char *op, struct csinn_tensor *input, struct csinn_tensor *output, const void *params,
                        struct move_call *c)
{
    (void)params; /* reshape's and flatten's: the output tensor's dims say it all */
    int dtype;
    int rc = check_io(op, input, output, &dtype);
    if (rc != CSINN_TRUE) return rc;
    const int64_t elems = shl_mi355x_tensor_elems(input);
    if (input->dim_count < 1 || output->dim_count < 1 || elems != shl_mi355x_tensor_elems(output)) {
        shl_debug_error("mi355x: %s: the input holds %lld elements, the output %lld\n", op, (long long)elems,
                        (long long)shl_mi355x_tensor_elems(output));
        return CSINN_FALSE;
    }
    memset(c, 0, sizeof(*c));
    c->kind = MOVE_FLAT;
    c->elems = elems;
    c->d.flat.dtype = dtype;
    c->d.flat.in_scale = input->qinfo->scale, c->d.flat.in_zp = input->qinfo->zero_point;
    c->d.flat.out_scale = output->qinfo->scale, c->d.flat.out_zp = output->qinfo->zero_point;
    return CSINN_TRUE;
}

/* ------------------------------------------------------------------------ pad */
static int pad_prepare(const char *op, struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pad_params *params,
                       struct move_call *c)
{
    int dtype;
    int rc = check_io(op, input, output, &dtype);
    if (rc != CSINN_TRUE) return rc;
    if (params->base.layout != CSINN_LAYOUT_NCHW && params->base.layout != CSINN_LAYOUT_NHWC) return CSINN_UNSUPPORT_LAYOUT;
    if (params->pad_mode != CSINN_PAD_CONSTANT) {
        shl_debug_error("mi355x: pad: mode %d (only CSINN_PAD_CONSTANT is defined)\n", (int)params->pad_mode);
        return CSINN_FALSE;
    }
    if (params->pad_num != 4 || input->dim_count != 4 || output->dim_count != 4 || params->pad_before == NULL ||
        params->pad_after == NULL) {
        shl_debug_error("mi355x: pad expects 4-d tensors and pad_num == 4 (pad_num %d, input %d-d, output %d-d)\n",
                        params->pad_num, input->dim_count, output->dim_count);
        return CSINN_FALSE;
    }
    memset(c, 0, sizeof(*c));
    c->kind = MOVE_PAD;
    struct shl_mi355x_pad_desc *d = &c->d.pad;
    for (int k = 0; k < 4; k++) {
        const int64_t b = params->pad_before[k], a = params->pad_after[k];
        if (b < 0 || a < 0) {
            shl_debug_error("mi355x: pad: negative pad (%lld, %lld) along dim %d\n", (long long)b, (long long)a, k);
            return CSINN_FALSE;
        }
        if ((int64_t)output->dim[k] != (int64_t)input->dim[k] + b + a) {
            shl_debug_error("mi355x: pad: dim %d of the output is %d, expected %lld\n", k, output->dim[k],
                            (long long)(input->dim[k] + b + a));
            return CSINN_FALSE;
        }
        d->dim[k] = input->dim[k], d->before[k] = (int32_t)b, d->after[k] = (int32_t)a;
    }
    d->dtype = dtype;
    d->pad_value = params->pad_value;
    d->in_scale = input->qinfo->scale, d->in_zp = input->qinfo->zero_point;
    d->out_scale = output->qinfo->scale, d->out_zp = output->qinfo->zero_point;
    return CSINN_TRUE;
}

/* init (a refused layer falls through to the reference where there is one), exec and perf around a prepare function */
#define MOVE_OP(name, OP, PARAMS, prepare)                                                                                     \
    int shl_mi355x_##name##_init(struct csinn_tensor *input, struct csinn_tensor *output, struct PARAMS *params)               \
    {                                                                                                                          \
        struct move_call c;                                                                                                    \
        if (prepare(#name, input, output, params, &c) != CSINN_TRUE)                                                           \
            shl_mi355x_fall_through(&params->base, OP, input ? input->dtype : -1);                                             \
        return CSINN_TRUE;                                                                                                     \
    }                                                                                                                          \
    int shl_mi355x_##name##_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct PARAMS *params)               \
    {                                                                                                                          \
        struct move_call c;                                                                                                    \
        int rc = prepare(#name, input, output, params, &c);                                                                    \
        if (rc != CSINN_TRUE) return rc;                                                                                       \
        return move_run(#name, input, output, &params->base, &c);                                                              \
    }                                                                                                                          \
    int shl_mi355x_##name##_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct PARAMS *params,               \
                                 struct csinn_perf_info *info)                                                                 \
    {                                                                                                                          \
        struct move_call c;                                                                                                    \
        int rc = prepare(#name, input, output, params, &c);                                                                    \
        if (rc != CSINN_TRUE) return rc;                                                                                       \
        return move_perf(input, output, &c, info);                                                                             \
    }

MOVE_OP(transpose, CSINN_OP_TRANSPOSE, csinn_transpose_params, transpose_prepare)
MOVE_OP(reshape, CSINN_OP_RESHAPE, csinn_reshape_params, flat_prepare)
MOVE_OP(flatten, CSINN_OP_FLATTEN, csinn_flatten_params, flat_prepare)
MOVE_OP(pad, CSINN_OP_PAD, csinn_pad_params, pad_prepare)


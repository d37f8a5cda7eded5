/*
 * layer.c -- what every layer callback of the MI355X backend shares: the tensor checks, the made-up addresses of the perf
 * callbacks, the fall-through at init and the staging sequence around a launch.
 *
 * A new op's callbacks call them in this order:
 *   prepare (init, exec and perf alike; looks at dims, dtypes and records only, never at `data`):
 *       shl_mi355x_check_tensor   once per tensor, the same *dtype (-1 before the first) through all of them
 *       shl_mi355x_check_dims     where the op takes tensors of any rank
 *       ... the op's own shape rules, then its descriptor of include/shl_mi355x.h
 *   init:  prepare; on a refusal shl_mi355x_fall_through
 *   exec:  prepare; (the op's own "empty output: nothing to do"); shl_mi355x_staged_begin; the launch, a plain call with
 *          s.in[], s.out and s.stream; shl_mi355x_staged_end with the launch's status
 *   perf:  prepare; shl_mi355x_perf_address per tensor from one cursor; the op's *_kernel_name
 * and the op gets one row in the table of setup.c.
 */
#include "mi355x_internal.h"

struct csinn_callback *shl_cb_map_ref(int op, int dtype) __attribute__((weak));

int shl_mi355x_dtype_code(const struct csinn_tensor *t)
{
    if (t->dtype == CSINN_DTYPE_INT8) return SHL_MI355X_I8;
    if (t->dtype == CSINN_DTYPE_FLOAT16) return SHL_MI355X_F16;
    return -1;
}

/* is `t` a tensor the device carries: int8 or binary16 (*dtype: the first tensor's, every later one must match), one
 * quantisation record, binary16 with scale 1 */
int shl_mi355x_check_tensor(const char *op, const char *what, struct csinn_tensor *t, int *dtype)
{
    if (t == NULL) {
        shl_debug_error("mi355x: %s: the %s is missing\n", op, what);
        return CSINN_FALSE;
    }
    const int dt = shl_mi355x_dtype_code(t);
    if (dt < 0 || (*dtype >= 0 && dt != *dtype)) {
        shl_debug_error("mi355x: %s: dtype %d of the %s is unsupported or differs from the other tensors'\n", op, t->dtype, what);
        return CSINN_UNSUPPORT_DTYPE;
    }
    *dtype = dt;
    if (t->qinfo == NULL) {
        shl_debug_error("mi355x: %s: the %s needs a quantisation record\n", op, what);
        return CSINN_FALSE;
    }
    if (t->quant_channel > 1) {
        /* the reference's converters honour per-channel activation records (source/nn2/utils.c:1504-1642); the device
         * path carries one record per activation tensor */
        shl_debug_error("mi355x: %s: per-channel quantised activations are not supported\n", op);
        return CSINN_UNSUPPORT_DTYPE;
    }
    if (dt == SHL_MI355X_F16 && t->qinfo->scale != 1.0f) {
        /* f16_to_float / float_to_f16 scale by qinfo->scale when it differs from 1 (source/nn2/utils.c:1175-1205); not
         * carried to the device */
        shl_debug_error("mi355x: %s fp16 with qinfo scale != 1 is not supported\n", op);
        return CSINN_FALSE;
    }
    return CSINN_TRUE;
}

/* what every device op asks of an (input, output) pair */
int shl_mi355x_check_io(const char *op, struct csinn_tensor *input, struct csinn_tensor *output, int *dtype)
{
    *dtype = -1;
    /* a pair that disagrees on the dtype is CSINN_UNSUPPORT_DTYPE whatever else is wrong with the input */
    if (input && output && shl_mi355x_dtype_code(output) != shl_mi355x_dtype_code(input)) {
        shl_debug_error("mi355x: %s dtypes in=%d out=%d differ\n", op, input->dtype, output->dtype);
        return CSINN_UNSUPPORT_DTYPE;
    }
    int rc = shl_mi355x_check_tensor(op, "input", input, dtype);
    if (rc == CSINN_TRUE) rc = shl_mi355x_check_tensor(op, "output", output, dtype);
    return rc;
}

/* the rank of `t` is min_rank .. MAX_DIM, every extent at least min_extent (0 or 1) and, with max_elems > 0, the element
 * count at most max_elems */
int shl_mi355x_check_dims(const char *op, const char *what, const struct csinn_tensor *t, int min_rank, int min_extent,
                          int64_t max_elems)
{
    if (t->dim_count < min_rank || t->dim_count > MAX_DIM) {
        shl_debug_error("mi355x: %s: the %s has %d dims (%d .. %d)\n", op, what, t->dim_count, min_rank, MAX_DIM);
        return CSINN_FALSE;
    }
    int64_t n = 1;
    for (int k = 0; k < t->dim_count; k++) {
        if (t->dim[k] < min_extent) {
            shl_debug_error("mi355x: %s: dim %d of the %s is %d\n", op, k, what, t->dim[k]);
            return CSINN_FALSE;
        }
        if (max_elems > 0 && (n *= t->dim[k]) > max_elems) {
            shl_debug_error("mi355x: %s: the %s has more than %lld elements\n", op, what, (long long)max_elems);
            return CSINN_FALSE;
        }
    }
    return CSINN_TRUE;
}

/* the product of the extents; a 0-d tensor holds nothing (csinn_tensor_size's rule) */
int64_t shl_mi355x_tensor_elems(const struct csinn_tensor *t)
{
    int64_t n = 1;
    for (int k = 0; k < t->dim_count; k++) n *= t->dim[k];
    return t->dim_count == 0 ? 0 : n;
}

/* a layer this backend refused at init: next to the genuine library it runs on the reference's kernel, elsewhere exec
 * refuses it again (the front-ends drop init's status, source/nn2/split.c:30-35) */
void shl_mi355x_fall_through(struct csinn_params_base *base, int op, int dtype)
{
    if (shl_cb_map_ref && base->cb) {
        struct csinn_callback *cb = shl_cb_map_ref(op, dtype);
        if (cb && cb->exec) base->cb->exec = cb->exec;
    }
}

/* the address a tensor's bytes will have on the device as far as its alignment goes: a DMABUF tensor's own, else a made-up
 * one with the staging path's alignment (disjoint: nothing is staged or followed).  *at: the cursor, SHL_MI355X_PERF_BASE
 * before a layer's first tensor */
uintptr_t shl_mi355x_perf_address(struct csinn_tensor *t, uintptr_t *at)
{
    if (t->mtype == CSINN_MEM_TYPE_DMABUF && t->data) return (uintptr_t)t->data;
    const uintptr_t bytes = (uintptr_t)csinn_tensor_byte_size(t), here = *at;
    *at += (bytes + SHL_MI355X_STAGE_ALIGN - 1) / SHL_MI355X_STAGE_ALIGN * SHL_MI355X_STAGE_ALIGN + SHL_MI355X_STAGE_ALIGN;
    return here;
}

/* stage the inputs (slot 0, and slot 2 for in1 when there is one) and find where the kernel writes (slot 1) */
int shl_mi355x_staged_begin(struct csinn_params_base *base, struct csinn_tensor *in0, struct csinn_tensor *in1,
                            struct csinn_tensor *out, struct shl_mi355x_staged *s)
{
    s->ctx = shl_mi355x_ctx_of(base->sess);
    s->stream = shl_mi355x_ctx_stream(s->ctx);
    s->in[0] = shl_mi355x_stage_in(s->ctx, in0, 0);
    s->in[1] = in1 ? shl_mi355x_stage_in(s->ctx, in1, 2) : NULL;
    s->out = shl_mi355x_stage_out_begin(s->ctx, out, 1);
    return s->in[0] != NULL && (in1 == NULL || s->in[1] != NULL) && s->out != NULL ? CSINN_TRUE : CSINN_FALSE;
}

/* `status`: the launch's; fetches the output of a launch that went well */
int shl_mi355x_staged_end(const char *op, struct shl_mi355x_staged *s, struct csinn_tensor *out, int status)
{
    if (status != SHL_MI355X_OK) {
        shl_debug_error("mi355x: %s failed (%d): %s\n", op, status, shl_mi355x_last_error());
        return CSINN_FALSE;
    }
    return shl_mi355x_stage_out_end(s->ctx, out, s->out);
}

/*
 * resize.c -- the resize callback of the MI355X backend: the upsample of an FPN top-down path, a U-Net decoder, a YOLO
 * neck, so that detection and segmentation graphs stay inside a session's single hipGraph.
 *
 * exec(input, output, params) with the reference's signature (source/reference/resize.c:464-468).  The output size is the
 * OUTPUT tensor's; the two scales are computed here, once, as the reference computes them -- one float division each --
 * and travel to the kernel by value (csrc/resize.hip).  int8 nearest-neighbour is a gather of requantised bytes: with one
 * record per tensor the output byte is a function of the input byte, so the 256 results are built on the host with the
 * reference's own formula and the device only looks up.
 */
#include <math.h>
#include <string.h>

#include "mi355x_internal.h"

float shl_mi355x_resize_scale(int32_t in, int32_t out, int align_corners)
{
    /* resize.c:37-43: (float)int / int -- the divisor is converted too, ONE rounding in the division */
    return align_corners ? (float)(in - 1) / (float)(out - 1) : (float)in / (float)out;
}

/* table[(uint8_t)q] = float_to_int8_base(int8_to_float_base(q)) (source/nn2/utils.c:499-502, 550-560) */
void shl_mi355x_resize_table_i8(float in_scale, int32_t in_zp, float out_scale, int32_t out_zp, uint8_t table[256])
{
    for (int q = -128; q < 128; q++) {
        const float x = ((float)q - in_zp) * in_scale;
        const float ret = nearbyint(x / out_scale) + out_zp;
        int8_t r;
        if (ret > 127) r = 127;
        else if (ret < -128) r = -128;
        else r = (int8_t)ret;
        table[(uint8_t)q] = (uint8_t)r;
    }
}

/* the descriptor of the layer, or why there is none; nothing is staged or written before this has passed */
static int resize_desc(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_resize_params *params,
                       struct shl_mi355x_resize_desc *desc)
{
    int dtype;
    if (input->dtype == CSINN_DTYPE_INT8) dtype = SHL_MI355X_I8;
    else if (input->dtype == CSINN_DTYPE_FLOAT16) dtype = SHL_MI355X_F16;
    else dtype = -1;
    if (dtype < 0 || output->dtype != input->dtype) {
        shl_debug_error("mi355x: resize dtypes in=%d out=%d unsupported\n", input->dtype, output->dtype);
        return CSINN_UNSUPPORT_DTYPE;
    }
    if (input->qinfo == NULL || output->qinfo == NULL) {
        shl_debug_error("mi355x: resize needs quantisation records\n");
        return CSINN_FALSE;
    }
    if (input->quant_channel > 1 || output->quant_channel > 1) {
        shl_debug_error("mi355x: resize: per-channel quantised activations are not supported\n");
        return CSINN_UNSUPPORT_DTYPE;
    }
    if (dtype == SHL_MI355X_F16 && (input->qinfo->scale != 1.0f || output->qinfo->scale != 1.0f)) {
        shl_debug_error("mi355x: resize fp16 with qinfo scale != 1 is not supported\n");
        return CSINN_FALSE;
    }
    if (input->dim_count != 4 || output->dim_count != 4) {
        shl_debug_error("mi355x: resize expects 4-d tensors\n");
        return CSINN_FALSE;
    }
    struct shl_mi355x_resize_desc d;
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
        shl_debug_error("mi355x: resize: batch / channels of input and output differ\n");
        return CSINN_FALSE;
    }
    if (params->resize_mode == CSINN_RESIZE_BILINEAR) d.mode = SHL_MI355X_RESIZE_BILINEAR;
    else if (params->resize_mode == CSINN_RESIZE_NEAREST_NEIGHBOR) d.mode = SHL_MI355X_RESIZE_NEAREST;
    else {
        shl_debug_error("mi355x: resize mode %d is not supported (nearest neighbour and bilinear are)\n", (int)params->resize_mode);
        return CSINN_FALSE;
    }
    d.align_corners = params->align_corners ? 1 : 0;
    if (d.in_h < 1 || d.in_w < 1) {
        shl_debug_error("mi355x: resize: an input without pixels\n");
        return CSINN_FALSE;
    }
    if (d.align_corners && (d.out_h == 1 || d.out_w == 1)) {
        shl_debug_error("mi355x: resize: align_corners with an output extent of 1 (the reference divides by zero)\n");
        return CSINN_FALSE;
    }
    d.dtype = dtype;
    d.n = input->dim[0];
    if (d.out_h > 0 && d.out_w > 0) {
        d.height_scale = shl_mi355x_resize_scale(d.in_h, d.out_h, d.align_corners);
        d.width_scale = shl_mi355x_resize_scale(d.in_w, d.out_w, d.align_corners);
    }
    d.in_scale = input->qinfo->scale, d.in_zp = input->qinfo->zero_point;
    d.out_scale = output->qinfo->scale, d.out_zp = output->qinfo->zero_point;
    if (dtype == SHL_MI355X_I8 && d.mode == SHL_MI355X_RESIZE_NEAREST)
        shl_mi355x_resize_table_i8(d.in_scale, d.in_zp, d.out_scale, d.out_zp, d.table);
    *desc = d;
    return CSINN_TRUE;
}

int shl_mi355x_resize_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_resize_params *params)
{
    struct shl_mi355x_resize_desc d;
    int rc = resize_desc(input, output, params, &d);
    if (rc != CSINN_TRUE) return rc;
    if (csinn_tensor_size(output) == 0) return CSINN_TRUE;
    struct shl_mi355x_ctx *ctx = shl_mi355x_ctx_of(params->base.sess);
    const void *in_dev = shl_mi355x_stage_in(ctx, input, 0);
    void *out_dev = shl_mi355x_stage_out_begin(ctx, output, 1);
    if (in_dev == NULL || out_dev == NULL) return CSINN_FALSE;
    int st = shl_mi355x_resize(in_dev, out_dev, &d, shl_mi355x_ctx_stream(ctx));
    if (st != SHL_MI355X_OK) {
        shl_debug_error("mi355x: resize failed (%d): %s\n", st, shl_mi355x_last_error());
        return CSINN_FALSE;
    }
    return shl_mi355x_stage_out_end(ctx, output, out_dev);
}

/* the address a tensor's bytes will have on the device as far as its alignment goes: a DMABUF tensor's own, the staging
 * buffers' alignment for a host tensor (made-up, disjoint: nothing is staged or followed) */
static const void *perf_address(struct csinn_tensor *t, int slot)
{
    if (t->mtype == CSINN_MEM_TYPE_DMABUF && t->data) return t->data;
    return (const void *)(((uintptr_t)1 << 56) + ((uintptr_t)slot << 48));
}

int shl_mi355x_resize_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_resize_params *params,
                           struct csinn_perf_info *info)
{
    struct shl_mi355x_resize_desc d;
    int rc = resize_desc(input, output, params, &d);
    if (rc != CSINN_TRUE) return rc;
    info->kernel_name = (char *)shl_mi355x_resize_kernel_name(&d, perf_address(input, 0), perf_address(output, 1));
    return CSINN_TRUE;
}

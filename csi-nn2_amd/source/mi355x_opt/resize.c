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
    int rc = shl_mi355x_check_io("resize", input, output, &dtype);
    if (rc != CSINN_TRUE) return rc;
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
    struct shl_mi355x_staged s;
    if (shl_mi355x_staged_begin(&params->base, input, NULL, output, &s) != CSINN_TRUE) return CSINN_FALSE;
    int st = shl_mi355x_resize(s.in[0], s.out, &d, s.stream);
    return shl_mi355x_staged_end("resize", &s, output, st);
}

int shl_mi355x_resize_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_resize_params *params,
                           struct csinn_perf_info *info)
{
    struct shl_mi355x_resize_desc d;
    int rc = resize_desc(input, output, params, &d);
    if (rc != CSINN_TRUE) return rc;
    uintptr_t at = SHL_MI355X_PERF_BASE;
    const void *in = (const void *)shl_mi355x_perf_address(input, &at);
    info->kernel_name = (char *)shl_mi355x_resize_kernel_name(&d, in, (const void *)shl_mi355x_perf_address(output, &at));
    return CSINN_TRUE;
}

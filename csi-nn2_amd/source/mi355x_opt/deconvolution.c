/*
 * deconvolution.c -- init / exec / perf callbacks of the MI355X backend for the transposed convolution
 * (CSINN_OP_DECONV2D, CSINN_OP_DEPTHWISE_DECONV2D; int8 and fp16, NHWC and NCHW): the learned upsampling of a U-Net / FCN
 * decoder, pix2pix, DCGAN, FSRCNN, so that such a model stays inside a session's single hipGraph.
 *
 * init  translates tensors + params into the C-ABI descriptor (in_* / out_* are the deconvolution's own), derives the
 *       per-output-channel tables with convolution.c's rules (fuse_zp2bias is never read by the reference's deconvolution:
 *       off) and creates the plan (shl_mi355x_deconv_plan_create, csrc/deconv.hip).
 * exec  shl_mi355x_run_plan: host staging, DMABUF tensors, SHL_MI355X_TRACE_EXEC as for every convolution.
 * Reference: shl_ref_deconv2d_quant / shl_ref_depthwise_deconv2d_quant (source/reference/deconvolution.c:334-369), i.e.
 * shl_ref_conv_callback_base (utils.c:639-655) around the fp32 scatter.  Per-channel kernel records are applied along the
 * kernel tensor's dim 0 (source/nn2/utils.c): the output channel for [O,Kh,Kw,I] and both depthwise layouts -- they fold
 * into mult[oc] -- but the INPUT channel for the NCHW group-1 kernel [I,O,Kh,Kw], which no per-output-channel epilogue can
 * express: refused.
 */
#include <stdlib.h>
#include <string.h>

#include "mi355x_internal.h"

static int refuse(struct csinn_conv2d_params *params, int op, int dtype, int rc)
{
    /* csinn_deconv2d_init drops this status (source/nn2/deconvolution.c:41-45), so the callback itself must not stay: next
     * to the genuine library the layer runs on the reference's kernel, elsewhere exec finds no plan and fails */
    shl_mi355x_release_params(params);
    shl_mi355x_fall_through(&params->base, op, dtype);
    return rc;
}

static int deconv_init_act(CSINN_CONV_ARGS, int act)
{
    const int nhwc = params->base.layout == CSINN_LAYOUT_NHWC, nchw = params->base.layout == CSINN_LAYOUT_NCHW;
    const int group = params->group > 0 ? params->group : 1;
    const int cin = input->dim[nhwc ? 3 : 1], cout = output->dim[nhwc ? 3 : 1];
    const int op = group == 1 ? CSINN_OP_DECONV2D : (group == cin ? CSINN_OP_DEPTHWISE_DECONV2D : CSINN_OP_GROUP_DECONV2D);
#define REFUSE(rc, ...)                       \
    do {                                      \
        shl_debug_error(__VA_ARGS__);         \
        return refuse(params, op, input->dtype, rc); \
    } while (0)
    if (!nhwc && !nchw) REFUSE(CSINN_UNSUPPORT_LAYOUT, "mi355x: deconv2d layout %d unsupported\n", params->base.layout);
    if (input->dim_count != 4 || output->dim_count != 4 || kernel->dim_count != 4)
        REFUSE(CSINN_FALSE, "mi355x: deconv2d expects 4-d tensors\n");
    if (op == CSINN_OP_GROUP_DECONV2D)
        REFUSE(CSINN_FALSE, "mi355x: group_deconv2d (group %d, %d -> %d channels) is not supported\n", group, cin, cout);
    struct shl_mi355x_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.layout = nhwc ? SHL_MI355X_NHWC : SHL_MI355X_NCHW;
    d.dtype = input->dtype == CSINN_DTYPE_INT8 ? SHL_MI355X_I8 : (input->dtype == CSINN_DTYPE_FLOAT16 ? SHL_MI355X_F16 : -1);
    if (d.dtype < 0 || kernel->dtype != input->dtype || output->dtype != input->dtype)
        REFUSE(CSINN_UNSUPPORT_DTYPE, "mi355x: deconv2d dtypes in=%d kernel=%d out=%d unsupported\n", input->dtype, kernel->dtype,
               output->dtype);
    if (kernel->data == NULL || kernel->mtype == CSINN_MEM_TYPE_DMABUF)
        REFUSE(CSINN_FALSE, "mi355x: deconv2d: the kernel tensor must be host resident at init time\n");
    if (input->qinfo == NULL || output->qinfo == NULL || kernel->qinfo == NULL)
        REFUSE(CSINN_FALSE, "mi355x: deconv2d tensors need quantisation records\n");
    if (input->quant_channel > 1 || output->quant_channel > 1)
        REFUSE(CSINN_UNSUPPORT_DTYPE, "mi355x: deconv2d: per-channel quantised activations are not supported\n");
    if (nchw && group == 1 && kernel->quant_channel > 1)
        REFUSE(CSINN_UNSUPPORT_DTYPE, "mi355x: deconv2d: per-channel records of an NCHW [I,O,Kh,Kw] kernel run along the INPUT channel: "
                                      "not supported\n");
    d.act = act;
    d.batch = input->dim[0];
    d.in_h = input->dim[nhwc ? 1 : 2], d.in_w = input->dim[nhwc ? 2 : 3], d.in_c = cin;
    d.out_h = output->dim[nhwc ? 1 : 2], d.out_w = output->dim[nhwc ? 2 : 3], d.out_c = cout;
    d.kernel_h = kernel->dim[nhwc ? 1 : 2], d.kernel_w = kernel->dim[nhwc ? 2 : 3];
    d.stride_h = params->stride_height, d.stride_w = params->stride_width;
    d.pad_top = params->pad_top, d.pad_left = params->pad_left;
    d.dilation_h = params->dilation_height > 0 ? params->dilation_height : 1;
    d.dilation_w = params->dilation_width > 0 ? params->dilation_width : 1;
    d.group = group;
    if (d.dtype == SHL_MI355X_I8) d.in_zp = input->qinfo->zero_point, d.out_zp = output->qinfo->zero_point;
    d.out_scale = output->qinfo->scale;
    /* the kernel's channel counts: [O,Kh,Kw,I] / [I,O,Kh,Kw]; depthwise [1,Kh,Kw,C] / [C,1,Kh,Kw] */
    const int k_out = group == 1 ? kernel->dim[nhwc ? 0 : 1] : kernel->dim[nhwc ? 3 : 0];
    const int k_in = group == 1 ? kernel->dim[nhwc ? 3 : 0] : kernel->dim[nhwc ? 0 : 1];
    if (k_out != cout || k_in != (group == 1 ? cin : 1) || output->dim[0] != input->dim[0])
        REFUSE(CSINN_FALSE, "mi355x: deconv2d: kernel [%d,%d,%d,%d] does not fit %d -> %d channels (group %d)\n", kernel->dim[0],
               kernel->dim[1], kernel->dim[2], kernel->dim[3], cin, cout, group);

    float *mult = shl_mem_alloc((int64_t)cout * sizeof(float));
    float *bias_f = shl_mem_alloc((int64_t)cout * sizeof(float));
    int32_t *kzp = shl_mem_alloc((int64_t)cout * sizeof(int32_t));
    /* (a depthwise NHWC kernel's channel is its last dim; nothing else of that flag is read with fuse_zp2bias off) */
    int rc = shl_mi355x_conv_build_tables(&d, input, kernel, bias, 0, group > 1 && nhwc, mult, bias_f, kzp);
    for (int oc = 0; rc == CSINN_TRUE && oc < cout; oc++)
        if (kzp[oc] != 0) {
            shl_debug_error("mi355x: deconv2d: a kernel zero point (%d at channel %d) is not supported\n", kzp[oc], oc);
            rc = CSINN_UNSUPPORT_DTYPE;
        }
    shl_mi355x_conv_plan *plan = NULL;
    if (rc == CSINN_TRUE) {
        int st = shl_mi355x_deconv_plan_create(&d, kernel->data, mult, bias_f, shl_mi355x_ctx_stream(shl_mi355x_ctx_of(params->base.sess)),
                                               &plan);
        if (st != SHL_MI355X_OK) {
            shl_debug_error("mi355x: deconv2d plan creation failed (%d): %s\n", st, shl_mi355x_last_error());
            rc = st == SHL_MI355X_ENOTSUP ? CSINN_UNSUPPORT_LAYOUT : CSINN_FALSE;
        }
    }
    shl_mem_free(mult);
    shl_mem_free(bias_f);
    shl_mem_free(kzp);
    if (rc != CSINN_TRUE) return refuse(params, op, input->dtype, rc);
#undef REFUSE
    shl_mi355x_registry_put(params, plan);
    params->base.cb->exec = shl_mi355x_deconv2d_exec;
    return CSINN_TRUE;
}

int shl_mi355x_deconv2d_init(CSINN_CONV_ARGS) { return deconv_init_act(input, output, kernel, bias, params, SHL_MI355X_ACT_NONE); }

int shl_mi355x_deconv2d_exec(CSINN_CONV_ARGS)
{
    (void)kernel;
    (void)bias;
    return shl_mi355x_run_plan(&params->base, input, output, input->dim[0], "deconv2d");
}

/* session.c:plan_fusion: deconv2d -> relu | relu6, the deconvolution's only consumer, same output record (what every
 * decoder emits): the activation moves into the deconvolution's epilogue.  `output` is the ACTIVATION's output tensor.
 * Replaces the plan under `params` on success; on failure the old plan stays. */
int shl_mi355x_deconv2d_fold_activation(struct csinn_tensor *input, struct csinn_tensor *deconv_output,
                                        struct csinn_tensor *output, struct csinn_tensor *kernel, struct csinn_tensor *bias,
                                        struct csinn_conv2d_params *params, int relu6)
{
    shl_mi355x_conv_plan *old = shl_mi355x_registry_get(params);
    if (old == NULL || !shl_mi355x_activation_folds(deconv_output, output)) return CSINN_FALSE;
    /* (a refused re-init would drop the plan: the same descriptor with another activation cannot be refused) */
    return deconv_init_act(input, output, kernel, bias, params, relu6 ? SHL_MI355X_ACT_RELU6 : SHL_MI355X_ACT_RELU);
}

int shl_mi355x_deconv2d_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_tensor *kernel,
                             struct csinn_tensor *bias, struct csinn_conv2d_params *params, struct csinn_perf_info *info)
{
    (void)input; (void)output; (void)kernel; (void)bias;
    info->kernel_name = (char *)shl_mi355x_params_kernel_name(params); /* the plan's: "deconv_phase_*" or "deconv_gather_*" */
    return CSINN_TRUE;
}

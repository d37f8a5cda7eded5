/* mi355x_internal.h -- private glue of the source/mi355x_opt backend. */
#ifndef MI355X_INTERNAL_H_
#define MI355X_INTERNAL_H_

#include "shl_mi355x.h"
#include "shl_mi355x_backend.h"

/* params-block -> device plan association (struct csinn_fc_params has no spare pointer, so a
 * side table serves every op uniformly); grouped convolutions keep one plan per group */
void shl_mi355x_registry_put(void *params, shl_mi355x_conv_plan *plan);
void shl_mi355x_registry_put_group(void *params, shl_mi355x_conv_plan **plans, int n); /* takes the array */
shl_mi355x_conv_plan *shl_mi355x_registry_get(void *params);
shl_mi355x_conv_plan *shl_mi355x_registry_get_group(void *params, int i);
/* a fingerprint of what the plan under `params` was built from, stored WITH the plan (released with it) */
void shl_mi355x_registry_set_tag(void *params, const void *tag, size_t bytes);
int shl_mi355x_registry_tag_matches(void *params, const void *tag, size_t bytes);

/* Per-session execution context: the stream exec callbacks enqueue on and the session's own HBM
 * staging buffers (setup.c).  ctx_of(NULL) is the context of session-less calls. */
struct shl_mi355x_ctx;
struct shl_mi355x_ctx *shl_mi355x_ctx_of(struct csinn_session *sess);
void *shl_mi355x_ctx_stream(struct shl_mi355x_ctx *ctx);
void shl_mi355x_ctx_release(struct csinn_session *sess);

/* Host <-> HBM staging for tensors that do not already live on the device.
 * slot: 0 = first input, 1 = output, 2 = second input.
 *   stage_in        device address holding the tensor's bytes (uploads host tensors)
 *   stage_out_begin device address the kernel should write
 *   stage_out_end   downloads + synchronises for host tensors; CSINN_TRUE on success */
const void *shl_mi355x_stage_in(struct shl_mi355x_ctx *ctx, struct csinn_tensor *t, int slot);
void *shl_mi355x_stage_out_begin(struct shl_mi355x_ctx *ctx, struct csinn_tensor *t, int slot);
int shl_mi355x_stage_out_end(struct shl_mi355x_ctx *ctx, struct csinn_tensor *t, void *dev);
/* n inputs at once (concat): host tensors are packed into staging slot 0 at 256-byte-aligned offsets and uploaded on the
 * context's stream, DMABUF tensors are used in place, tensors of zero elements get NULL; dev[i]: where tensor i lives.
 * SHL_MI355X_STAGE_ALIGN is that alignment, for callers that predict a kernel form before anything is staged */
#define SHL_MI355X_STAGE_ALIGN 256
int shl_mi355x_stage_in_many(struct shl_mi355x_ctx *ctx, struct csinn_tensor **t, int n, const void **dev);

/* n outputs at once (split): host tensors are packed into staging slot 1 at the same alignment, DMABUF tensors are written
 * in place; _end downloads the host tensors and synchronises once */
int shl_mi355x_stage_out_many_begin(struct shl_mi355x_ctx *ctx, struct csinn_tensor **t, int n, void **dev);
int shl_mi355x_stage_out_many_end(struct shl_mi355x_ctx *ctx, struct csinn_tensor **t, int n, void *const *dev);

/* perf callbacks of the windowed pools (pooling.c): single-input signature + the trailing info block */
int shl_mi355x_maxpool2d_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pool_params *params,
                              struct csinn_perf_info *info);
int shl_mi355x_avgpool2d_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pool_params *params,
                              struct csinn_perf_info *info);

/* ... and of concat: the array-of-inputs signature */
int shl_mi355x_concat_perf(struct csinn_tensor **input, struct csinn_tensor *output, struct csinn_concat_params *params,
                           struct csinn_perf_info *info);

/* split and shuffle_channel (split.c): init (a refused layer falls through to the reference where there is one) and perf */
int shl_mi355x_split_init(struct csinn_tensor *input, struct csinn_tensor **output, struct csinn_split_params *params);
int shl_mi355x_split_perf(struct csinn_tensor *input, struct csinn_tensor **output, struct csinn_split_params *params,
                          struct csinn_perf_info *info);
int shl_mi355x_shuffle_channel_init(struct csinn_tensor *input, struct csinn_tensor *output,
                                    struct csinn_shuffle_channel_params *params);
int shl_mi355x_shuffle_channel_perf(struct csinn_tensor *input, struct csinn_tensor *output,
                                    struct csinn_shuffle_channel_params *params, struct csinn_perf_info *info);

/* shared by the callbacks of the ops that move data (split.c, move.c).  check_io: dtypes and records, what every device op
 * asks of an (input, output) pair.  fall_through: a layer refused at init runs on the reference's kernel next to the genuine
 * library (elsewhere exec refuses it again: the front-ends drop init's status).  perf_address: the address a tensor's bytes
 * will have on the device as far as its alignment goes -- a DMABUF tensor's own, else a made-up one with the staging path's
 * alignment */
int shl_mi355x_check_io(const char *op, struct csinn_tensor *input, struct csinn_tensor *output, int *dtype);
void shl_mi355x_fall_through(struct csinn_params_base *base, int op, int dtype);
uintptr_t shl_mi355x_perf_address(struct csinn_tensor *t, uintptr_t *at);

/* transpose, reshape, flatten and pad (move.c): init (a refused layer falls through to the reference where there is one)
 * and perf */
int shl_mi355x_transpose_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_transpose_params *params);
int shl_mi355x_transpose_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_transpose_params *params,
        struct csinn_perf_info *info);
int shl_mi355x_reshape_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reshape_params *params);
int shl_mi355x_reshape_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reshape_params *params,
        struct csinn_perf_info *info);
int shl_mi355x_flatten_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_flatten_params *params);
int shl_mi355x_flatten_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_flatten_params *params,
        struct csinn_perf_info *info);
int shl_mi355x_pad_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pad_params *params);
int shl_mi355x_pad_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pad_params *params,
        struct csinn_perf_info *info);

/* the reductions (reduce.c): init (a refused layer falls through to the reference where there is one) and perf */
int shl_mi355x_mean_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_mean_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params,
        struct csinn_perf_info *info);
int shl_mi355x_sum_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_sum_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params,
        struct csinn_perf_info *info);
int shl_mi355x_max_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_max_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params,
        struct csinn_perf_info *info);
int shl_mi355x_min_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_min_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params,
        struct csinn_perf_info *info);
int shl_mi355x_reduce_mean_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_reduce_mean_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params,
        struct csinn_perf_info *info);
int shl_mi355x_reduce_sum_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_reduce_sum_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params,
        struct csinn_perf_info *info);
int shl_mi355x_reduce_max_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_reduce_max_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params,
        struct csinn_perf_info *info);
int shl_mi355x_reduce_min_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_reduce_min_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params,
        struct csinn_perf_info *info);
int shl_mi355x_global_maxpool2d_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pool_params *params);
int shl_mi355x_global_maxpool2d_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pool_params *params,
        struct csinn_perf_info *info);

/* matmul (matmul.c): init (a refused layer falls through to the reference where there is one) and perf */
int shl_mi355x_matmul_init(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
        struct csinn_matmul_params *params);
int shl_mi355x_matmul_perf(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
        struct csinn_matmul_params *params, struct csinn_perf_info *info);

/* ... and of the elementwise layers (eltwise.c): the kernel form the rules choose */
int shl_mi355x_sigmoid_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params,
                            struct csinn_perf_info *info);
int shl_mi355x_hard_sigmoid_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params,
                                 struct csinn_perf_info *info);
int shl_mi355x_silu_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params,
                         struct csinn_perf_info *info);
int shl_mi355x_leaky_relu_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_relu_params *params,
                               struct csinn_perf_info *info);
int shl_mi355x_mul_perf(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                        struct csinn_diso_params *params, struct csinn_perf_info *info);

/* ... and of resize (resize.c) */
int shl_mi355x_resize_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_resize_params *params,
                           struct csinn_perf_info *info);

float shl_mi355x_half_to_float(uint16_t h);

/* session.c: fold the relu / relu6 layer that is the convolution's only consumer into its plan (convolution.c) */
int shl_mi355x_conv2d_fold_activation(struct csinn_tensor *input, struct csinn_tensor *conv_output,
                                      struct csinn_tensor *output, struct csinn_tensor *kernel, struct csinn_tensor *bias,
                                      struct csinn_conv2d_params *params, int relu6);
int shl_mi355x_conv2d_relu_init(CSINN_CONV_ARGS);
int shl_mi355x_conv2d_relu6_init(CSINN_CONV_ARGS);
/* ... the conditions of that fold (same dims, same record; binary16: scale 1), and the same fold for a transposed convolution
 * (deconvolution.c) */
int shl_mi355x_activation_folds(struct csinn_tensor *conv_output, struct csinn_tensor *output);
int shl_mi355x_deconv2d_fold_activation(struct csinn_tensor *input, struct csinn_tensor *deconv_output,
                                        struct csinn_tensor *output, struct csinn_tensor *kernel, struct csinn_tensor *bias,
                                        struct csinn_conv2d_params *params, int relu6);

/* convolution.c, shared with deconvolution.c: the per-output-channel fp32 tables of the numerical contract from the tensors'
 * records (dw_weights_last: the kernel's channel is its LAST dim), and exec of the plan registered under `base` (host
 * staging, DMABUF tensors, SHL_MI355X_TRACE_EXEC) */
int shl_mi355x_conv_build_tables(const struct shl_mi355x_conv_desc *d, struct csinn_tensor *input, struct csinn_tensor *kernel,
                                 struct csinn_tensor *bias, int fuse_zp2bias, int dw_weights_last, float *mult, float *bias_f,
                                 int32_t *kzp);
int shl_mi355x_run_plan(struct csinn_params_base *base, struct csinn_tensor *input, struct csinn_tensor *output, int batch,
                        const char *what);
int shl_mi355x_deconv2d_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_tensor *kernel,
                             struct csinn_tensor *bias, struct csinn_conv2d_params *params, struct csinn_perf_info *info);

#endif /* MI355X_INTERNAL_H_ */

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

/* ------------------------------------------------------------------------ layer.c: what every layer callback shares
 * (the order to call them in is at the top of that file) */
int shl_mi355x_dtype_code(const struct csinn_tensor *t); /* SHL_MI355X_I8 / _F16, or -1 */
/* one tensor: int8 or binary16, one quantisation record, binary16 with scale 1.  *dtype < 0: the layer's first tensor, which
 * sets it; every later tensor must match.  check_io: an (input, output) pair */
int shl_mi355x_check_tensor(const char *op, const char *what, struct csinn_tensor *t, int *dtype);
int shl_mi355x_check_io(const char *op, struct csinn_tensor *input, struct csinn_tensor *output, int *dtype);
/* rank min_rank .. MAX_DIM, extents of at least min_extent (0 or 1), at most max_elems elements (0: any number: the ops
 * that only move data count in 64 bits).  SHL_MI355X_INT32_ELEMS: for descriptors that index with 32 bits */
#define SHL_MI355X_INT32_ELEMS 0x7FFFFFFFll
int shl_mi355x_check_dims(const char *op, const char *what, const struct csinn_tensor *t, int min_rank, int min_extent,
                          int64_t max_elems);
int64_t shl_mi355x_tensor_elems(const struct csinn_tensor *t); /* 0-d: 0 */
/* fall_through: a layer refused at init runs on the reference's kernel next to the genuine library (elsewhere exec refuses
 * it again: the front-ends drop init's status).  perf_address: the address a tensor's bytes will have on the device as far
 * as its alignment goes -- a DMABUF tensor's own, else a made-up one with the staging path's alignment; `at` is a cursor
 * that starts at SHL_MI355X_PERF_BASE and runs through the layer's tensors */
void shl_mi355x_fall_through(struct csinn_params_base *base, int op, int dtype);
#define SHL_MI355X_PERF_BASE ((uintptr_t)1 << 56)
uintptr_t shl_mi355x_perf_address(struct csinn_tensor *t, uintptr_t *at);
/* the staging sequence around a launch: begin stages in0 (slot 0), in1 (slot 2; may be NULL) and finds the output's address
 * (slot 1); the launch is the caller's own call on s.in[], s.out, s.stream; end reports a failed launch ("<op> failed (status):
 * message") or fetches the output.  Both return CSINN_TRUE or CSINN_FALSE */
struct shl_mi355x_staged {
    struct shl_mi355x_ctx *ctx;
    void *stream;
    const void *in[2];
    void *out;
};
int shl_mi355x_staged_begin(struct csinn_params_base *base, struct csinn_tensor *in0, struct csinn_tensor *in1,
                            struct csinn_tensor *out, struct shl_mi355x_staged *s);
int shl_mi355x_staged_end(const char *op, struct shl_mi355x_staged *s, struct csinn_tensor *out, int status);

/* ------------------------------------------------------------------------ the operator table (setup.c)
 * how an exec callback is called.  The value is the number of inputs such a layer has in the graph (kernel and bias
 * included); 0: as many as its params block says; < 0: see inputs_of (session.c) */
enum call_shape {
    CALL_NONE = -2,  /* no session row: a session with such a layer stays host-staged */
    CALL_SPLIT = -1, /* exec(input, outputs[], params): one input, as many outputs as its params block says */
    CALL_ARRAY = 0,  /* exec(inputs[], output, params) */
    CALL_SISO = 1,   /* exec(input, output, params) */
    CALL_DISO = 2,   /* exec(input0, input1, output, params) */
    CALL_CONV = 3,   /* exec(input, output, kernel, bias, params) */
};

/* All the backend knows about an operator, one row per op id: what shl_target_init_mi355x registers for it, and what a
 * session needs to run it on the device */
struct shl_mi355x_op {
    int type;
    unsigned dtypes; /* SHL_MI355X_OP_I8 | SHL_MI355X_OP_F16 */
    void *init, *exec, *est, *perf;
    enum call_shape call;
    int activations; /* the leading inputs that are activations; 0: all of them */
    int first_const; /* of those, the ones from this index on may be constants instead: uploaded once, kept resident */
};
#define SHL_MI355X_OP_I8 1u
#define SHL_MI355X_OP_F16 2u
const struct shl_mi355x_op *shl_mi355x_op_row(int type); /* NULL: not an op of this backend */

/* ------------------------------------------------------------------------ init and perf callbacks, for the table
 * (the exec callbacks are public: shl_mi355x_backend.h).  An init of these files refuses nothing: a layer it would refuse
 * falls through to the reference where there is one.  perf reports the kernel form the rules choose */
#define SISO_INIT(name, PARAMS) \
    int shl_mi355x_##name##_init(struct csinn_tensor *input, struct csinn_tensor *output, struct PARAMS *params);
#define SISO_PERF(name, PARAMS)                                                                                  \
    int shl_mi355x_##name##_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct PARAMS *params, \
                                 struct csinn_perf_info *info);
/* pooling.c, eltwise.c, resize.c */
SISO_PERF(maxpool2d, csinn_pool_params)
SISO_PERF(avgpool2d, csinn_pool_params)
SISO_PERF(sigmoid, csinn_sigmoid_params)
SISO_PERF(hard_sigmoid, csinn_sigmoid_params)
SISO_PERF(silu, csinn_sigmoid_params)
SISO_PERF(leaky_relu, csinn_relu_params)
SISO_PERF(resize, csinn_resize_params)
/* split.c */
SISO_INIT(shuffle_channel, csinn_shuffle_channel_params)
SISO_PERF(shuffle_channel, csinn_shuffle_channel_params)
/* move.c */
SISO_INIT(transpose, csinn_transpose_params)
SISO_PERF(transpose, csinn_transpose_params)
SISO_INIT(reshape, csinn_reshape_params)
SISO_PERF(reshape, csinn_reshape_params)
SISO_INIT(flatten, csinn_flatten_params)
SISO_PERF(flatten, csinn_flatten_params)
SISO_INIT(pad, csinn_pad_params)
SISO_PERF(pad, csinn_pad_params)
/* reduce.c */
SISO_INIT(mean, csinn_reduce_params)
SISO_PERF(mean, csinn_reduce_params)
SISO_INIT(sum, csinn_reduce_params)
SISO_PERF(sum, csinn_reduce_params)
SISO_INIT(max, csinn_reduce_params)
SISO_PERF(max, csinn_reduce_params)
SISO_INIT(min, csinn_reduce_params)
SISO_PERF(min, csinn_reduce_params)
SISO_INIT(reduce_mean, csinn_reduce_params)
SISO_PERF(reduce_mean, csinn_reduce_params)
SISO_INIT(reduce_sum, csinn_reduce_params)
SISO_PERF(reduce_sum, csinn_reduce_params)
SISO_INIT(reduce_max, csinn_reduce_params)
SISO_PERF(reduce_max, csinn_reduce_params)
SISO_INIT(reduce_min, csinn_reduce_params)
SISO_PERF(reduce_min, csinn_reduce_params)
SISO_INIT(global_maxpool2d, csinn_pool_params)
SISO_PERF(global_maxpool2d, csinn_pool_params)
#undef SISO_INIT
#undef SISO_PERF
/* the other call shapes: mul (eltwise.c), add (pooling.c), matmul (matmul.c), concat (pooling.c), split (split.c) */
int shl_mi355x_mul_perf(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                        struct csinn_diso_params *params, struct csinn_perf_info *info);
int shl_mi355x_add_perf(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                        struct csinn_diso_params *params, struct csinn_perf_info *info);
/* eltwise.c: the broadcast geometry of a two-operand layer (`op`: "mul" / "add", for the messages): which operand has the
 * output's shape, which is broadcast to it, and the descriptor of the pair; refuses with a message what the kernels do not take */
int shl_mi355x_bcast_prepare(const char *op, struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                             struct csinn_tensor **full, struct csinn_tensor **small, struct shl_mi355x_mul_desc *desc);
int shl_mi355x_matmul_init(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
                           struct csinn_matmul_params *params);
int shl_mi355x_matmul_perf(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
                           struct csinn_matmul_params *params, struct csinn_perf_info *info);
/* matmul.c, for session.c: a matmul layer and the add of a constant bias behind it as one launch on device buffers */
int shl_mi355x_matmul_bias_forward(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *mid,
                                   struct csinn_tensor *bias, struct csinn_tensor *output, struct csinn_matmul_params *params,
                                   int bias_is_first, const void *a_dev, const void *b_dev, const void *bias_dev, void *out_dev,
                                   void *stream);
/* attention.c, for session.c: matmul(q, k, trans_b) -> [mul by the one-element constant c, output sc] -> softmax (output p) ->
 * matmul(p, v) as one descriptor (prepare: CSINN_TRUE when shl_mi355x_attention takes it and, unless `force`, fuses it by
 * default) and as one launch on device buffers */
int shl_mi355x_attention_prepare(struct csinn_tensor *q, struct csinn_tensor *k, struct csinn_tensor *s,
                                 struct csinn_matmul_params *qk_params, struct csinn_tensor *c, struct csinn_tensor *sc,
                                 int const_first, struct csinn_tensor *p, int axis, struct csinn_tensor *v,
                                 struct csinn_tensor *out, struct csinn_matmul_params *pv_params, int force,
                                 struct shl_mi355x_attention_desc *d);
int shl_mi355x_attention_forward(const struct shl_mi355x_attention_desc *d, const void *q_dev, const void *k_dev, const void *v_dev,
                                 void *out_dev, void *stream);
/* ... and the same chain with a broadcasting add (layer tensors in0, in1, sum; x: the chain's own operand of it) between the
 * [scaled] scores and the softmax: the add's part of the descriptor, and the launch (shl_mi355x_attention_bias) */
int shl_mi355x_attention_bias_prepare(struct csinn_tensor *in0, struct csinn_tensor *in1, struct csinn_tensor *sum,
                                      struct csinn_tensor *x, const struct shl_mi355x_attention_desc *d, int force,
                                      struct shl_mi355x_attention_bias_desc *bd);
int shl_mi355x_attention_bias_forward(const struct shl_mi355x_attention_desc *d, const struct shl_mi355x_attention_bias_desc *bd,
                                      const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev, void *out_dev,
                                      void *stream);
/* ... and either chain on operands where the projections left them (shl_mi355x_attention_layout; bd NULL: without a bias) */
int shl_mi355x_attention_layout_forward(const struct shl_mi355x_attention_desc *d, const struct shl_mi355x_attention_bias_desc *bd,
                                        const struct shl_mi355x_attention_layout_desc *ld, const void *q_dev, const void *k_dev,
                                        const void *v_dev, const void *bias_dev, void *out_dev, void *stream);
int shl_mi355x_concat_perf(struct csinn_tensor **input, struct csinn_tensor *output, struct csinn_concat_params *params,
                           struct csinn_perf_info *info);
int shl_mi355x_split_init(struct csinn_tensor *input, struct csinn_tensor **output, struct csinn_split_params *params);
int shl_mi355x_split_perf(struct csinn_tensor *input, struct csinn_tensor **output, struct csinn_split_params *params,
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

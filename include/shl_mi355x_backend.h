/*
 * shl_mi355x_backend.h -- public surface of the source/mi355x_opt backend (host C code).
 *
 * The backend plugs into the CSI-NN2 front-end through the two registration calls of
 * include/shl_utils.h (reference: source/nn2/setup.c:98-99,127-129), exactly like the
 * reference's own optimised backends do (pattern: source/c920v2_opt/setup.c:391-413):
 *
 *     shl_target_init_mi355x();            // once, after the first csinn_alloc_session()
 *     params->base.api = CSINN_MI355X;     // or sess->base_api for graph mode
 *     csinn_conv2d_init(...); csinn_conv2d(...);
 *
 * Tensors may live on the host (any mtype except DMABUF: the backend stages them through HBM
 * and synchronises before returning) or in HBM (mtype == CSINN_MEM_TYPE_DMABUF: `data` is a
 * device pointer, nothing is copied and nothing synchronises -- this is the mode bench.py
 * measures).
 */
#ifndef SHL_MI355X_BACKEND_H_
#define SHL_MI355X_BACKEND_H_

#include "shl_gref.h"

#ifdef __cplusplus
extern "C" {
#endif

/* registers the op map and the runtime map in slot CSINN_MI355X */
void shl_target_init_mi355x(void);
/* ... and in one more slot `api` (also: environment SHL_MI355X_SLOT=<api> at shl_target_init_mi355x time), so that a
 * program that hard-codes another target's slot -- example/c906_mobilenetv1_f16.c:24 uses CSINN_C906 -- dispatches
 * to this backend unchanged.  CSINN_REF / CSINN_GREF are refused.  CSINN_TRUE on success */
int shl_target_init_mi355x_slot(int api);
struct csinn_callback *shl_cb_map_mi355x(int op, int dtype);
void *shl_mi355x_runtime_callback(int runtime_op);

/* Streams.  Every csinn session (layer-mode sessions included) has its own execution context: the
 * HIP stream its exec callbacks enqueue on and its own HBM staging buffers, so two sessions never race
 * (SURVEY 8b "Threading": serialise per session).  shl_mi355x_session_set_stream binds an opaque
 * hipStream_t to one session; sessions without one use the process default of shl_mi355x_set_stream
 * (NULL = HIP's default stream).  A device-resident graph session creates and owns its stream. */
void shl_mi355x_set_stream(void *stream);
void *shl_mi355x_get_stream(void);
void shl_mi355x_session_set_stream(struct csinn_session *sess, void *stream);
/* undo it: the session follows the process default (shl_mi355x_set_stream) again; 1 when it has a stream of its own */
void shl_mi355x_session_inherit_stream(struct csinn_session *sess);
int shl_mi355x_session_has_own_stream(struct csinn_session *sess);

/* release the device plan attached to a params block by an init callback (the reference's
 * optimised backends leak theirs: "XXX: memory leak", thead_rvv/int8/convolution.c:177) */
int shl_mi355x_release_params(void *params);
/* number of live plans and their total HBM bytes (leak checks in tests) */
int shl_mi355x_live_plans(int64_t *hbm_bytes);
/* how many times a plan (or a grouped layer's plan set) has been bound to a params block since the library was loaded:
 * lets a caller see that an exec-time planner (the CSINN_OP_*_CHANNEL ids) does NOT plan again on a repeated call */
int64_t shl_mi355x_plans_created(void);
/* device block of the plan attached to `params` (for the RCCL weight broadcast) */
void *shl_mi355x_params_const_block(void *params, size_t *bytes);
/* multi-GPU setup: RCCL broadcast of the layers' constant blocks from rank `root` over the
 * communicator of shl_mi355x_comm_create (include/shl_mi355x.h); CSINN_TRUE once they have landed */
int shl_mi355x_bcast_const_blocks(void *comm, void **params, int32_t n, int32_t root, struct csinn_session *sess);
/* for a caller that moved the constant blocks with a transport of its own: every plan of params[0..n) adopts the
 * epilogue choices recorded in the block it now holds (shl_mi355x_conv_plan_adopt_block) */
int shl_mi355x_params_adopt_blocks(void **params, int32_t n, struct csinn_session *sess);
/* name of the HIP kernel the plan attached to `params` launches ("" if none) */
const char *shl_mi355x_params_kernel_name(void *params);

/* init / exec callbacks (exported so that a reference-side setup.c can list them) */
int shl_mi355x_conv2d_init(CSINN_CONV_ARGS);
int shl_mi355x_conv2d_exec(CSINN_CONV_ARGS);
/* transposed convolution (source/mi355x_opt/deconvolution.c): CSINN_OP_DECONV2D and CSINN_OP_DEPTHWISE_DECONV2D, int8 and
 * fp16, NHWC and NCHW.  Refused at init (the layer then runs on the reference where libshl is loaded, and fails at exec
 * otherwise): CSINN_OP_GROUP_DECONV2D, a non-zero kernel zero point, per-channel kernel records on an NCHW group-1 kernel
 * (their axis is the INPUT channel there), per-channel activations, fp16 scales != 1, dilation != 1 */
int shl_mi355x_deconv2d_init(CSINN_CONV_ARGS);
int shl_mi355x_deconv2d_exec(CSINN_CONV_ARGS);
int shl_mi355x_group_conv2d_exec(CSINN_CONV_ARGS);  /* selected by init when 1 < group < Cin */
/* CSINN_OP_CONV2D_CHANNEL* / CSINN_OP_DEPTHWISE_CONV2D_CHANNEL* (int8 NCHW; source/reference/
 * convolution_channel.c).  The reference registers no init for these ids: exec plans on first use. */
int shl_mi355x_conv2d_channel_init(CSINN_CONV_ARGS);
int shl_mi355x_conv2d_channel_exec(CSINN_CONV_ARGS);
int shl_mi355x_conv2d_channel_relu_init(CSINN_CONV_ARGS);
int shl_mi355x_conv2d_channel_relu_exec(CSINN_CONV_ARGS);
int shl_mi355x_conv2d_channel_relu6_init(CSINN_CONV_ARGS);
int shl_mi355x_conv2d_channel_relu6_exec(CSINN_CONV_ARGS);
int shl_mi355x_group_conv2d_channel_init(CSINN_CONV_ARGS);      /* CSINN_OP_GROUP_CONV2D_CHANNEL{,_RELU}: one image */
int shl_mi355x_group_conv2d_channel_exec(CSINN_CONV_ARGS);
int shl_mi355x_group_conv2d_channel_relu_init(CSINN_CONV_ARGS);
int shl_mi355x_group_conv2d_channel_relu_exec(CSINN_CONV_ARGS);
int shl_mi355x_depthwise_conv2d_channel_init(CSINN_CONV_ARGS);
int shl_mi355x_depthwise_conv2d_channel_exec(CSINN_CONV_ARGS);
int shl_mi355x_depthwise_conv2d_channel_relu_init(CSINN_CONV_ARGS);
int shl_mi355x_depthwise_conv2d_channel_relu_exec(CSINN_CONV_ARGS);
int shl_mi355x_depthwise_conv2d_channel_relu6_init(CSINN_CONV_ARGS);
int shl_mi355x_depthwise_conv2d_channel_relu6_exec(CSINN_CONV_ARGS);
int shl_mi355x_fullyconnected_init(struct csinn_tensor *input, struct csinn_tensor *output,
                                   struct csinn_tensor *weights, struct csinn_tensor *bias,
                                   struct csinn_fc_params *params);
int shl_mi355x_fullyconnected_exec(struct csinn_tensor *input, struct csinn_tensor *output,
                                   struct csinn_tensor *weights, struct csinn_tensor *bias,
                                   struct csinn_fc_params *params);
int shl_mi355x_relu_exec(struct csinn_tensor *input, struct csinn_tensor *output,
                         struct csinn_relu_params *params);
int shl_mi355x_relu6_exec(struct csinn_tensor *input, struct csinn_tensor *output,
                          struct csinn_relu_params *params);
int shl_mi355x_add_exec(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                        struct csinn_diso_params *params);
/* concat along params->axis (-1: the last axis) of params->inputs_count tensors: every non-axis dim must equal the
 * output's and the axis dims must sum to the output's, else the call is refused; the same tensor may appear twice */
int shl_mi355x_concat_exec(struct csinn_tensor **input, struct csinn_tensor *output, struct csinn_concat_params *params);
/* split along params->axis (< 0: from the back) into params->output_num tensors, each with its own record: the outputs'
 * dims must be the ones the reference's rule gives (split_index, or chunks of ceil(dim / output_num) with the last output
 * taking what is left), every chunk longer than 0, else the call is refused (source/mi355x_opt/split.c) */
int shl_mi355x_split_exec(struct csinn_tensor *input, struct csinn_tensor **output, struct csinn_split_params *params);
/* shuffle_channel of a 4-d NHWC / NCHW tensor whose channel count is a multiple of params->group */
int shl_mi355x_shuffle_channel_exec(struct csinn_tensor *input, struct csinn_tensor *output,
                                    struct csinn_shuffle_channel_params *params);
/* transpose of a tensor of up to 8 dims under any permutation: permute_num must equal dim_count, permute be a permutation
 * and the output's dims the permuted input dims, else the call is refused (source/mi355x_opt/move.c) */
int shl_mi355x_transpose_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_transpose_params *params);
/* reshape / flatten: a flat requantised copy into the output tensor's dims; unequal element counts are refused */
int shl_mi355x_reshape_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reshape_params *params);
int shl_mi355x_flatten_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_flatten_params *params);
/* constant pad of a 4-d NCHW / NHWC tensor (pad_num == 4): EDGE / REFLECT, negative pads and output dims other than
 * input + before + after are refused */
int shl_mi355x_pad_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pad_params *params);
/* reductions (source/mi355x_opt/reduce.c): mean / sum / max / min over the params' two group lists (up to 8 groups a list,
 * 4 after canonicalisation), reduce_mean / _sum / _max / _min over ONE axis or the whole tensor (axis[0] == -1), and
 * global_maxpool2d of a 4-d NCHW / NHWC tensor.  A layer the kernels' descriptor cannot express (axis_count != 1, an index
 * past the input, an output tensor of another size) is refused */
int shl_mi355x_mean_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_sum_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_max_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_min_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_reduce_mean_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_reduce_sum_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_reduce_max_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_reduce_min_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int shl_mi355x_global_maxpool2d_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pool_params *params);
/* matmul (source/mi355x_opt/matmul.c): tensors of 2 .. 8 dims, the leading dims of each multiplied into a batch count; equal
 * counts with any transposes, or mat1's count of 1 with none (the reference's "dense" broadcast).  mat1 may be a constant.
 * Any other broadcast, operands that disagree on K and an output tensor of another size are refused */
int shl_mi355x_matmul_exec(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
                           struct csinn_matmul_params *params);
/* resize (source/mi355x_opt/resize.c): 4-d tensors, nearest-neighbour or bilinear, to the output tensor's height and
 * width; batch and channels of input and output must agree; bicubic, and align_corners with an output extent of 1 (the
 * reference divides by zero), are refused */
int shl_mi355x_resize_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_resize_params *params);
/* the reference's scale of one axis: ONE float division, (float)in / out or, with align_corners, (float)(in - 1) / (out - 1) */
float shl_mi355x_resize_scale(int32_t in, int32_t out, int align_corners);
/* the 256 results of the int8 nearest-neighbour gather for the two records: table[(uint8_t)q] =
 * float_to_int8(int8_to_float(q, in record), out record).  Pure host code */
void shl_mi355x_resize_table_i8(float in_scale, int32_t in_zp, float out_scale, int32_t out_zp, uint8_t table[256]);
/* sigmoid / hard_sigmoid / silu / leaky_relu (source/mi355x_opt/eltwise.c): int8 through a 256-entry table built on the
 * host, binary16 through the formula kernel; input and output hold the same number of elements */
int shl_mi355x_sigmoid_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params);
int shl_mi355x_hard_sigmoid_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params);
int shl_mi355x_silu_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params);
int shl_mi355x_leaky_relu_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_relu_params *params);
/* the 256 results of the int8 operator for the two records, as the reference computes them: table[(uint8_t)q] =
 * float_to_int8(f(int8_to_float(q, in record)), out record).  Pure host code.  `n`: leaky_relu's slope */
void shl_mi355x_sigmoid_table_i8(float in_scale, int32_t in_zp, float out_scale, int32_t out_zp, uint8_t table[256]);
void shl_mi355x_hard_sigmoid_table_i8(float in_scale, int32_t in_zp, float out_scale, int32_t out_zp, uint8_t table[256]);
void shl_mi355x_silu_table_i8(float in_scale, int32_t in_zp, float out_scale, int32_t out_zp, uint8_t table[256]);
void shl_mi355x_leaky_relu_table_i8(float in_scale, int32_t in_zp, float out_scale, int32_t out_zp, float n, uint8_t table[256]);
/* the gate of a swish / hard-swish, act(x) -> mul(x, gate), as ONE table: table[(uint8_t)b] = the byte the reference's mul gives
 * for the operands (b, act(b)).  `kind`: SHL_MI355X_UNARY_SIGMOID or SHL_MI355X_UNARY_HARD_SIGMOID; x: the record of the tensor
 * both layers read; gate: the activation's output record; `x_is_first`: x is the mul's first operand; out: the mul's output
 * record.  Pure host code */
void shl_mi355x_gate_mul_table_i8(int kind, float x_scale, int32_t x_zp, float gate_scale, int32_t gate_zp, int x_is_first,
                                  float out_scale, int32_t out_zp, uint8_t table[256]);
/* elementwise product; one operand has the output's shape, the other is broadcast to it by the reference's rule (either
 * order).  Both operands needing a broadcast, or shapes that break the rule, are refused */
int shl_mi355x_mul_exec(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                        struct csinn_diso_params *params);
int shl_mi355x_global_avgpool2d_exec(struct csinn_tensor *input, struct csinn_tensor *output,
                                     struct csinn_pool_params *params);
/* windowed pooling: 4-d tensors, the output size is the output tensor's; a window without an in-image tap is refused */
int shl_mi355x_maxpool2d_exec(struct csinn_tensor *input, struct csinn_tensor *output,
                              struct csinn_pool_params *params);
int shl_mi355x_avgpool2d_exec(struct csinn_tensor *input, struct csinn_tensor *output,
                              struct csinn_pool_params *params);
int shl_mi355x_softmax_exec(struct csinn_tensor *input, struct csinn_tensor *output,
                            struct csinn_softmax_params *params);

/* device-resident graph execution (source/mi355x_opt/session.c): SESSION_SETUP / SESSION_RUN /
 * SESSION_DEINIT handlers returned by shl_mi355x_runtime_callback.  A session whose layers all run
 * on the GPU keeps every tensor in HBM and replays one hipGraph per csinn_session_run. */
int shl_mi355x_session_setup(struct csinn_session *sess);
int shl_mi355x_session_run(struct csinn_session *sess);
void shl_mi355x_session_deinit(struct csinn_session *sess);
/* 0: host-staged (executor's own run), 1: device-resident eager, 2: device-resident hipGraph */
int shl_mi355x_session_is_device_resident(struct csinn_session *sess);
/* the stream `sess` enqueues on.  When every graph output of a device-resident session is a DMABUF tensor
 * csinn_session_run only enqueues (no synchronisation); wait with shl_mi355x_stream_sync on this stream */
void *shl_mi355x_session_stream(struct csinn_session *sess);
/* depthwise + pointwise pairs of `sess` that run as one fused launch (graph-level fusion) */
int shl_mi355x_session_fused_pairs(struct csinn_session *sess);
/* global_avgpool2d layers that run inside the launch of the convolution / fullyconnected layer consuming them */
int shl_mi355x_session_fused_pools(struct csinn_session *sess);
/* relu / relu6 layers of `sess` that were folded into the epilogue of the convolution they follow */
int shl_mi355x_session_folded_activations(struct csinn_session *sess);
/* matmul layers of `sess` that run the add of a constant bias behind them inside their own launch (shl_mi355x_matmul_bias) */
int shl_mi355x_session_fused_linears(struct csinn_session *sess);
/* chains matmul(q, k, trans_b) -> [mul by a one-element constant] -> softmax over the last axis -> matmul(p, v) of `sess` that
 * run as one launch (shl_mi355x_attention).  By default those of a shape class the fused launch was measured faster on
 * (shl_mi355x_attention_by_default); at setup SHL_MI355X_ATTENTION=1 merges every chain the kernel takes, SHL_MI355X_ATTENTION=0
 * or SHL_MI355X_NO_FUSION=1 keeps the layers apart */
int shl_mi355x_session_fused_attentions(struct csinn_session *sess);
/* ... those of them that carry an add of a bias or mask between the [scaled] scores and the softmax, on either side, its other
 * operand a constant or an earlier activation broadcast to the scores (shl_mi355x_attention_bias; counted in the number above
 * as well).  Their default is shl_mi355x_attention_bias_by_default; the switches are the same.  Operands of equal shape, a
 * bias that needs more than two groups of the batch dims, and a mul behind the add stay apart */
int shl_mi355x_session_fused_attention_biases(struct csinn_session *sess);
/* The reshape / transpose layers around those cores -- a model's head split in front of q, k and v (reshape [B,S,H,D],
 * transpose(0,2,1,3); K also as transpose(0,2,3,1) into a product without trans_b) and the merge behind the output -- that run
 * inside the core's launch, which reads the sources' buffers and writes the last folded layer's output through strides
 * (shl_mi355x_attention_layout).  A run folds when every layer in it is this backend's, is read by one consumer and is no graph
 * output (the last one behind the core may be read by any), copies its elements unchanged (int8: equal records whose
 * requantisation is the identity; binary16: scale 1, with the movers' rule for infinities and NaNs applied by the launch), and the
 * strides express the view; each of the four sides folds or stays on its own.  At setup SHL_MI355X_ATTENTION_LAYOUT=0 folds
 * nothing, =1 every run the kernel takes around every chain that SHL_MI355X_ATTENTION lets merge; unset, the classes one layout
 * launch was measured faster on (shl_mi355x_attention_layout_by_default) -- a core the dense default leaves apart then merges
 * too when all four sides fold.  SHL_MI355X_ATTENTION=0 keeps everything apart */
int shl_mi355x_session_folded_head_moves(struct csinn_session *sess);
/* tails of skip connections of `sess` -- convolution -> add(conv_out, skip) -> [relu | relu6] -- that run as one launch of the
 * convolution (shl_mi355x_conv_add_forward; int8 NHWC implicit-GEMM plans, same-shape adds).  By default those of a shape class
 * the fused launch was measured faster on (shl_mi355x_conv_add_by_default); at setup SHL_MI355X_RESIDUAL=1 merges every tail the
 * kernel takes, SHL_MI355X_RESIDUAL=0 or SHL_MI355X_NO_FUSION=1 keeps the layers apart */
int shl_mi355x_session_fused_residuals(struct csinn_session *sess);
/* table activations of `sess` that run inside their convolution's launch (shl_mi355x_conv_lut_forward: int8 NHWC
 * implicit-GEMM plans; shl_mi355x_dwconv_lut_forward: int8 NHWC depthwise plans): convolution -> sigmoid | hard_sigmoid | silu | leaky_relu, and the gates convolution -> sigmoid |
 * hard_sigmoid -> mul(conv_out, gate), each counted once.  By default those of a shape class the fused launch was measured
 * faster on (shl_mi355x_conv_lut_by_default, shl_mi355x_dwconv_lut_by_default); at setup SHL_MI355X_ACT_FUSE=1 merges every one the kernel takes,
 * SHL_MI355X_ACT_FUSE=0 or SHL_MI355X_NO_FUSION=1 keeps the layers apart */
int shl_mi355x_session_fused_activations(struct csinn_session *sess);
/* the plan of `sess` as text, for tests and for reading: one line per step in launch order -- the rule's name ("layer": a plain
 * layer), the layers it stands for, " -> " and the name of the tensor it writes, for an attention step also the layers folded in
 * front of q, k, v and behind the output and whether it carries a bias -- then "folded <n>", the count of folded activations.
 * Writes at most len bytes, the terminator included; returns the length needed, 0 for a host-staged session */
int shl_mi355x_session_describe(struct csinn_session *sess, char *buf, int len);

#ifdef __cplusplus
}
#endif
#endif /* SHL_MI355X_BACKEND_H_ */

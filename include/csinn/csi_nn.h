/*
 * csi_nn.h -- operator entry points of the hot path.
 *
 * Restated from the reference's include/csinn/csi_nn.h (conv2d :55/:75,
 * depthwise_conv2d :91/:107, conv2d_relu :155/:171, depthwise_conv2d_relu
 * :187/:203, conv2d_relu6 :219/:235, fullyconnected :393/:409, relu, relu6,
 * global_avgpool2d, softmax).  Every op is a pair:
 *   csinn_<op>_init(...)  choose the backend callbacks for (api, op, dtype);
 *                         in layer mode also run the backend's `init`
 *   csinn_<op>(...)       layer mode: run `exec`; graph mode: run `est`
 * Both return CSINN_TRUE (1) on success or a negative csinn_status_enum.
 */
#ifndef CSINN_MI355X_CSI_NN_H_
#define CSINN_MI355X_CSI_NN_H_

#include "csinn_data_structure.h"
#include "csinn_runtime.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSINN_CONV_ARGS                                                        \
    struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_tensor *kernel, \
        struct csinn_tensor *bias, struct csinn_conv2d_params *params

int csinn_conv2d_init(CSINN_CONV_ARGS);
int csinn_conv2d(CSINN_CONV_ARGS);
int csinn_conv2d_relu_init(CSINN_CONV_ARGS);
int csinn_conv2d_relu(CSINN_CONV_ARGS);
int csinn_conv2d_relu6_init(CSINN_CONV_ARGS);
int csinn_conv2d_relu6(CSINN_CONV_ARGS);
int csinn_depthwise_conv2d_init(CSINN_CONV_ARGS);
int csinn_depthwise_conv2d(CSINN_CONV_ARGS);
int csinn_depthwise_conv2d_relu_init(CSINN_CONV_ARGS);
int csinn_depthwise_conv2d_relu(CSINN_CONV_ARGS);

int csinn_fullyconnected_init(struct csinn_tensor *input, struct csinn_tensor *output,
                              struct csinn_tensor *weights, struct csinn_tensor *bias,
                              struct csinn_fc_params *params);
int csinn_fullyconnected(struct csinn_tensor *input, struct csinn_tensor *output,
                         struct csinn_tensor *weights, struct csinn_tensor *bias,
                         struct csinn_fc_params *params);

/* ops between MobileNet convolutions */
int csinn_relu_init(struct csinn_tensor *input, struct csinn_tensor *output,
                    struct csinn_relu_params *params);
int csinn_relu(struct csinn_tensor *input, struct csinn_tensor *output,
               struct csinn_relu_params *params);
int csinn_relu6_init(struct csinn_tensor *input, struct csinn_tensor *output,
                     struct csinn_relu_params *params);
int csinn_relu6(struct csinn_tensor *input, struct csinn_tensor *output,
                struct csinn_relu_params *params);
/* residual add of two same-shape tensors (source/nn2/add.c) */
int csinn_add_init(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                   struct csinn_diso_params *params);
int csinn_add(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
              struct csinn_diso_params *params);
/* sigmoid family and leaky_relu (source/nn2/sigmoid.c, hard_sigmoid.c, silu.c, leaky_relu.c of the reference);
 * leaky_relu's slope is params->n */
int csinn_sigmoid_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params);
int csinn_sigmoid(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params);
int csinn_hard_sigmoid_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params);
int csinn_hard_sigmoid(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params);
int csinn_silu_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params);
int csinn_silu(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params);
int csinn_leaky_relu_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_relu_params *params);
int csinn_leaky_relu(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_relu_params *params);
/* elementwise product with broadcasting of either operand (source/nn2/mul.c) */
int csinn_mul_init(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                   struct csinn_diso_params *params);
int csinn_mul(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
              struct csinn_diso_params *params);
/* transposed convolution (source/nn2/deconvolution.c of the reference): group == 1 is CSINN_OP_DECONV2D, group == Cin
 * CSINN_OP_DEPTHWISE_DECONV2D, group == Cout CSINN_OP_GROUP_DECONV2D, anything else CSINN_FALSE; kernel [O,Kh,Kw,I] (NHWC) /
 * [I,O,Kh,Kw] (NCHW), depthwise [1,Kh,Kw,C] / [C,1,Kh,Kw]; the output size is the output tensor's.  As in the reference the
 * init callback's status is not returned: a layer the backend refused fails at csinn_deconv2d */
int csinn_deconv2d_init(CSINN_CONV_ARGS);
int csinn_deconv2d(CSINN_CONV_ARGS);
/* nearest-neighbour / bilinear resize to the output tensor's height and width (source/nn2/resize.c of the reference) */
int csinn_resize_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_resize_params *params);
int csinn_resize(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_resize_params *params);
/* concat along one axis (source/nn2/concat.c of the reference): `input` is an array of params->inputs_count tensors; the
 * callbacks are looked up by the OUTPUT's dtype */
int csinn_concat_init(struct csinn_tensor **input, struct csinn_tensor *output, struct csinn_concat_params *params);
int csinn_concat(struct csinn_tensor **input, struct csinn_tensor *output, struct csinn_concat_params *params);
/* split along one axis (source/nn2/split.c of the reference): `output` is an array of params->output_num tensors */
int csinn_split_init(struct csinn_tensor *input, struct csinn_tensor **output, struct csinn_split_params *params);
int csinn_split(struct csinn_tensor *input, struct csinn_tensor **output, struct csinn_split_params *params);
/* shuffle_channel (source/nn2/shuffle_channel.c of the reference): one input, one output */
int csinn_shuffle_channel_init(struct csinn_tensor *input, struct csinn_tensor *output,
                               struct csinn_shuffle_channel_params *params);
int csinn_shuffle_channel(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_shuffle_channel_params *params);
/* transpose, reshape, flatten, pad (source/nn2/transpose.c, reshape.c, flatten.c, pad.c of the reference): one input, one
 * output */
int csinn_transpose_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_transpose_params *params);
int csinn_transpose(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_transpose_params *params);
int csinn_reshape_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reshape_params *params);
int csinn_reshape(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reshape_params *params);
int csinn_flatten_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_flatten_params *params);
int csinn_flatten(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_flatten_params *params);
int csinn_pad_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pad_params *params);
int csinn_pad(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pad_params *params);
/* batched matrix product (source/nn2/matmul.c of the reference): two inputs, either of which may be a constant */
int csinn_matmul_init(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
                      struct csinn_matmul_params *params);
int csinn_matmul(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
                 struct csinn_matmul_params *params);
/* reductions (source/nn2/mean.c, sum.c, max.c, min.c, reduce_*.c, global_maxpool2d.c of the reference): one input, one output */
int csinn_mean_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_mean(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_sum_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_sum(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_max_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_max(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_min_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_min(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_reduce_mean_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_reduce_mean(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_reduce_sum_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_reduce_sum(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_reduce_max_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_reduce_max(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_reduce_min_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_reduce_min(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params);
int csinn_global_maxpool2d_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pool_params *params);
int csinn_global_maxpool2d(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pool_params *params);
/* MobileNet tail (source/nn2/global_avgpool2d.c, softmax.c of the reference) */
int csinn_global_avgpool2d_init(struct csinn_tensor *input, struct csinn_tensor *output,
                                struct csinn_pool_params *params);
int csinn_global_avgpool2d(struct csinn_tensor *input, struct csinn_tensor *output,
                           struct csinn_pool_params *params);
/* windowed pooling (source/nn2/maxpool.c, averagepool.c of the reference): the output tensor's dims set the output size */
int csinn_maxpool2d_init(struct csinn_tensor *input, struct csinn_tensor *output,
                         struct csinn_pool_params *params);
int csinn_maxpool2d(struct csinn_tensor *input, struct csinn_tensor *output,
                    struct csinn_pool_params *params);
int csinn_avgpool2d_init(struct csinn_tensor *input, struct csinn_tensor *output,
                         struct csinn_pool_params *params);
int csinn_avgpool2d(struct csinn_tensor *input, struct csinn_tensor *output,
                    struct csinn_pool_params *params);
int csinn_softmax_init(struct csinn_tensor *input, struct csinn_tensor *output,
                       struct csinn_softmax_params *params);
int csinn_softmax(struct csinn_tensor *input, struct csinn_tensor *output,
                  struct csinn_softmax_params *params);

#ifdef __cplusplus
}
#endif
#endif /* CSINN_MI355X_CSI_NN_H_ */

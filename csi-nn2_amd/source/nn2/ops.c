/*
 * ops.c -- csinn_<op>_init / csinn_<op> pairs for the operators on the MI355X hot path.
 *
 * Behaviour follows the reference front-end:
 *   conv2d ............ source/nn2/convolution.c:26-84   (classifies conv / depthwise / group)
 *   conv2d_relu(6) .... source/nn2/convolution_relu.c, convolution_relu6.c
 *   depthwise_conv2d .. source/nn2/depthwise_conv2d.c:26-57, depthwise_conv2d_relu.c
 *   fullyconnected .... source/nn2/fullyconnected.c:26-57
 *   relu / relu6 ...... source/nn2/relu.c, relu6.c
 *   maxpool2d / avgpool2d  source/nn2/maxpool.c, averagepool.c
 *   concat ............ source/nn2/concat.c
 *   resize ............ source/nn2/resize.c
 *   split / shuffle_channel  source/nn2/split.c, shuffle_channel.c
 *   transpose / reshape / flatten / pad  source/nn2/transpose.c, reshape.c, flatten.c, pad.c
 *   mean / sum / max / min / reduce_* / global_maxpool2d  source/nn2/mean.c, sum.c, max.c, min.c, reduce_*.c, global_maxpool2d.c
 *   matmul ............ source/nn2/matmul.c
 *   deconv2d .......... source/nn2/deconvolution.c
 *   sigmoid / hard_sigmoid / silu / leaky_relu / mul  source/nn2/sigmoid.c, hard_sigmoid.c, silu.c, leaky_relu.c, mul.c
 * The only deliberate difference: a missing callback is reported (CSINN_CALLBACK_UNSET and an
 * error message) instead of being dereferenced.
 */
#include "shl_utils.h"

/* group == 1 -> plain conv; group == Cin with a single-input-channel kernel -> depthwise;
 * anything else -> grouped.  `plain` is the op id of the group==1 flavour; depthwise and
 * grouped ids sit at fixed distances from it in enum csinn_op_enum. */
static int classify(struct csinn_tensor *input, struct csinn_tensor *kernel,
                    struct csinn_conv2d_params *params, int plain, int depthwise, int grouped)
{
    int cin, k_in;
    if (params->base.layout == CSINN_LAYOUT_NCHW) {
        cin = input->dim[1];
        k_in = kernel->dim[1];
    } else if (params->base.layout == CSINN_LAYOUT_NHWC) {
        cin = input->dim[3];
        k_in = kernel->dim[0];
    } else {
        return CSINN_UNSUPPORT_LAYOUT;
    }
    if (params->group == 1) return plain;
    if (params->group == cin && k_in == 1) return depthwise;
    return grouped;
}

/* The arity of a callback is a property of the operator, never of the data: a convolution without a
 * bias tensor still passes all five arguments (bias == NULL), as the reference front-end does
 * (source/nn2/convolution.c:45-52). */
static int map_and_init5(struct csinn_params_base *base, int op, int dtype, void *a, void *b,
                         void *c, void *d, void *params)
{
    int rc = shl_op_callback_map(base, op, dtype);
    if (rc != CSINN_TRUE) return rc;
    int (*init)() = shl_get_init_cb(base);
    if (init != NULL) {
        rc = init(a, b, c, d, params);
        if (rc != CSINN_TRUE) return rc;
    }
    return CSINN_TRUE;
}

static int map_and_init3(struct csinn_params_base *base, int op, int dtype, void *a, void *b,
                         void *params)
{
    int rc = shl_op_callback_map(base, op, dtype);
    if (rc != CSINN_TRUE) return rc;
    int (*init)() = shl_get_init_cb(base);
    if (init != NULL) {
        rc = init(a, b, params);
        if (rc != CSINN_TRUE) return rc;
    }
    return CSINN_TRUE;
}

static int run5(struct csinn_params_base *base, void *a, void *b, void *c, void *d, void *params)
{
    int (*fn)() = shl_get_p0_cb(base);
    if (fn == NULL) return CSINN_CALLBACK_UNSET;
    int rc = fn(a, b, c, d, params);
    return rc == CSINN_TRUE ? CSINN_TRUE : rc;
}

static int run3(struct csinn_params_base *base, void *a, void *b, void *params)
{
    int (*fn)() = shl_get_p0_cb(base);
    if (fn == NULL) return CSINN_CALLBACK_UNSET;
    int rc = fn(a, b, params);
    return rc == CSINN_TRUE ? CSINN_TRUE : rc;
}

#define CONV_FAMILY(fn_name, PLAIN, DW, GROUP)                                               \
    int fn_name##_init(CSINN_CONV_ARGS)                                                      \
    {                                                                                        \
        int op = classify(input, kernel, params, PLAIN, DW, GROUP);                          \
        if (op < 0) return op;                                                               \
        return map_and_init5(&params->base, op, input->dtype, input, output, kernel, bias,   \
                             params);                                                         \
    }                                                                                        \
    int fn_name(CSINN_CONV_ARGS) { return run5(&params->base, input, output, kernel, bias, params); }

CONV_FAMILY(csinn_conv2d, CSINN_OP_CONV2D, CSINN_OP_DEPTHWISE_CONV2D, CSINN_OP_GROUP_CONV2D)
CONV_FAMILY(csinn_conv2d_relu, CSINN_OP_CONV2D_RELU, CSINN_OP_DEPTHWISE_CONV2D_RELU,
            CSINN_OP_GROUP_CONV2D_RELU)
CONV_FAMILY(csinn_conv2d_relu6, CSINN_OP_CONV2D_RELU6, CSINN_OP_DEPTHWISE_CONV2D_RELU6,
            CSINN_OP_GROUP_CONV2D_RELU6)

int csinn_depthwise_conv2d_init(CSINN_CONV_ARGS)
{
    return map_and_init5(&params->base, CSINN_OP_DEPTHWISE_CONV2D, input->dtype, input, output,
                         kernel, bias, params);
}
int csinn_depthwise_conv2d(CSINN_CONV_ARGS)
{
    return run5(&params->base, input, output, kernel, bias, params);
}

int csinn_depthwise_conv2d_relu_init(CSINN_CONV_ARGS)
{
    return map_and_init5(&params->base, CSINN_OP_DEPTHWISE_CONV2D_RELU, input->dtype, input,
                         output, kernel, bias, params);
}
int csinn_depthwise_conv2d_relu(CSINN_CONV_ARGS)
{
    return run5(&params->base, input, output, kernel, bias, params);
}

int csinn_fullyconnected_init(struct csinn_tensor *input, struct csinn_tensor *output,
                              struct csinn_tensor *weights, struct csinn_tensor *bias,
                              struct csinn_fc_params *params)
{
    return map_and_init5(&params->base, CSINN_OP_FULLYCONNECTED, input->dtype, input, output,
                         weights, bias, params);
}
int csinn_fullyconnected(struct csinn_tensor *input, struct csinn_tensor *output,
                         struct csinn_tensor *weights, struct csinn_tensor *bias,
                         struct csinn_fc_params *params)
{
    return run5(&params->base, input, output, weights, bias, params);
}

int csinn_relu_init(struct csinn_tensor *input, struct csinn_tensor *output,
                    struct csinn_relu_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_RELU, input->dtype, input, output, params);
}
int csinn_relu(struct csinn_tensor *input, struct csinn_tensor *output,
               struct csinn_relu_params *params)
{
    return run3(&params->base, input, output, params);
}

int csinn_relu6_init(struct csinn_tensor *input, struct csinn_tensor *output,
                     struct csinn_relu_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_RELU6, input->dtype, input, output, params);
}
int csinn_relu6(struct csinn_tensor *input, struct csinn_tensor *output,
                struct csinn_relu_params *params)
{
    return run3(&params->base, input, output, params);
}

int csinn_global_avgpool2d_init(struct csinn_tensor *input, struct csinn_tensor *output,
                                struct csinn_pool_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_GLOBAL_AVGPOOL2D, input->dtype, input, output, params);
}
int csinn_global_avgpool2d(struct csinn_tensor *input, struct csinn_tensor *output,
                           struct csinn_pool_params *params)
{
    return run3(&params->base, input, output, params);
}

/* source/nn2/maxpool.c, averagepool.c of the reference: same dispatch as the global pool */
int csinn_maxpool2d_init(struct csinn_tensor *input, struct csinn_tensor *output,
                         struct csinn_pool_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_MAXPOOL2D, input->dtype, input, output, params);
}
int csinn_maxpool2d(struct csinn_tensor *input, struct csinn_tensor *output,
                    struct csinn_pool_params *params)
{
    return run3(&params->base, input, output, params);
}

int csinn_avgpool2d_init(struct csinn_tensor *input, struct csinn_tensor *output,
                         struct csinn_pool_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_AVGPOOL2D, input->dtype, input, output, params);
}
int csinn_avgpool2d(struct csinn_tensor *input, struct csinn_tensor *output,
                    struct csinn_pool_params *params)
{
    return run3(&params->base, input, output, params);
}

int csinn_softmax_init(struct csinn_tensor *input, struct csinn_tensor *output,
                       struct csinn_softmax_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_SOFTMAX, input->dtype, input, output, params);
}
int csinn_softmax(struct csinn_tensor *input, struct csinn_tensor *output,
                  struct csinn_softmax_params *params)
{
    return run3(&params->base, input, output, params);
}

/* source/nn2/sigmoid.c, hard_sigmoid.c, silu.c, leaky_relu.c of the reference: one input, one output */
int csinn_sigmoid_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_SIGMOID, input->dtype, input, output, params);
}
int csinn_sigmoid(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params)
{
    return run3(&params->base, input, output, params);
}

int csinn_hard_sigmoid_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_HARD_SIGMOID, input->dtype, input, output, params);
}
int csinn_hard_sigmoid(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params)
{
    return run3(&params->base, input, output, params);
}

int csinn_silu_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_SILU, input->dtype, input, output, params);
}
int csinn_silu(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params)
{
    return run3(&params->base, input, output, params);
}

int csinn_leaky_relu_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_relu_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_LEAKY_RELU, input->dtype, input, output, params);
}
int csinn_leaky_relu(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_relu_params *params)
{
    return run3(&params->base, input, output, params);
}

/* source/nn2/add.c:26-55, mul.c: two inputs, one output; the callbacks are looked up by the FIRST input's dtype */
static int map_and_init4(struct csinn_params_base *base, int op, struct csinn_tensor *input0, struct csinn_tensor *input1,
                         struct csinn_tensor *output, void *params)
{
    int rc = shl_op_callback_map(base, op, input0->dtype);
    if (rc != CSINN_TRUE) return rc;
    int (*init)() = shl_get_init_cb(base);
    if (init != NULL) {
        rc = init(input0, input1, output, params);
        if (rc != CSINN_TRUE) return rc;
    }
    return CSINN_TRUE;
}

static int run4(struct csinn_params_base *base, void *a, void *b, void *c, void *params)
{
    int (*fn)() = shl_get_p0_cb(base);
    if (fn == NULL) return CSINN_CALLBACK_UNSET;
    int rc = fn(a, b, c, params);
    return rc == CSINN_TRUE ? CSINN_TRUE : rc;
}

int csinn_add_init(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                   struct csinn_diso_params *params)
{
    return map_and_init4(&params->base, CSINN_OP_ADD, input0, input1, output, params);
}
int csinn_add(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
              struct csinn_diso_params *params)
{
    return run4(&params->base, input0, input1, output, params);
}

int csinn_mul_init(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                   struct csinn_diso_params *params)
{
    return map_and_init4(&params->base, CSINN_OP_MUL, input0, input1, output, params);
}
int csinn_mul(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
              struct csinn_diso_params *params)
{
    return run4(&params->base, input0, input1, output, params);
}

/* source/nn2/matmul.c of the reference: two inputs, one output, the dtype of the first input picks the callback */
int csinn_matmul_init(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
                      struct csinn_matmul_params *params)
{
    return map_and_init4(&params->base, CSINN_OP_MATMUL, mat0, mat1, output, params);
}
int csinn_matmul(struct csinn_tensor *mat0, struct csinn_tensor *mat1, struct csinn_tensor *output,
                 struct csinn_matmul_params *params)
{
    return run4(&params->base, mat0, mat1, output, params);
}

/* source/nn2/deconvolution.c:26-46 of the reference: the op id by the group count alone, and the init callback's status
 * is dropped -- a layer whose init refused it is left with a callback that fails at csinn_deconv2d */
int csinn_deconv2d_init(CSINN_CONV_ARGS)
{
    const int nchw = params->base.layout == CSINN_LAYOUT_NCHW, nhwc = params->base.layout == CSINN_LAYOUT_NHWC;
    int op;
    if (params->group == 1) op = CSINN_OP_DECONV2D;
    else if ((nchw && params->group == input->dim[1]) || (nhwc && params->group == input->dim[3])) op = CSINN_OP_DEPTHWISE_DECONV2D;
    else if ((nchw && params->group == output->dim[1]) || (nhwc && params->group == output->dim[3])) op = CSINN_OP_GROUP_DECONV2D;
    else return CSINN_FALSE;
    if (shl_op_callback_map(&params->base, op, input->dtype) != CSINN_TRUE) return CSINN_TRUE; /* (csinn_deconv2d reports it) */
    int (*init)() = shl_get_init_cb(&params->base);
    if (init != NULL) init(input, output, kernel, bias, params);
    return CSINN_TRUE;
}
int csinn_deconv2d(CSINN_CONV_ARGS) { return run5(&params->base, input, output, kernel, bias, params); }

/* source/nn2/resize.c of the reference: one input, one output */
int csinn_resize_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_resize_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_RESIZE, input->dtype, input, output, params);
}
int csinn_resize(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_resize_params *params)
{
    return run3(&params->base, input, output, params);
}

/* source/nn2/concat.c: an array of params->inputs_count inputs; the callbacks are looked up by the OUTPUT's dtype */
int csinn_concat_init(struct csinn_tensor **input, struct csinn_tensor *output, struct csinn_concat_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_CONCAT, output->dtype, input, output, params);
}
int csinn_concat(struct csinn_tensor **input, struct csinn_tensor *output, struct csinn_concat_params *params)
{
    return run3(&params->base, input, output, params);
}

/* source/nn2/split.c: one input, an array of params->output_num outputs; the callbacks are looked up by the input's dtype */
int csinn_split_init(struct csinn_tensor *input, struct csinn_tensor **output, struct csinn_split_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_SPLIT, input->dtype, input, output, params);
}
int csinn_split(struct csinn_tensor *input, struct csinn_tensor **output, struct csinn_split_params *params)
{
    return run3(&params->base, input, output, params);
}

/* source/nn2/shuffle_channel.c: one input, one output */
int csinn_shuffle_channel_init(struct csinn_tensor *input, struct csinn_tensor *output,
                               struct csinn_shuffle_channel_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_SHUFFLE_CHANNEL, input->dtype, input, output, params);
}
int csinn_shuffle_channel(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_shuffle_channel_params *params)
{
    return run3(&params->base, input, output, params);
}

/* source/nn2/transpose.c, reshape.c, flatten.c, pad.c: one input, one output */
int csinn_transpose_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_transpose_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_TRANSPOSE, input->dtype, input, output, params);
}
int csinn_transpose(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_transpose_params *params)
{
    return run3(&params->base, input, output, params);
}
int csinn_reshape_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reshape_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_RESHAPE, input->dtype, input, output, params);
}
int csinn_reshape(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reshape_params *params)
{
    return run3(&params->base, input, output, params);
}
int csinn_flatten_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_flatten_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_FLATTEN, input->dtype, input, output, params);
}
int csinn_flatten(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_flatten_params *params)
{
    return run3(&params->base, input, output, params);
}
int csinn_pad_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pad_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_PAD, input->dtype, input, output, params);
}
int csinn_pad(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pad_params *params)
{
    return run3(&params->base, input, output, params);
}

/* source/nn2/mean.c, sum.c, max.c, min.c, reduce_mean.c, reduce_sum.c, reduce_max.c, reduce_min.c, global_maxpool2d.c: one
 * input, one output */
int csinn_mean_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_MEAN, input->dtype, input, output, params);
}
int csinn_mean(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return run3(&params->base, input, output, params);
}
int csinn_sum_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_SUM, input->dtype, input, output, params);
}
int csinn_sum(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return run3(&params->base, input, output, params);
}
int csinn_max_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_MAX, input->dtype, input, output, params);
}
int csinn_max(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return run3(&params->base, input, output, params);
}
int csinn_min_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_MIN, input->dtype, input, output, params);
}
int csinn_min(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return run3(&params->base, input, output, params);
}
int csinn_reduce_mean_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_REDUCE_MEAN, input->dtype, input, output, params);
}
int csinn_reduce_mean(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return run3(&params->base, input, output, params);
}
int csinn_reduce_sum_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_REDUCE_SUM, input->dtype, input, output, params);
}
int csinn_reduce_sum(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return run3(&params->base, input, output, params);
}
int csinn_reduce_max_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_REDUCE_MAX, input->dtype, input, output, params);
}
int csinn_reduce_max(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return run3(&params->base, input, output, params);
}
int csinn_reduce_min_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_REDUCE_MIN, input->dtype, input, output, params);
}
int csinn_reduce_min(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_reduce_params *params)
{
    return run3(&params->base, input, output, params);
}
int csinn_global_maxpool2d_init(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pool_params *params)
{
    return map_and_init3(&params->base, CSINN_OP_GLOBAL_MAXPOOL2D, input->dtype, input, output, params);
}
int csinn_global_maxpool2d(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_pool_params *params)
{
    return run3(&params->base, input, output, params);
}

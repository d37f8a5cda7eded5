/*
 * eltwise.c -- sigmoid / hard_sigmoid / silu / leaky_relu and the broadcasting mul of the MI355X backend: what a
 * squeeze-and-excite block, swish / hard-swish and a per-channel scale need between the convolutions.
 *
 * exec(input, output, params) / exec(input0, input1, output, params) with the reference's signatures
 * (source/reference/sigmoid.c:38-42, hard_sigmoid.c:42-46, silu.c:38-42, leaky_relu.c:38-42, mul.c:36-40).
 *
 * int8 unary: the reference dequantises, applies a pure per-element function and requantises
 * (shl_ref_siso_callback_base, source/reference/utils.c:609-621), so with one record per tensor the output byte is a
 * function of the input byte: the table builders below walk the 256 bytes through the reference's own formula in the
 * reference's own precision on the host, and the device only looks up (csrc/eltwise.hip).  Exact by construction.
 */
#include <math.h>
#include <string.h>

#include "mi355x_internal.h"

/* ---- the reference's per-element functions, each in the precision its source uses ------------------------------ */
static float f_sigmoid(float val, float n)
{
    (void)n;
    return 1.0f / (1.0f + exp(-val)); /* sigmoid.c:33: double exp, double sum and quotient, rounded on the store */
}

static float f_silu(float val, float n)
{
    (void)n;
    return val / (1.0f + exp(-val)); /* silu.c:33 */
}

static float f_hard_sigmoid(float val, float n)
{
    (void)n;
    if (val < -2.5) return 0; /* hard_sigmoid.c:31-37: double comparisons, double 0.2 x + 0.5 */
    if (val > 2.5) return 1;
    /* the reference's build (-O3 -mfma) contracts the sum into one fused multiply-add; this file is built without
     * contraction, so it is spelled out (binary16 shows the difference at x = -2.5: -0, not +0) */
    return fma(0.2, val, 0.5);
}

static float f_leaky_relu(float val, float n) { return val > 0 ? val : val * n; /* leaky_relu.c:33 */ }

/* table[(uint8_t)q] = float_to_int8_base(f(int8_to_float_base(q))) (source/nn2/utils.c:499-502, 550-560) */
static void build_table(float (*f)(float, float), float n, float in_scale, int32_t in_zp, float out_scale, int32_t out_zp,
                        uint8_t table[256])
{
    for (int q = -128; q < 128; q++) {
        const float x = ((float)q - in_zp) * in_scale;
        const float y = f(x, n);
        const float ret = nearbyint(y / out_scale) + out_zp;
        int8_t r;
        if (ret > 127) r = 127;
        else if (ret < -128) r = -128;
        else r = (int8_t)ret; /* (a NaN reaches here: records of real models never make one) */
        table[(uint8_t)q] = (uint8_t)r;
    }
}

void shl_mi355x_sigmoid_table_i8(float in_scale, int32_t in_zp, float out_scale, int32_t out_zp, uint8_t table[256])
{
    build_table(f_sigmoid, 0.0f, in_scale, in_zp, out_scale, out_zp, table);
}

void shl_mi355x_hard_sigmoid_table_i8(float in_scale, int32_t in_zp, float out_scale, int32_t out_zp, uint8_t table[256])
{
    build_table(f_hard_sigmoid, 0.0f, in_scale, in_zp, out_scale, out_zp, table);
}

void shl_mi355x_silu_table_i8(float in_scale, int32_t in_zp, float out_scale, int32_t out_zp, uint8_t table[256])
{
    build_table(f_silu, 0.0f, in_scale, in_zp, out_scale, out_zp, table);
}

void shl_mi355x_leaky_relu_table_i8(float in_scale, int32_t in_zp, float out_scale, int32_t out_zp, float n, uint8_t table[256])
{
    build_table(f_leaky_relu, n, in_scale, in_zp, out_scale, out_zp, table);
}

/* The gate of a swish / hard-swish as converters export it, act(x) -> mul(x, gate): table[(uint8_t)b] is the byte the
 * reference's mul gives for the operands (b, act(b)) in the layer's operand order.  The gate byte is the activation's own
 * table entry; the product is source/reference/mul.c:23 behind shl_ref_diso_callback_base (utils.c:623-637): both operands
 * dequantised (int8_to_float_base), ONE float32 product, float_to_int8_base.  Nothing contracted, as in build_table */
void shl_mi355x_gate_mul_table_i8(int kind, float x_scale, int32_t x_zp, float gate_scale, int32_t gate_zp, int x_is_first,
                                  float out_scale, int32_t out_zp, uint8_t table[256])
{
    uint8_t gate[256];
    build_table(kind == SHL_MI355X_UNARY_HARD_SIGMOID ? f_hard_sigmoid : f_sigmoid, 0.0f, x_scale, x_zp, gate_scale, gate_zp, gate);
    for (int q = -128; q < 128; q++) {
        const float x = ((float)q - x_zp) * x_scale;
        const float g = ((float)(int8_t)gate[(uint8_t)q] - gate_zp) * gate_scale;
        const float p = x_is_first ? x * g : g * x; /* input0's element times input1's */
        const float ret = nearbyint(p / out_scale) + out_zp;
        int8_t r;
        if (ret > 127) r = 127;
        else if (ret < -128) r = -128;
        else r = (int8_t)ret;
        table[(uint8_t)q] = (uint8_t)r;
    }
}

/* ---- unary callbacks ------------------------------------------------------------------------------------------ */
static float (*const g_unary_f[])(float, float) = {f_sigmoid, f_hard_sigmoid, f_silu, f_leaky_relu}; /* by shl_mi355x_unary_kind */
static const char *const g_unary_name[] = {"sigmoid", "hard_sigmoid", "silu", "leaky_relu"};

static int unary_check(int kind, struct csinn_tensor *input, struct csinn_tensor *output, int *dtype)
{
    const char *op = g_unary_name[kind];
    int rc = shl_mi355x_check_io(op, input, output, dtype);
    if (rc != CSINN_TRUE) return rc;
    if (csinn_tensor_size(input) != csinn_tensor_size(output)) {
        shl_debug_error("mi355x: %s: input and output hold different numbers of elements\n", op);
        return CSINN_FALSE;
    }
    return CSINN_TRUE;
}

static int unary_exec(int kind, float n, struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_params_base *base)
{
    int dtype;
    int rc = unary_check(kind, input, output, &dtype);
    if (rc != CSINN_TRUE) return rc;
    const size_t count = (size_t)csinn_tensor_size(output);
    if (count == 0) return CSINN_TRUE;
    struct shl_mi355x_staged s;
    if (shl_mi355x_staged_begin(base, input, NULL, output, &s) != CSINN_TRUE) return CSINN_FALSE;
    int st;
    if (dtype == SHL_MI355X_I8) {
        uint8_t table[256];
        build_table(g_unary_f[kind], n, input->qinfo->scale, input->qinfo->zero_point, output->qinfo->scale,
                    output->qinfo->zero_point, table);
        st = shl_mi355x_unary_lut_i8(s.in[0], s.out, count, table, s.stream);
    } else {
        st = shl_mi355x_unary_f16(s.in[0], s.out, count, kind, n, s.stream);
    }
    return shl_mi355x_staged_end(g_unary_name[kind], &s, output, st);
}

static int unary_perf(int kind, struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_perf_info *info)
{
    int dtype;
    int rc = unary_check(kind, input, output, &dtype);
    if (rc != CSINN_TRUE) return rc;
    uintptr_t at = SHL_MI355X_PERF_BASE;
    const void *in = (const void *)shl_mi355x_perf_address(input, &at), *out = (const void *)shl_mi355x_perf_address(output, &at);
    info->kernel_name = dtype == SHL_MI355X_F16 ? "unary_f16" : (char *)shl_mi355x_unary_lut_i8_kernel_name(in, out);
    return CSINN_TRUE;
}

int shl_mi355x_sigmoid_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params)
{
    return unary_exec(SHL_MI355X_UNARY_SIGMOID, 0.0f, input, output, &params->base);
}

int shl_mi355x_hard_sigmoid_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params)
{
    return unary_exec(SHL_MI355X_UNARY_HARD_SIGMOID, 0.0f, input, output, &params->base);
}

int shl_mi355x_silu_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params)
{
    return unary_exec(SHL_MI355X_UNARY_SILU, 0.0f, input, output, &params->base);
}

int shl_mi355x_leaky_relu_exec(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_relu_params *params)
{
    return unary_exec(SHL_MI355X_UNARY_LEAKY_RELU, params->n, input, output, &params->base);
}

int shl_mi355x_sigmoid_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params,
                            struct csinn_perf_info *info)
{
    (void)params;
    return unary_perf(SHL_MI355X_UNARY_SIGMOID, input, output, info);
}

int shl_mi355x_hard_sigmoid_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params,
                                 struct csinn_perf_info *info)
{
    (void)params;
    return unary_perf(SHL_MI355X_UNARY_HARD_SIGMOID, input, output, info);
}

int shl_mi355x_silu_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_sigmoid_params *params,
                         struct csinn_perf_info *info)
{
    (void)params;
    return unary_perf(SHL_MI355X_UNARY_SILU, input, output, info);
}

int shl_mi355x_leaky_relu_perf(struct csinn_tensor *input, struct csinn_tensor *output, struct csinn_relu_params *params,
                               struct csinn_perf_info *info)
{
    (void)params;
    return unary_perf(SHL_MI355X_UNARY_LEAKY_RELU, input, output, info);
}

/* ---- mul, and the broadcasting add (pooling.c) ------------------------------------------------------------------ */
/* Which operand has the output's shape (*full) and which is broadcast to it (*small), and the descriptor of the pair.
 * The rule is shl_ref_broadcast_to_shape_f32's (source/reference/utils.c:692-785): ranks right-aligned, every dim of an
 * operand equals the output's or is 1.  The fp32 product and sum are commutative, so the operands may swap.  `op`: "mul" or
 * "add", for the messages */
int shl_mi355x_bcast_prepare(const char *op, struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                             struct csinn_tensor **full, struct csinn_tensor **small, struct shl_mi355x_mul_desc *desc)
{
    int dtype = -1;
    int rc = shl_mi355x_check_tensor(op, "first input", input0, &dtype);
    if (rc == CSINN_TRUE) rc = shl_mi355x_check_tensor(op, "second input", input1, &dtype);
    if (rc == CSINN_TRUE) rc = shl_mi355x_check_tensor(op, "output", output, &dtype);
    if (rc != CSINN_TRUE) return rc;
    const int rank = output->dim_count;
    if (rank < 1 || rank > MAX_DIM) {
        shl_debug_error("%s: a %d-d output\n", op, rank);
        return CSINN_FALSE;
    }
    struct csinn_tensor *in[2] = {input0, input1};
    int same[2];
    for (int k = 0; k < 2; k++) {
        if (in[k]->dim_count < 1 || in[k]->dim_count > rank) {
            shl_debug_error("mi355x: %s: a %d-d operand cannot be broadcast to the %d-d output\n", op, in[k]->dim_count, rank);
            return CSINN_FALSE;
        }
        same[k] = 1;
        for (int i = 0; i < rank; i++) {
            const int j = i - (rank - in[k]->dim_count);
            const int32_t d = j >= 0 ? in[k]->dim[j] : 1;
            if (d != output->dim[i] && d != 1) {
                shl_debug_error("mi355x: %s: dim %d of operand %d is %d, the output's %d: not a broadcast\n", op, j, k, d, output->dim[i]);
                return CSINN_FALSE;
            }
            if (d != output->dim[i]) same[k] = 0;
        }
    }
    if (!same[0] && !same[1]) {
        shl_debug_error("mi355x: %s: both operands need broadcasting, which is not supported\n", op);
        return CSINN_FALSE;
    }
    const int s = same[0] ? 1 : 0; /* the broadcast operand (or the second of two full ones) */
    *full = in[1 - s];
    *small = in[s];
    struct shl_mi355x_mul_desc d;
    memset(&d, 0, sizeof(d));
    d.dtype = dtype;
    /* groups of neighbouring dims along which the small operand varies (1) or is broadcast (0); dims of size 1 join
     * either neighbour */
    int ng = 0, cls[4] = {0, 0, 0, 0};
    for (int i = 0; i < rank; i++) {
        if (output->dim[i] == 1) continue;
        const int j = i - (rank - (*small)->dim_count);
        const int varies = j >= 0 && (*small)->dim[j] != 1;
        if (ng > 0 && cls[ng - 1] == varies) {
            d.dim[ng - 1] *= output->dim[i];
            continue;
        }
        if (ng == 4) {
            shl_debug_error("mi355x: %s: the broadcast pattern has more than 4 groups of dims\n", op);
            return CSINN_FALSE;
        }
        cls[ng] = varies;
        d.dim[ng++] = output->dim[i];
    }
    if (ng == 0) { /* one element, or none */
        d.dim[0] = csinn_tensor_size(output) == 0 ? 0 : 1;
        cls[0] = 1;
        ng = 1;
    }
    int64_t stride = 1;
    for (int g = ng - 1; g >= 0; g--) {
        d.b_stride[g] = cls[g] ? stride : 0;
        if (cls[g]) stride *= d.dim[g];
    }
    d.ngroups = ng;
    d.a_scale = (*full)->qinfo->scale, d.a_zp = (*full)->qinfo->zero_point;
    d.b_scale = (*small)->qinfo->scale, d.b_zp = (*small)->qinfo->zero_point;
    d.out_scale = output->qinfo->scale, d.out_zp = output->qinfo->zero_point;
    d.a_is_second = *full == input1;
    *desc = d;
    return CSINN_TRUE;
}

int shl_mi355x_mul_exec(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                        struct csinn_diso_params *params)
{
    struct csinn_tensor *full, *small;
    struct shl_mi355x_mul_desc d;
    int rc = shl_mi355x_bcast_prepare("mul", input0, input1, output, &full, &small, &d);
    if (rc != CSINN_TRUE) return rc;
    if (csinn_tensor_size(output) == 0) return CSINN_TRUE;
    /* the inputs are staged in their own order, whichever of them is the broadcast one */
    struct shl_mi355x_staged s;
    if (shl_mi355x_staged_begin(&params->base, input0, input1, output, &s) != CSINN_TRUE) return CSINN_FALSE;
    const int a = full == input0 ? 0 : 1;
    int st = shl_mi355x_mul(s.in[a], s.in[1 - a], s.out, &d, s.stream);
    return shl_mi355x_staged_end("mul", &s, output, st);
}

int shl_mi355x_mul_perf(struct csinn_tensor *input0, struct csinn_tensor *input1, struct csinn_tensor *output,
                        struct csinn_diso_params *params, struct csinn_perf_info *info)
{
    (void)params;
    struct csinn_tensor *full, *small;
    struct shl_mi355x_mul_desc d;
    int rc = shl_mi355x_bcast_prepare("mul", input0, input1, output, &full, &small, &d);
    if (rc != CSINN_TRUE) return rc;
    uintptr_t at = SHL_MI355X_PERF_BASE;
    const void *in[2];
    in[0] = (const void *)shl_mi355x_perf_address(input0, &at), in[1] = (const void *)shl_mi355x_perf_address(input1, &at);
    const int a = full == input0 ? 0 : 1;
    info->kernel_name = (char *)shl_mi355x_mul_kernel_name(&d, in[a], in[1 - a], (const void *)shl_mi355x_perf_address(output, &at));
    return CSINN_TRUE;
}

/*
 * setup.c -- registration and run-time services of the MI355X backend.
 *
 * Mirrors the shape of the reference's optimised backends (source/c920v2_opt/setup.c:23-56
 * callback table + lookup with fall-through, :355-389 runtime map forwarding to gref,
 * :391-413 shl_target_init_*), for slot CSINN_MI355X.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "mi355x_internal.h"

/* ------------------------------------------------------------------------ the operator table */
static int conv_caps() { return CSINN_OPT_INTRINSIC; }

static int conv_perf(struct csinn_tensor *input, struct csinn_tensor *output,
                     struct csinn_tensor *kernel, struct csinn_tensor *bias, void *params,
                     struct csinn_perf_info *info)
{
    (void)input; (void)output; (void)kernel; (void)bias;
    info->kernel_name = (char *)shl_mi355x_params_kernel_name(params);
    return CSINN_TRUE;
}

/* the reference's gref has no est for CSINN_OP_GROUP_CONV2D_RELU6 (no such symbol): next to it that row is not registered */
#pragma weak shl_gref_group_conv2d_relu6

/* One row per op id: {op, dtypes, init, exec, est, perf, call shape, activations, first_const}.  shl_target_init_mi355x
 * registers the first six columns; a session (session.c) runs a layer on the device when its op's row has a call shape and
 * the layer's exec callback is still the row's (one that fell through to the reference at init is not) */
#define BOTH (SHL_MI355X_OP_I8 | SHL_MI355X_OP_F16)
#define I8 SHL_MI355X_OP_I8
static const struct shl_mi355x_op g_ops[] = {
    {CSINN_OP_CONV2D, BOTH, shl_mi355x_conv2d_init, shl_mi355x_conv2d_exec, shl_gref_conv2d, conv_perf, CALL_CONV, 1, 1},
    {CSINN_OP_CONV2D_RELU, BOTH, shl_mi355x_conv2d_relu_init, shl_mi355x_conv2d_exec, shl_gref_conv2d_relu, conv_perf, CALL_CONV, 1, 1},
    {CSINN_OP_CONV2D_RELU6, BOTH, shl_mi355x_conv2d_relu6_init, shl_mi355x_conv2d_exec, shl_gref_conv2d_relu6, conv_perf, CALL_CONV, 1, 1},
    {CSINN_OP_DEPTHWISE_CONV2D, BOTH, shl_mi355x_conv2d_init, shl_mi355x_conv2d_exec, shl_gref_depthwise_conv2d, conv_perf, CALL_CONV, 1, 1},
    {CSINN_OP_DEPTHWISE_CONV2D_RELU, BOTH, shl_mi355x_conv2d_relu_init, shl_mi355x_conv2d_exec, shl_gref_depthwise_conv2d_relu, conv_perf,
     CALL_CONV, 1, 1},
    {CSINN_OP_DEPTHWISE_CONV2D_RELU6, BOTH, shl_mi355x_conv2d_relu6_init, shl_mi355x_conv2d_exec, shl_gref_depthwise_conv2d_relu6, conv_perf,
     CALL_CONV, 1, 1},
    {CSINN_OP_GROUP_CONV2D, BOTH, shl_mi355x_conv2d_init, shl_mi355x_group_conv2d_exec, shl_gref_group_conv2d, conv_perf, CALL_CONV, 1, 1},
    {CSINN_OP_GROUP_CONV2D_RELU, BOTH, shl_mi355x_conv2d_relu_init, shl_mi355x_group_conv2d_exec, shl_gref_group_conv2d_relu, conv_perf,
     CALL_CONV, 1, 1},
    {CSINN_OP_GROUP_CONV2D_RELU6, BOTH, shl_mi355x_conv2d_relu6_init, shl_mi355x_group_conv2d_exec, shl_gref_group_conv2d_relu6, conv_perf,
     CALL_CONV, 1, 1},
    /* the learned upsampling of a decoder */
    {CSINN_OP_DECONV2D, BOTH, shl_mi355x_deconv2d_init, shl_mi355x_deconv2d_exec, shl_gref_deconv2d, shl_mi355x_deconv2d_perf, CALL_CONV, 1, 1},
    {CSINN_OP_DEPTHWISE_DECONV2D, BOTH, shl_mi355x_deconv2d_init, shl_mi355x_deconv2d_exec, shl_gref_depthwise_deconv2d,
     shl_mi355x_deconv2d_perf, CALL_CONV, 1, 1},
    /* (refused at init with a message: next to libshl the layer then runs on the reference's kernel) */
    {CSINN_OP_GROUP_DECONV2D, BOTH, shl_mi355x_deconv2d_init, shl_mi355x_deconv2d_exec, shl_gref_group_deconv2d, shl_mi355x_deconv2d_perf,
     CALL_NONE, 0, 0},
    {CSINN_OP_FULLYCONNECTED, BOTH, shl_mi355x_fullyconnected_init, shl_mi355x_fullyconnected_exec, shl_gref_fullyconnected, conv_perf,
     CALL_CONV, 1, 1},
    /* the per-channel op ids exist for int8 only (reference/setup.c:786-808 registers them for every dtype,
     * convolution_channel.c implements u8 / i8); their sessions stay host-staged */
    {CSINN_OP_CONV2D_CHANNEL, I8, shl_mi355x_conv2d_channel_init, shl_mi355x_conv2d_channel_exec, shl_gref_conv2d, conv_perf, CALL_NONE, 0, 0},
    {CSINN_OP_CONV2D_CHANNEL_RELU, I8, shl_mi355x_conv2d_channel_relu_init, shl_mi355x_conv2d_channel_relu_exec, shl_gref_conv2d_relu,
     conv_perf, CALL_NONE, 0, 0},
    {CSINN_OP_CONV2D_CHANNEL_RELU6, I8, shl_mi355x_conv2d_channel_relu6_init, shl_mi355x_conv2d_channel_relu6_exec, shl_gref_conv2d_relu6,
     conv_perf, CALL_NONE, 0, 0},
    {CSINN_OP_GROUP_CONV2D_CHANNEL, I8, shl_mi355x_group_conv2d_channel_init, shl_mi355x_group_conv2d_channel_exec, shl_gref_group_conv2d,
     conv_perf, CALL_NONE, 0, 0},
    {CSINN_OP_GROUP_CONV2D_CHANNEL_RELU, I8, shl_mi355x_group_conv2d_channel_relu_init, shl_mi355x_group_conv2d_channel_relu_exec,
     shl_gref_group_conv2d_relu, conv_perf, CALL_NONE, 0, 0},
    {CSINN_OP_DEPTHWISE_CONV2D_CHANNEL, I8, shl_mi355x_depthwise_conv2d_channel_init, shl_mi355x_depthwise_conv2d_channel_exec,
     shl_gref_depthwise_conv2d, conv_perf, CALL_NONE, 0, 0},
    {CSINN_OP_DEPTHWISE_CONV2D_CHANNEL_RELU, I8, shl_mi355x_depthwise_conv2d_channel_relu_init, shl_mi355x_depthwise_conv2d_channel_relu_exec,
     shl_gref_depthwise_conv2d_relu, conv_perf, CALL_NONE, 0, 0},
    {CSINN_OP_DEPTHWISE_CONV2D_CHANNEL_RELU6, I8, shl_mi355x_depthwise_conv2d_channel_relu6_init, shl_mi355x_depthwise_conv2d_channel_relu6_exec,
     shl_gref_depthwise_conv2d_relu6, conv_perf, CALL_NONE, 0, 0},
    {CSINN_OP_RELU, BOTH, NULL, shl_mi355x_relu_exec, shl_gref_relu, conv_perf, CALL_SISO, 1, 1},
    {CSINN_OP_RELU6, BOTH, NULL, shl_mi355x_relu6_exec, shl_gref_relu6, conv_perf, CALL_SISO, 1, 1},
    {CSINN_OP_GLOBAL_AVGPOOL2D, BOTH, NULL, shl_mi355x_global_avgpool2d_exec, shl_gref_global_avgpool2d, conv_perf, CALL_SISO, 1, 1},
    {CSINN_OP_MAXPOOL2D, BOTH, NULL, shl_mi355x_maxpool2d_exec, shl_gref_maxpool2d, shl_mi355x_maxpool2d_perf, CALL_SISO, 1, 1},
    {CSINN_OP_AVGPOOL2D, BOTH, NULL, shl_mi355x_avgpool2d_exec, shl_gref_avgpool2d, shl_mi355x_avgpool2d_perf, CALL_SISO, 1, 1},
    {CSINN_OP_SOFTMAX, BOTH, NULL, shl_mi355x_softmax_exec, shl_gref_softmax, conv_perf, CALL_SISO, 1, 1},
    /* either operand may be a constant (a bias, a mask, a positional embedding) and may be broadcast to the other */
    {CSINN_OP_ADD, BOTH, NULL, shl_mi355x_add_exec, shl_gref_add, shl_mi355x_add_perf, CALL_DISO, 2, 0},
    /* ... and may be broadcast (an SE gate, a per-channel scale) */
    {CSINN_OP_MUL, BOTH, NULL, shl_mi355x_mul_exec, shl_gref_mul, shl_mi355x_mul_perf, CALL_DISO, 2, 1},
    {CSINN_OP_SIGMOID, BOTH, NULL, shl_mi355x_sigmoid_exec, shl_gref_sigmoid, shl_mi355x_sigmoid_perf, CALL_SISO, 1, 1},
    {CSINN_OP_HARD_SIGMOID, BOTH, NULL, shl_mi355x_hard_sigmoid_exec, shl_gref_hard_sigmoid, shl_mi355x_hard_sigmoid_perf, CALL_SISO, 1, 1},
    {CSINN_OP_SILU, BOTH, NULL, shl_mi355x_silu_exec, shl_gref_silu, shl_mi355x_silu_perf, CALL_SISO, 1, 1},
    {CSINN_OP_LEAKY_RELU, BOTH, NULL, shl_mi355x_leaky_relu_exec, shl_gref_leaky_relu, shl_mi355x_leaky_relu_perf, CALL_SISO, 1, 1},
    /* an FPN top-down path, a U-Net decoder, a YOLO neck */
    {CSINN_OP_RESIZE, BOTH, NULL, shl_mi355x_resize_exec, shl_gref_resize, shl_mi355x_resize_perf, CALL_SISO, 1, 1},
    /* any input may be a constant */
    {CSINN_OP_CONCAT, BOTH, NULL, shl_mi355x_concat_exec, shl_gref_concat, shl_mi355x_concat_perf, CALL_ARRAY, 0, 0},
    /* from here on: a layer the op refuses falls through at init (next to libshl it runs on the reference's kernel) */
    /* a ShuffleNetV2 unit, a CSP / C2f block */
    {CSINN_OP_SPLIT, BOTH, shl_mi355x_split_init, shl_mi355x_split_exec, shl_gref_split, shl_mi355x_split_perf, CALL_SPLIT, 1, 1},
    {CSINN_OP_SHUFFLE_CHANNEL, BOTH, shl_mi355x_shuffle_channel_init, shl_mi355x_shuffle_channel_exec, shl_gref_shuffle_channel,
     shl_mi355x_shuffle_channel_perf, CALL_SISO, 1, 1},
    /* order and shape only: a detection head, an attention block, TensorFlow's SAME padding, the classifier's flatten */
    {CSINN_OP_TRANSPOSE, BOTH, shl_mi355x_transpose_init, shl_mi355x_transpose_exec, shl_gref_transpose, shl_mi355x_transpose_perf,
     CALL_SISO, 1, 1},
    /* (one copy node; sharing the producer's buffer is a later change) */
    {CSINN_OP_RESHAPE, BOTH, shl_mi355x_reshape_init, shl_mi355x_reshape_exec, shl_gref_reshape, shl_mi355x_reshape_perf, CALL_SISO, 1, 1},
    {CSINN_OP_FLATTEN, BOTH, shl_mi355x_flatten_init, shl_mi355x_flatten_exec, shl_gref_flatten, shl_mi355x_flatten_perf, CALL_SISO, 1, 1},
    {CSINN_OP_PAD, BOTH, shl_mi355x_pad_init, shl_mi355x_pad_exec, shl_gref_pad, shl_mi355x_pad_perf, CALL_SISO, 1, 1},
    /* QK^T and PV of an attention block (two activations), a linear layer exported as MatMul (the second operand a constant) */
    {CSINN_OP_MATMUL, BOTH, shl_mi355x_matmul_init, shl_mi355x_matmul_exec, shl_gref_matmul, shl_mi355x_matmul_perf, CALL_DISO, 2, 1},
    /* reductions: TensorFlow's global pooling (mean over H and W), CBAM's channel max / mean and global max pool, a head's
     * reduce_max / reduce_sum */
    {CSINN_OP_MEAN, BOTH, shl_mi355x_mean_init, shl_mi355x_mean_exec, shl_gref_mean, shl_mi355x_mean_perf, CALL_SISO, 1, 1},
    {CSINN_OP_SUM, BOTH, shl_mi355x_sum_init, shl_mi355x_sum_exec, shl_gref_sum, shl_mi355x_sum_perf, CALL_SISO, 1, 1},
    {CSINN_OP_MAX, BOTH, shl_mi355x_max_init, shl_mi355x_max_exec, shl_gref_max, shl_mi355x_max_perf, CALL_SISO, 1, 1},
    {CSINN_OP_MIN, BOTH, shl_mi355x_min_init, shl_mi355x_min_exec, shl_gref_min, shl_mi355x_min_perf, CALL_SISO, 1, 1},
    {CSINN_OP_REDUCE_MEAN, BOTH, shl_mi355x_reduce_mean_init, shl_mi355x_reduce_mean_exec, shl_gref_reduce_mean, shl_mi355x_reduce_mean_perf,
     CALL_SISO, 1, 1},
    {CSINN_OP_REDUCE_SUM, BOTH, shl_mi355x_reduce_sum_init, shl_mi355x_reduce_sum_exec, shl_gref_reduce_sum, shl_mi355x_reduce_sum_perf,
     CALL_SISO, 1, 1},
    {CSINN_OP_REDUCE_MAX, BOTH, shl_mi355x_reduce_max_init, shl_mi355x_reduce_max_exec, shl_gref_reduce_max, shl_mi355x_reduce_max_perf,
     CALL_SISO, 1, 1},
    {CSINN_OP_REDUCE_MIN, BOTH, shl_mi355x_reduce_min_init, shl_mi355x_reduce_min_exec, shl_gref_reduce_min, shl_mi355x_reduce_min_perf,
     CALL_SISO, 1, 1},
    {CSINN_OP_GLOBAL_MAXPOOL2D, BOTH, shl_mi355x_global_maxpool2d_init, shl_mi355x_global_maxpool2d_exec, shl_gref_global_maxpool2d,
     shl_mi355x_global_maxpool2d_perf, CALL_SISO, 1, 1},
};
#undef BOTH
#undef I8
#define N_OPS (sizeof(g_ops) / sizeof(g_ops[0]))

const struct shl_mi355x_op *shl_mi355x_op_row(int type)
{
    for (size_t i = 0; i < N_OPS; i++)
        if (g_ops[i].type == type) return &g_ops[i];
    return NULL;
}

/* what shl_target_init_mi355x made of the rows: [row][0] int8, [row][1] binary16; exec == NULL: not registered */
static struct csinn_callback g_cb[N_OPS][2];

/* present when the backend is loaded next to the genuine library: unsupported (op, dtype)
 * pairs fall through to the C reference, as c920v2 falls through to rvv */
struct csinn_callback *shl_cb_map_ref(int op, int dtype) __attribute__((weak));

struct csinn_callback *shl_cb_map_mi355x(int op, int dtype)
{
    const struct shl_mi355x_op *row = shl_mi355x_op_row(op);
    if (row && (dtype == CSINN_DTYPE_INT8 || dtype == CSINN_DTYPE_FLOAT16)) {
        struct csinn_callback *cb = &g_cb[row - g_ops][dtype == CSINN_DTYPE_FLOAT16];
        if (cb->exec) return cb;
    }
    if (shl_cb_map_ref) return shl_cb_map_ref(op, dtype);
    return NULL;
}

/* ------------------------------------------------------------------------ execution contexts
 * SURVEY 8(b) "Threading": a GPU backend serialises its own stream use PER SESSION.  Every csinn
 * session (layer-mode sessions included: params->base.sess) owns one context = the HIP stream its exec
 * callbacks enqueue on + the HBM staging buffers host tensors travel through.  Two sessions therefore
 * never share a staging buffer or an ordering assumption; a layer-mode call cannot disturb a session
 * graph in flight.  A context without an explicit stream uses the process default set by
 * shl_mi355x_set_stream (NULL = HIP's default stream). */
struct shl_mi355x_ctx {
    struct csinn_session *sess;
    void *stream;
    int own_stream; /* stream was set for this session explicitly */
    struct {
        void *dev;
        size_t bytes;
    } stage[3]; /* 0: first input (concat: all of them, packed), 1: output (split: all of them, packed), 2: second input */
    struct shl_mi355x_ctx *next;
};

static void *g_default_stream;
static struct shl_mi355x_ctx *g_ctx;
static pthread_mutex_t g_ctx_lock = PTHREAD_MUTEX_INITIALIZER;

void shl_mi355x_set_stream(void *stream) { g_default_stream = stream; }
void *shl_mi355x_get_stream(void) { return g_default_stream; }

struct shl_mi355x_ctx *shl_mi355x_ctx_of(struct csinn_session *sess)
{
    pthread_mutex_lock(&g_ctx_lock);
    struct shl_mi355x_ctx *c = g_ctx;
    while (c && c->sess != sess) c = c->next;
    if (c == NULL) {
        c = calloc(1, sizeof(*c));
        if (c) {
            c->sess = sess;
            c->next = g_ctx;
            g_ctx = c;
        }
    }
    pthread_mutex_unlock(&g_ctx_lock);
    return c;
}

void *shl_mi355x_ctx_stream(struct shl_mi355x_ctx *ctx)
{
    return ctx && ctx->own_stream ? ctx->stream : g_default_stream;
}

static int ctx_has_staging(struct shl_mi355x_ctx *c) { return c->stage[0].dev || c->stage[1].dev || c->stage[2].dev; }

void shl_mi355x_session_set_stream(struct csinn_session *sess, void *stream)
{
    struct shl_mi355x_ctx *c = shl_mi355x_ctx_of(sess);
    if (c == NULL) return;
    /* staged uploads still queued on the previous stream must land before another stream reuses
     * the staging buffers */
    if (ctx_has_staging(c)) shl_mi355x_stream_sync(shl_mi355x_ctx_stream(c));
    c->stream = stream;
    c->own_stream = 1;
}

/* back to the process default stream (shl_mi355x_set_stream), followed from now on */
void shl_mi355x_session_inherit_stream(struct csinn_session *sess)
{
    struct shl_mi355x_ctx *c = shl_mi355x_ctx_of(sess);
    if (c == NULL) return;
    if (ctx_has_staging(c)) shl_mi355x_stream_sync(shl_mi355x_ctx_stream(c));
    c->stream = NULL;
    c->own_stream = 0;
}

int shl_mi355x_session_has_own_stream(struct csinn_session *sess)
{
    struct shl_mi355x_ctx *c = shl_mi355x_ctx_of(sess);
    return c && c->own_stream;
}

void *shl_mi355x_session_stream(struct csinn_session *sess)
{
    return shl_mi355x_ctx_stream(shl_mi355x_ctx_of(sess));
}

/* drop the context of `sess`: waits for its stream, frees its staging buffers (the stream itself
 * belongs to whoever created it) */
void shl_mi355x_ctx_release(struct csinn_session *sess)
{
    pthread_mutex_lock(&g_ctx_lock);
    struct shl_mi355x_ctx **pp = &g_ctx, *dead = NULL;
    while (*pp) {
        if ((*pp)->sess == sess) {
            dead = *pp;
            *pp = dead->next;
            break;
        }
        pp = &(*pp)->next;
    }
    pthread_mutex_unlock(&g_ctx_lock);
    if (dead == NULL) return;
    if (ctx_has_staging(dead)) shl_mi355x_stream_sync(shl_mi355x_ctx_stream(dead));
    for (int i = 0; i < 3; i++)
        if (dead->stage[i].dev) shl_mi355x_free(dead->stage[i].dev);
    free(dead);
}

/* ------------------------------------------------------------------------ plan registry
 * params block -> device plan(s).  A grouped convolution keeps one plan per group in `sub`. */
struct slot {
    void *key;
    shl_mi355x_conv_plan *plan;
    shl_mi355x_conv_plan **sub;
    int nsub;
    void *tag; /* what the plan was built from, for callbacks that plan at exec time (CSINN_OP_*_CHANNEL): lives and
                * dies with the plan, so there is no second table to fill up or to go stale */
    size_t tag_bytes;
};
static struct slot *g_slots;
static size_t g_cap, g_used;
static int64_t g_stored; /* plans (or plan groups) ever bound: see shl_mi355x_plans_created */
static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;
#define TOMBSTONE ((void *)(uintptr_t)1)

static size_t hash_ptr(void *p, size_t cap)
{
    uint64_t x = (uint64_t)(uintptr_t)p;
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    return (size_t)x & (cap - 1);
}

static void rehash(size_t cap)
{
    struct slot *old = g_slots;
    size_t old_cap = g_cap;
    g_slots = calloc(cap, sizeof(struct slot));
    g_cap = cap;
    g_used = 0;
    for (size_t i = 0; i < old_cap; i++) {
        if (old[i].key == NULL || old[i].key == TOMBSTONE) continue;
        size_t h = hash_ptr(old[i].key, cap);
        while (g_slots[h].key) h = (h + 1) & (cap - 1);
        g_slots[h] = old[i];
        g_used++;
    }
    free(old);
}

static struct slot *find(void *params);

static void destroy_contents(struct slot *s)
{
    if (s->plan) shl_mi355x_conv_plan_destroy(s->plan);
    for (int i = 0; i < s->nsub; i++)
        if (s->sub[i]) shl_mi355x_conv_plan_destroy(s->sub[i]);
    free(s->sub);
    free(s->tag);
}

/* (re)binds `params` to a plan, or to `nsub` per-group plans (ownership of the array passes) */
static void registry_store(void *params, shl_mi355x_conv_plan *plan, shl_mi355x_conv_plan **sub, int nsub)
{
    pthread_mutex_lock(&g_lock);
    if (g_cap == 0 || (g_used + 1) * 2 > g_cap) rehash(g_cap ? g_cap * 2 : 64);
    size_t h = hash_ptr(params, g_cap);
    struct slot stale = {0};
    for (;;) {
        if (g_slots[h].key == params) { /* re-init of the same layer replaces the plan */
            stale = g_slots[h];
            break;
        }
        if (g_slots[h].key == NULL) {
            g_slots[h].key = params;
            g_used++;
            break;
        }
        h = (h + 1) & (g_cap - 1);
    }
    g_slots[h].plan = plan;
    g_slots[h].sub = sub;
    g_slots[h].nsub = nsub;
    g_slots[h].tag = NULL;
    g_slots[h].tag_bytes = 0;
    g_stored++;
    pthread_mutex_unlock(&g_lock);
    destroy_contents(&stale);
}

int64_t shl_mi355x_plans_created(void)
{
    pthread_mutex_lock(&g_lock);
    const int64_t n = g_stored;
    pthread_mutex_unlock(&g_lock);
    return n;
}

/* attach a copy of `tag` to the plan bound to `params` (replaces an earlier one) */
void shl_mi355x_registry_set_tag(void *params, const void *tag, size_t bytes)
{
    void *copy = malloc(bytes ? bytes : 1);
    if (copy == NULL) return;
    memcpy(copy, tag, bytes);
    pthread_mutex_lock(&g_lock);
    struct slot *s = find(params);
    void *old = NULL;
    if (s) {
        old = s->tag;
        s->tag = copy;
        s->tag_bytes = bytes;
        copy = NULL;
    }
    pthread_mutex_unlock(&g_lock);
    free(old);
    free(copy);
}

/* 1 when `params` has a plan whose tag equals these bytes */
int shl_mi355x_registry_tag_matches(void *params, const void *tag, size_t bytes)
{
    pthread_mutex_lock(&g_lock);
    struct slot *s = find(params);
    const int hit = s && (s->plan || s->nsub) && s->tag && s->tag_bytes == bytes && memcmp(s->tag, tag, bytes) == 0;
    pthread_mutex_unlock(&g_lock);
    return hit;
}

void shl_mi355x_registry_put(void *params, shl_mi355x_conv_plan *plan) { registry_store(params, plan, NULL, 0); }

void shl_mi355x_registry_put_group(void *params, shl_mi355x_conv_plan **plans, int n)
{
    registry_store(params, NULL, plans, n);
}

static struct slot *find(void *params)
{
    if (g_cap == 0) return NULL;
    size_t h = hash_ptr(params, g_cap);
    for (size_t probes = 0; probes < g_cap; probes++) {
        if (g_slots[h].key == params) return &g_slots[h];
        if (g_slots[h].key == NULL) return NULL;
        h = (h + 1) & (g_cap - 1);
    }
    return NULL;
}

shl_mi355x_conv_plan *shl_mi355x_registry_get(void *params)
{
    pthread_mutex_lock(&g_lock);
    struct slot *s = find(params);
    shl_mi355x_conv_plan *p = s ? s->plan : NULL;
    pthread_mutex_unlock(&g_lock);
    return p;
}

shl_mi355x_conv_plan *shl_mi355x_registry_get_group(void *params, int i)
{
    pthread_mutex_lock(&g_lock);
    struct slot *s = find(params);
    shl_mi355x_conv_plan *p = s && i >= 0 && i < s->nsub ? s->sub[i] : NULL;
    pthread_mutex_unlock(&g_lock);
    return p;
}

int shl_mi355x_release_params(void *params)
{
    pthread_mutex_lock(&g_lock);
    struct slot *s = find(params);
    struct slot dead = {0};
    if (s) {
        dead = *s;
        s->key = TOMBSTONE;
        s->plan = NULL;
        s->sub = NULL;
        s->nsub = 0;
        s->tag = NULL;
        s->tag_bytes = 0;
    }
    pthread_mutex_unlock(&g_lock);
    if (dead.plan == NULL && dead.nsub == 0) return CSINN_FALSE;
    destroy_contents(&dead);
    return CSINN_TRUE;
}

int shl_mi355x_live_plans(int64_t *hbm_bytes)
{
    int n = 0;
    int64_t bytes = 0;
    pthread_mutex_lock(&g_lock);
    for (size_t i = 0; i < g_cap; i++) {
        if (g_slots[i].key == NULL || g_slots[i].key == TOMBSTONE) continue;
        if (g_slots[i].plan) {
            n++;
            bytes += (int64_t)shl_mi355x_conv_plan_bytes(g_slots[i].plan);
        }
        for (int k = 0; k < g_slots[i].nsub; k++)
            if (g_slots[i].sub[k]) {
                n++;
                bytes += (int64_t)shl_mi355x_conv_plan_bytes(g_slots[i].sub[k]);
            }
    }
    pthread_mutex_unlock(&g_lock);
    if (hbm_bytes) *hbm_bytes = bytes;
    return n;
}

void *shl_mi355x_params_const_block(void *params, size_t *bytes)
{
    shl_mi355x_conv_plan *p = shl_mi355x_registry_get(params);
    return p ? shl_mi355x_conv_plan_const_block(p, bytes) : NULL;
}

const char *shl_mi355x_params_kernel_name(void *params)
{
    shl_mi355x_conv_plan *p = shl_mi355x_registry_get(params);
    if (p == NULL) p = shl_mi355x_registry_get_group(params, 0);
    return p ? shl_mi355x_conv_plan_kernel_name(p) : "";
}

/* One-time weight broadcast of a set of layers: the constant blocks of the plans attached to
 * `params[0..n)` travel from rank `root` to every rank of `comm` (shl_mi355x_comm_create) as one RCCL
 * group on the session's stream; returns once they have landed.  Every rank must have initialised the
 * same layers (same shapes -> same block sizes); only the root's weights matter. */
int shl_mi355x_bcast_const_blocks(void *comm, void **params, int32_t n, int32_t root, struct csinn_session *sess)
{
    if (n <= 0) return CSINN_TRUE;
    /* a grouped convolution keeps one plan per group: every one of them travels */
    int total = 0;
    for (int i = 0; i < n; i++) {
        int g = 0;
        while (shl_mi355x_registry_get_group(params[i], g)) g++;
        total += g ? g : 1;
    }
    shl_mi355x_conv_plan **plans = calloc((size_t)total, sizeof(*plans));
    void **blocks = calloc((size_t)total, sizeof(void *));
    size_t *bytes = calloc((size_t)total, sizeof(size_t));
    int rc = CSINN_TRUE, k = 0;
    for (int i = 0; i < n && rc == CSINN_TRUE; i++) {
        shl_mi355x_conv_plan *p = shl_mi355x_registry_get(params[i]);
        if (p) {
            plans[k++] = p;
        } else {
            int g = 0;
            while ((p = shl_mi355x_registry_get_group(params[i], g)) != NULL) plans[k++] = p, g++;
            if (g == 0) {
                shl_debug_error("mi355x: bcast_const_blocks: layer %d has no device plan\n", i);
                rc = CSINN_FALSE;
            }
        }
    }
    for (int i = 0; i < k; i++) blocks[i] = shl_mi355x_conv_plan_const_block(plans[i], &bytes[i]);
    void *stream = shl_mi355x_session_stream(sess);
    if (rc == CSINN_TRUE && (shl_mi355x_comm_bcast(comm, blocks, bytes, k, root, stream) != SHL_MI355X_OK ||
                             shl_mi355x_stream_sync(stream) != SHL_MI355X_OK)) {
        shl_debug_error("mi355x: weight broadcast failed: %s\n", shl_mi355x_last_error());
        rc = CSINN_FALSE;
    }
    /* tables and the code path chosen for them come from the same rank: the root's flags record is in the block */
    for (int i = 0; i < k && rc == CSINN_TRUE; i++)
        if (shl_mi355x_conv_plan_adopt_block(plans[i], stream) != SHL_MI355X_OK) {
            shl_debug_error("mi355x: bcast_const_blocks: %s\n", shl_mi355x_last_error());
            rc = CSINN_FALSE;
        }
    free(plans);
    free(blocks);
    free(bytes);
    return rc;
}

/* the same adoption for a caller that moved the constant blocks itself (any transport): every plan of
 * `params[0..n)` takes the epilogue choices of the flags record now in its block */
int shl_mi355x_params_adopt_blocks(void **params, int32_t n, struct csinn_session *sess)
{
    void *stream = shl_mi355x_session_stream(sess);
    for (int i = 0; i < n; i++) {
        shl_mi355x_conv_plan *p = shl_mi355x_registry_get(params[i]);
        int g = 0;
        if (p == NULL) p = shl_mi355x_registry_get_group(params[i], g++);
        if (p == NULL) {
            shl_debug_error("mi355x: params_adopt_blocks: layer %d has no device plan\n", i);
            return CSINN_FALSE;
        }
        while (p) {
            if (shl_mi355x_conv_plan_adopt_block(p, stream) != SHL_MI355X_OK) {
                shl_debug_error("mi355x: params_adopt_blocks: %s\n", shl_mi355x_last_error());
                return CSINN_FALSE;
            }
            p = g ? shl_mi355x_registry_get_group(params[i], g++) : NULL;
        }
    }
    return CSINN_TRUE;
}

/* ------------------------------------------------------------------------ staging */
static void *stage_buffer(struct shl_mi355x_ctx *c, int slot, size_t bytes)
{
    if (c->stage[slot].bytes >= bytes && c->stage[slot].dev) return c->stage[slot].dev;
    if (c->stage[slot].dev) {
        /* kernels that still read the old buffer must finish before it is freed */
        shl_mi355x_stream_sync(shl_mi355x_ctx_stream(c));
        shl_mi355x_free(c->stage[slot].dev);
    }
    size_t want = bytes < (1u << 20) ? (1u << 20) : bytes + bytes / 2;
    c->stage[slot].dev = shl_mi355x_malloc(want);
    c->stage[slot].bytes = c->stage[slot].dev ? want : 0;
    if (c->stage[slot].dev == NULL)
        shl_debug_error("mi355x: cannot allocate %zu bytes of HBM: %s\n", want, shl_mi355x_last_error());
    return c->stage[slot].dev;
}

const void *shl_mi355x_stage_in(struct shl_mi355x_ctx *c, struct csinn_tensor *t, int slot)
{
    if (t->data == NULL) {
        shl_debug_error("mi355x: input tensor has no data\n");
        return NULL;
    }
    if (t->mtype == CSINN_MEM_TYPE_DMABUF) return t->data;
    if (c == NULL) return NULL;
    const size_t bytes = (size_t)csinn_tensor_byte_size(t);
    void *dev = stage_buffer(c, slot, bytes);
    if (dev == NULL) return NULL;
    if (shl_mi355x_upload(dev, t->data, bytes, shl_mi355x_ctx_stream(c)) != SHL_MI355X_OK) {
        shl_debug_error("mi355x: upload failed: %s\n", shl_mi355x_last_error());
        return NULL;
    }
    return dev;
}

/* the inputs of a variadic layer: one staging buffer (slot 0, grown as for a single tensor) holds every host tensor */
int shl_mi355x_stage_in_many(struct shl_mi355x_ctx *c, struct csinn_tensor **t, int n, const void **dev)
{
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        dev[i] = NULL;
        if (csinn_tensor_size(t[i]) == 0) continue;
        if (t[i]->data == NULL) {
            shl_debug_error("mi355x: input tensor %d has no data\n", i);
            return CSINN_FALSE;
        }
        if (t[i]->mtype == CSINN_MEM_TYPE_DMABUF) continue;
        int seen = 0; /* the same tensor given twice travels once */
        for (int j = 0; j < i && !seen; j++) seen = t[j] == t[i];
        if (seen) continue;
        const size_t bytes = (size_t)csinn_tensor_byte_size(t[i]);
        total += (bytes + SHL_MI355X_STAGE_ALIGN - 1) / SHL_MI355X_STAGE_ALIGN * SHL_MI355X_STAGE_ALIGN;
    }
    char *base = NULL;
    if (total > 0) {
        if (c == NULL) return CSINN_FALSE;
        base = stage_buffer(c, 0, total);
        if (base == NULL) return CSINN_FALSE;
    }
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        if (csinn_tensor_size(t[i]) == 0) continue;
        if (t[i]->mtype == CSINN_MEM_TYPE_DMABUF) {
            dev[i] = t[i]->data;
            continue;
        }
        for (int j = 0; j < i && dev[i] == NULL; j++)
            if (t[j] == t[i]) dev[i] = dev[j];
        if (dev[i] != NULL) continue;
        const size_t bytes = (size_t)csinn_tensor_byte_size(t[i]);
        if (shl_mi355x_upload(base + at, t[i]->data, bytes, shl_mi355x_ctx_stream(c)) != SHL_MI355X_OK) {
            shl_debug_error("mi355x: upload failed: %s\n", shl_mi355x_last_error());
            return CSINN_FALSE;
        }
        dev[i] = base + at;
        at += (bytes + SHL_MI355X_STAGE_ALIGN - 1) / SHL_MI355X_STAGE_ALIGN * SHL_MI355X_STAGE_ALIGN;
    }
    return CSINN_TRUE;
}

void *shl_mi355x_stage_out_begin(struct shl_mi355x_ctx *c, struct csinn_tensor *t, int slot)
{
    if (t->data == NULL) {
        shl_debug_error("mi355x: output tensor has no data\n");
        return NULL;
    }
    if (t->mtype == CSINN_MEM_TYPE_DMABUF) return t->data;
    if (c == NULL) return NULL;
    return stage_buffer(c, slot, (size_t)csinn_tensor_byte_size(t));
}

/* the outputs of a layer with several (split): one staging buffer (slot 1, grown as for a single tensor) holds every host
 * tensor at SHL_MI355X_STAGE_ALIGN-aligned offsets, DMABUF tensors are written in place; dev[i]: where the kernel writes
 * tensor i.  Nothing is allocated when a tensor has no data: the caller then has written nothing */
int shl_mi355x_stage_out_many_begin(struct shl_mi355x_ctx *c, struct csinn_tensor **t, int n, void **dev)
{
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        dev[i] = NULL;
        if (t[i]->data == NULL) {
            shl_debug_error("mi355x: output tensor %d has no data\n", i);
            return CSINN_FALSE;
        }
        if (t[i]->mtype == CSINN_MEM_TYPE_DMABUF) continue;
        const size_t bytes = (size_t)csinn_tensor_byte_size(t[i]);
        total += (bytes + SHL_MI355X_STAGE_ALIGN - 1) / SHL_MI355X_STAGE_ALIGN * SHL_MI355X_STAGE_ALIGN;
    }
    char *base = NULL;
    if (total > 0) {
        if (c == NULL) return CSINN_FALSE;
        base = stage_buffer(c, 1, total);
        if (base == NULL) return CSINN_FALSE;
    }
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        if (t[i]->mtype == CSINN_MEM_TYPE_DMABUF) {
            dev[i] = t[i]->data;
            continue;
        }
        dev[i] = base + at;
        const size_t bytes = (size_t)csinn_tensor_byte_size(t[i]);
        at += (bytes + SHL_MI355X_STAGE_ALIGN - 1) / SHL_MI355X_STAGE_ALIGN * SHL_MI355X_STAGE_ALIGN;
    }
    return CSINN_TRUE;
}

/* downloads the host tensors among them, then synchronises once */
int shl_mi355x_stage_out_many_end(struct shl_mi355x_ctx *c, struct csinn_tensor **t, int n, void *const *dev)
{
    void *stream = shl_mi355x_ctx_stream(c);
    int host = 0;
    for (int i = 0; i < n; i++) {
        if (t[i]->mtype == CSINN_MEM_TYPE_DMABUF) continue; /* stays in HBM, stays async */
        host++;
        if (shl_mi355x_download(t[i]->data, dev[i], (size_t)csinn_tensor_byte_size(t[i]), stream) != SHL_MI355X_OK) {
            shl_debug_error("mi355x: download failed: %s\n", shl_mi355x_last_error());
            return CSINN_FALSE;
        }
    }
    if (host > 0 && shl_mi355x_stream_sync(stream) != SHL_MI355X_OK) {
        shl_debug_error("mi355x: download failed: %s\n", shl_mi355x_last_error());
        return CSINN_FALSE;
    }
    return CSINN_TRUE;
}

int shl_mi355x_stage_out_end(struct shl_mi355x_ctx *c, struct csinn_tensor *t, void *dev)
{
    if (t->mtype == CSINN_MEM_TYPE_DMABUF) return CSINN_TRUE; /* stays in HBM, stays async */
    void *stream = shl_mi355x_ctx_stream(c);
    if (shl_mi355x_download(t->data, dev, (size_t)csinn_tensor_byte_size(t), stream) != SHL_MI355X_OK ||
        shl_mi355x_stream_sync(stream) != SHL_MI355X_OK) {
        shl_debug_error("mi355x: download failed: %s\n", shl_mi355x_last_error());
        return CSINN_FALSE;
    }
    return CSINN_TRUE;
}

/* IEEE binary16 -> binary32, exact (float16_to_float32_base, source/nn2/utils.c:624-643) */
float shl_mi355x_half_to_float(uint16_t h)
{
    union { uint32_t u; float f; } v, up, lim;
    up.u = (254u - 15u) << 23;
    lim.u = (127u + 16u) << 23;
    v.u = (uint32_t)(h & 0x7FFFu) << 13;
    v.f = v.f * up.f;
    if (v.f >= lim.f) v.u |= 255u << 23;
    v.u |= (uint32_t)(h & 0x8000u) << 16;
    return v.f;
}

/* ------------------------------------------------------------------------ runtime map */
void *shl_mi355x_runtime_callback(int op)
{
    /* graph construction is served by the graph executor; setup / run / deinit are wrapped so
     * that all-GPU sessions execute device-resident as one hipGraph (session.c) */
    switch (op) {
        case CSINN_SESSION_SETUP: return shl_mi355x_session_setup;
        case CSINN_SESSION_RUN: return shl_mi355x_session_run;
        case CSINN_SESSION_DEINIT: return shl_mi355x_session_deinit;
        default: return shl_gref_runtime_callback(op);
    }
}

void shl_target_init_mi355x(void)
{
    static int done;
    if (done) return;
    done = 1;
    for (size_t i = 0; i < N_OPS; i++) {
        const struct shl_mi355x_op *row = &g_ops[i];
        if (row->est == NULL) continue; /* (the weak shl_gref_group_conv2d_relu6) */
        for (int f16 = 0; f16 < 2; f16++)
            if (row->dtypes & (f16 ? SHL_MI355X_OP_F16 : SHL_MI355X_OP_I8))
                g_cb[i][f16] = (struct csinn_callback){
                    .init = row->init, .exec = row->exec, .est = row->est, .caps = conv_caps, .perf = row->perf};
    }
    shl_register_op_callback(CSINN_MI355X, shl_cb_map_mi355x);
    shl_register_runtime_callback(CSINN_MI355X, shl_mi355x_runtime_callback);
    /* SHL_MI355X_SLOT=<api>: occupy one more dispatch slot, see shl_target_init_mi355x_slot */
    const char *slot = getenv("SHL_MI355X_SLOT");
    if (slot && *slot) shl_target_init_mi355x_slot(atoi(slot));
}

/* The backend under another backend's name.  Programs generated for a RISC-V target hard-code that target's
 * dispatch slot (example/c906_mobilenetv1_f16.c:24: `sess->base_api = CSINN_C906`); on a host whose libshl does not
 * contain that target the slot is empty, and registering there lets such a program run UNCHANGED on the GPU.
 * Nothing in the backend depends on the slot number: callbacks are found through params->base.api / sess->base_api,
 * whatever they are (source/nn2/setup.c:101-125). */
int shl_target_init_mi355x_slot(int api)
{
    if (api < 0 || api >= CSINN_API_SIZE || api == CSINN_REF || api == CSINN_GREF) {
        shl_debug_error("mi355x: dispatch slot %d cannot be taken\n", api);
        return CSINN_FALSE;
    }
    shl_target_init_mi355x();
    if (api != CSINN_MI355X) {
        shl_register_op_callback(api, shl_cb_map_mi355x);
        shl_register_runtime_callback(api, shl_mi355x_runtime_callback);
    }
    return CSINN_TRUE;
}

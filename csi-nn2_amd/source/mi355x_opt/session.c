/*
 * session.c -- device-resident execution of a whole csinn session.
 *
 * The reference's graph executor keeps every tensor in host memory: csinn_session_run
 * shl_mem_alloc's each intermediate, calls the layer's exec callback on host pointers and frees the
 * tensor when its last consumer has run (source/graph_ref/setup.c:1125-1154, 1256-1450).  Served
 * by this backend's staging path that is one H2D + D2H + synchronisation per LAYER.
 *
 * Here SESSION_SETUP / SESSION_RUN are overridden for sessions whose base_api is CSINN_MI355X:
 *   setup  runs the executor's own setup (node numbering, `init` of every layer -> device plans),
 *          then, if every layer is one this backend executes on the GPU, gives every graph tensor a
 *          fixed HBM buffer, builds "shadow" csinn_tensors pointing at them
 *          (mtype = CSINN_MEM_TYPE_DMABUF) and captures the complete layer sequence into ONE
 *          hipGraph on the session's stream;
 *   run    uploads the graph inputs, replays the hipGraph, downloads the graph outputs and
 *          synchronises once.
 * Sessions containing a layer that falls through to the C reference keep the executor's host path
 * (still correct, per-layer staging).  The graph structures are those of shl_node.h /
 * shl_gref.h (include/shl_gref.h), so the same code walks graphs built by the genuine
 * libshl's gref or by this repository's stand-in.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355x_internal.h"

struct dev_tensor {
    struct shl_node *node;       /* tensor node of the graph */
    void *dev;                   /* HBM buffer */
    size_t bytes;
    struct csinn_tensor shadow;  /* copy of the csinn_tensor with data = dev, mtype = DMABUF */
    int borrowed;                /* dev is the caller's own HBM buffer, bound at run time (rebind) */
    void *probe_ptr;             /* last pointer classified by is_device_ptr, and the verdict */
    int probe_dev;
};

/* one unit the session enqueues: a plain layer through its exec callback, or the layers a rule of the planner's table (rules[],
 * above plan_fusion) merged into one launch.  A relu / relu6 layer folded into the convolution in front of it is no step and no
 * layer of a step: the convolution's step writes the activation's output.  A step carries all its launch needs: enqueue_layers
 * looks up the device buffers of `src` and `out` and calls the rule's launch, nothing is matched again */
#define STEP_LAYERS 5 /* the longest chain: an attention core with its mul and its add */
#define STEP_SOURCES 4
#define FOLD_MAX 4 /* layers of one run of moves around an attention core */
struct rule;

struct step {
    const struct rule *rule; /* NULL: the plain layer layer[0] */
    int layer[STEP_LAYERS], nlayers; /* the layers it stands for, in graph order (an attention step's folded moves are not among them) */
    struct shl_node *out;    /* the tensor node the step finally writes (a split: the first of them) */
    struct shl_node *src[STEP_SOURCES]; /* the tensor nodes the launch reads, NULL from the first unused one on.  [0]: the first
                              * layer's input.  linear: the matmul's second operand, the bias.  residual: the skip tensor.
                              * attention: q, k, v (behind folded moves: the tensors the moves read), the bias or NULL */
    union {
        uint8_t lut[256]; /* table: the activation (and the gate's mul), built from the layers' records */
        int bias_at;      /* linear: which of the add's operands (0 or 1) is the bias */
        struct {
            int skip_at; /* which of the add's operands (0 or 1) is the skip tensor */
            int act;     /* the activation behind the sum: 0 none, 1 relu, 2 relu6 */
        } residual;
        struct {
            struct shl_mi355x_attention_desc ad;
            struct shl_mi355x_attention_bias_desc abd; /* with src[3] */
            struct shl_mi355x_attention_layout_desc ld; /* with a fold: the launch goes through strides */
            int fold[4]; /* the reshape / transpose layers in front of q, k, v and behind the output that the launch stands
                          * for (shl_mi355x_attention_layout); all 0: the dense launch */
        } attention;
    } u;
};

enum { R_ATTENTION, R_LINEAR, R_RESIDUAL, R_POOL_CONV, R_CONV_POOL, R_PAIR, R_TABLE, N_RULES }; /* rules[], in priority order */

struct dev_session {
    struct csinn_session *sess;
    struct dev_tensor *t;
    int nt, cap; /* entries of t in use / allocated */
    void *stream;
    void *prev_stream; /* the session's stream before it became device resident */
    int prev_own;      /* ... and whether that was a stream of its own (else: the process default) */
    void *graph_exec;
    struct step *steps; /* what enqueue_layers runs, in order (plan_fusion); kept for the re-capture after a rebind */
    int nsteps;
    int count[N_RULES];  /* steps of each rule */
    int nfolded;         /* relu / relu6 layers that run in the epilogue of the convolution in front of them */
    int nattention_bias; /* attention steps with the add of a bias or mask */
    int nhead_moves;     /* reshape / transpose layers around attention cores that those launches read and write through strides */
    struct dev_session *next;
};

static struct dev_session *g_sessions;

static struct dev_session *find_session(struct csinn_session *sess)
{
    for (struct dev_session *s = g_sessions; s; s = s->next)
        if (s->sess == sess) return s;
    return NULL;
}

static void free_session(struct dev_session *ds)
{
    if (ds->graph_exec) shl_mi355x_graph_destroy(ds->graph_exec);
    for (int i = 0; i < ds->nt; i++)
        if (ds->t[i].dev && !ds->t[i].borrowed) shl_mi355x_free(ds->t[i].dev);
    if (ds->stream) {
        shl_mi355x_stream_sync(ds->stream);
        /* the host path keeps working: back to the stream the session had -- or to "whatever the process default
         * is" when it had none of its own (a snapshot of the default would stop following shl_mi355x_set_stream) */
        if (ds->prev_own) shl_mi355x_session_set_stream(ds->sess, ds->prev_stream);
        else shl_mi355x_session_inherit_stream(ds->sess);
        shl_mi355x_stream_destroy(ds->stream);
    }
    free(ds->t);
    free(ds->steps);
    free(ds);
}

static void drop_session(struct csinn_session *sess)
{
    struct dev_session **pp = &g_sessions;
    while (*pp) {
        if ((*pp)->sess == sess) {
            struct dev_session *dead = *pp;
            *pp = dead->next;
            free_session(dead);
            return;
        }
        pp = &(*pp)->next;
    }
}

/* the row of layer `n` in the operator table (setup.c); NULL: not a layer this file runs.  A layer qualifies when its op's row
 * has a call shape and its callback is the row's: the one the backend registers, which runs on the GPU and honours DMABUF
 * tensors (a layer that fell through to the reference at init has another) */
static const struct shl_mi355x_op *session_op(struct shl_node *n)
{
    struct csinn_params_base *params = n->data;
    const struct shl_mi355x_op *op = shl_mi355x_op_row(n->type);
    return op && op->call != CALL_NONE && params->cb && (void *)params->cb->exec == op->exec ? op : NULL;
}

/* the number of inputs layer `n` must have; 0: none will do */
static int inputs_of(const struct shl_mi355x_op *op, struct shl_node *n)
{
    if (op->call == CALL_SPLIT) return 1;
    if (op->call != CALL_ARRAY) return op->call;
    struct csinn_concat_params *p = n->data;
    return p->inputs_count >= 1 ? p->inputs_count : 0;
}

/* the number of outputs layer `n` must have; 0: none will do */
static int outputs_of(const struct shl_mi355x_op *op, struct shl_node *n)
{
    if (op->call != CALL_SPLIT) return 1;
    struct csinn_split_params *p = n->data;
    return p->output_num >= 1 ? p->output_num : 0;
}

static struct dev_tensor *lookup(struct dev_session *ds, struct shl_node *node)
{
    for (int i = 0; i < ds->nt; i++)
        if (ds->t[i].node == node) return &ds->t[i];
    return NULL;
}

static struct dev_tensor *adopt(struct dev_session *ds, struct shl_node *node)
{
    struct dev_tensor *d = lookup(ds, node);
    if (d) return d;
    if (ds->nt >= ds->cap) {
        shl_debug_error("mi355x: the session's tensor table is full (%d entries)\n", ds->cap);
        return NULL;
    }
    d = &ds->t[ds->nt++];
    d->node = node;
    struct csinn_tensor *t = node->data;
    d->bytes = (size_t)csinn_tensor_byte_size(t);
    d->dev = shl_mi355x_malloc(d->bytes ? d->bytes : 16);
    d->shadow = *t;
    d->shadow.data = d->dev;
    d->shadow.mtype = CSINN_MEM_TYPE_DMABUF;
    return d->dev ? d : NULL;
}

static int is_dw_op(int type)
{
    return type == CSINN_OP_DEPTHWISE_CONV2D || type == CSINN_OP_DEPTHWISE_CONV2D_RELU ||
           type == CSINN_OP_DEPTHWISE_CONV2D_RELU6;
}

static int is_conv_op(int type)
{
    return type == CSINN_OP_CONV2D || type == CSINN_OP_CONV2D_RELU || type == CSINN_OP_CONV2D_RELU6;
}

static int consumers_of(struct shl_ref_graph *g, struct shl_node *tensor)
{
    int consumers = 0;
    for (int k = 0; k < g->layer_index; k++)
        for (int j = 0; j < g->layer[k]->in_num; j++)
            if (g->layer[k]->in[j] == tensor) consumers++;
    for (int k = 0; k < g->output_num; k++)
        if (g->output[k] == tensor) consumers++;
    return consumers;
}

static int one_record_i8(const struct csinn_tensor *t)
{
    return t->dtype == CSINN_DTYPE_INT8 && t->qinfo != NULL && t->quant_channel <= 1;
}

/* a binary16 tensor as the same-shape add and the relu layers take it: one record, scale 1 */
static int one_record_f16(const struct csinn_tensor *t)
{
    return t->dtype == CSINN_DTYPE_FLOAT16 && t->qinfo != NULL && t->quant_channel <= 1 && t->qinfo->scale == 1.0f;
}

static int same_dims(const struct csinn_tensor *x, const struct csinn_tensor *y)
{
    if (x->dim_count != y->dim_count) return 0;
    for (int i = 0; i < x->dim_count; i++)
        if (x->dim[i] != y->dim[i]) return 0;
    return 1;
}

/* matmul a -> add b, the add's other operand a constant whose only dim that is not 1 is the last and equals N ([N], [1,N],
 * [1,1,N], ...): the index (0 or 1) of that constant among the add's inputs, -1 when the pair does not fuse.  The add must be
 * a broadcasting one that the backend takes (one record per tensor, equal dtypes) and reads `mid` once */
static int linear_bias_input(struct shl_node *a, struct shl_node *b, struct shl_node *mid)
{
    if (a->type != CSINN_OP_MATMUL || b->type != CSINN_OP_ADD || session_op(a) == NULL || session_op(b) == NULL) return -1;
    if (a->in_num != 2 || b->in_num != 2 || (b->in[0] == mid) == (b->in[1] == mid)) return -1;
    const int k = b->in[0] == mid ? 1 : 0;
    struct csinn_tensor *c = b->in[k]->data, *tm = mid->data, *out = b->out[0]->data;
    if (!c->is_const || c->data == NULL || c->dim_count < 1 || tm->dim_count < 2 || !same_dims(out, tm)) return -1;
    const int32_t n = tm->dim[tm->dim_count - 1];
    if (c->dim[c->dim_count - 1] != n || n < 2) return -1;
    for (int i = 0; i < c->dim_count - 1; i++)
        if (c->dim[i] != 1) return -1;
    int64_t rows = 1;
    for (int i = 0; i < tm->dim_count - 1; i++) rows *= tm->dim[i];
    if (rows < 2) return -1; /* (one row: a same-shape add, which has its own kernel) */
    struct csinn_tensor *full, *small;
    struct shl_mi355x_mul_desc d;
    return shl_mi355x_bcast_prepare("add", b->in[0]->data, b->in[1]->data, out, &full, &small, &d) == CSINN_TRUE && small == c ? k : -1;
}

/* layers[0 .. n-1] (consecutive, each still a step of its own): matmul(q, k, trans_b; two activations) -> [mul by a one-element
 * constant, on either side] -> [add of a bias or mask, on either side: a constant or an activation an earlier step wrote, broadcast
 * to the scores] -> softmax over the last axis -> matmul(p, v; v an activation, no transposes), every intermediate
 * read once, by the next layer, and no graph output.  The number of layers the chain takes (3, one more with the mul, one more
 * with the add) and its descriptor in *d; with the add *bias is its other operand's node and *bd the add's part of the
 * descriptor, without it *bias is NULL.  0 when the layers run one by one -- also where the launch has no kernel for the
 * shape or, unless `force`, the shape is none it was measured faster on (shl_mi355x_attention_by_default, with the add
 * shl_mi355x_attention_bias_by_default).  A mul BEHIND the add is no part of the chain */
static int attention_chain(struct shl_ref_graph *g, const int *layers, int n, int force, struct shl_mi355x_attention_desc *d,
                           struct shl_mi355x_attention_bias_desc *bd, struct shl_node **bias, int *k_swapped)
{
    *bias = NULL;
    *k_swapped = 0;
    if (n < 3) return 0;
    struct shl_node *qk = g->layer[layers[0]];
    if (qk->type != CSINN_OP_MATMUL || session_op(qk) == NULL || qk->in_num != 2) return 0;
    struct csinn_tensor *tq = qk->in[0]->data, *tk = qk->in[1]->data;
    if (tq->is_const || tk->is_const || consumers_of(g, qk->out[0]) != 1) return 0;
    struct shl_node *cur = qk->out[0], *cst = NULL, *sc = NULL;
    int at = 1, const_first = 0;
    struct shl_node *mul = g->layer[layers[1]];
    if (mul->type == CSINN_OP_MUL) {
        if (n < 4 || session_op(mul) == NULL || mul->in_num != 2 || (mul->in[0] == cur) == (mul->in[1] == cur)) return 0;
        const_first = mul->in[1] == cur;
        cst = mul->in[const_first ? 0 : 1];
        sc = mul->out[0];
        if (consumers_of(g, sc) != 1) return 0;
        cur = sc;
        at = 2;
    }
    struct shl_node *add = g->layer[layers[at]], *x = cur;
    if (add->type == CSINN_OP_ADD) {
        if (session_op(add) == NULL || add->in_num != 2 || (add->in[0] == cur) == (add->in[1] == cur)) return 0;
        *bias = add->in[add->in[0] == cur ? 1 : 0];
        cur = add->out[0];
        if (consumers_of(g, cur) != 1) return 0;
        at++;
    } else {
        add = NULL;
    }
    if (n < at + 2) return 0;
    struct shl_node *sm = g->layer[layers[at]], *pv = g->layer[layers[at + 1]];
    if (sm->type != CSINN_OP_SOFTMAX || session_op(sm) == NULL || sm->in[0] != cur || consumers_of(g, sm->out[0]) != 1) return 0;
    struct shl_node *p = sm->out[0];
    if (pv->type != CSINN_OP_MATMUL || session_op(pv) == NULL || pv->in_num != 2 || pv->in[0] != p || pv->in[1] == p) return 0;
    struct csinn_tensor *tv = pv->in[1]->data;
    if (tv->is_const) return 0;
    struct csinn_softmax_params *sp = sm->data;
    /* K as ONNX exports it: [.., d, t] into a product without trans_b.  The chain is described as if K were [.., t, d] read with
     * trans_b; the caller takes it only where the moves in front of K fold into strides (head_moves: swap_last2) */
    struct csinn_matmul_params *qp = qk->data, qp_view;
    struct csinn_tensor k_view;
    if (!qp->trans_a && !qp->trans_b && tk->dim_count >= 2 && tk->dim_count <= MAX_DIM) {
        k_view = *tk;
        k_view.dim[tk->dim_count - 2] = tk->dim[tk->dim_count - 1], k_view.dim[tk->dim_count - 1] = tk->dim[tk->dim_count - 2];
        qp_view = *qp;
        qp_view.trans_b = true;
        tk = &k_view, qp = &qp_view;
        *k_swapped = 1;
    }
    if (shl_mi355x_attention_prepare(tq, tk, qk->out[0]->data, qp, cst ? cst->data : NULL, sc ? sc->data : NULL, const_first,
                                     p->data, sp->axis, tv, pv->out[0]->data, pv->data, force || add != NULL, d) != CSINN_TRUE)
        return 0;
    /* (with the add the default is the biased launch's own) */
    if (add != NULL && shl_mi355x_attention_bias_prepare(add->in[0]->data, add->in[1]->data, add->out[0]->data, x->data, d, force, bd) != CSINN_TRUE)
        return 0;
    return at + 2;
}

/* ---- the head split and merge moves around an attention core (shl_mi355x_attention_layout) ------------------------------------- */

/* a reshape or a transpose that this backend runs and that copies its elements unchanged by the movers' own rule: int8 under
 * equal records whose requantisation is the identity on all 256 values (csrc/requant_move.h:move_rec chooses MOVE_RAW where the
 * form may copy, and the other modes give the same bytes then); binary16 at scale 1 on both sides, where the movers change
 * infinities and NaNs only -- the launch applies that rule to an operand whose `moved` bit is set */
static int pure_move(struct shl_node *n)
{
    if ((n->type != CSINN_OP_RESHAPE && n->type != CSINN_OP_TRANSPOSE) || session_op(n) == NULL || n->in_num != 1 || n->out_num != 1) return 0;
    const struct csinn_tensor *in = n->in[0]->data, *out = n->out[0]->data;
    if (in->is_const || in->dtype != out->dtype || in->dim_count < 1 || in->dim_count > MAX_DIM || out->dim_count < 1 || out->dim_count > MAX_DIM)
        return 0;
    if (one_record_f16(in)) return one_record_f16(out);
    if (!one_record_i8(in) || !one_record_i8(out)) return 0;
    const float s = in->qinfo->scale, z = (float)in->qinfo->zero_point;
    if (in->qinfo->zero_point != out->qinfo->zero_point || memcmp(&in->qinfo->scale, &out->qinfo->scale, sizeof(float)) != 0) return 0;
    for (int q = -128; q < 128; q++) { /* (csrc/pool2d.hip:requant_is_identity) */
        const float x = ((float)q - z) * s; /* (this file is compiled without contraction) */
        float r = rintf(x / s) + z;
        r = r > 127.0f ? 127.0f : r;
        r = r < -128.0f ? -128.0f : r;
        if (!(r == r) || (int)r != q) return 0;
    }
    return 1;
}

/* The run of pure moves, with at most one transpose among them, that ends in `x` (out = 0: the layers that make x, each read by
 * exactly one consumer and no graph output) or starts from it (out = 1: the layers that consume x and each other): the longest
 * the strides express.  Returns the run's length, its
 * layers in graph order in `run`, the tensor at its far end in *far (the source the launch reads / the tensor it writes) and
 * the view's heads and strides; 0 when nothing folds.  rows / cols / batches: what the view must come out as; swap: x is
 * [.., cols, rows] (K without trans_b) */
static int head_moves(struct shl_ref_graph *g, struct shl_node *x, int out, int swap, int32_t batches, int32_t rows,
                      int32_t cols, int *run, struct shl_node **far, int32_t *heads, int32_t stride[3])
{
    int seen[FOLD_MAX], n = 0, transposes = 0;
    struct shl_node *cur = x;
    while (n < FOLD_MAX) {
        if (consumers_of(g, cur) != 1) break; /* (a graph output counts as a consumer) */
        int at = -1;
        for (int k = 0; at < 0 && k < g->layer_index; k++) {
            struct shl_node *l = g->layer[k];
            if (out ? (l->in_num >= 1 && l->in[0] == cur) : (l->out_num == 1 && l->out[0] == cur)) at = k;
        }
        if (at < 0 || !pure_move(g->layer[at])) break;
        if (g->layer[at]->type == CSINN_OP_TRANSPOSE && ++transposes > 1) break;
        seen[n++] = at;
        cur = out ? g->layer[at]->out[0] : g->layer[at]->in[0];
    }
    for (int len = n; len >= 1; len--) {
        /* the chain from the far end towards the core: for the output the destination and the layers inverted */
        struct shl_node *end = out ? g->layer[seen[len - 1]]->out[0] : g->layer[seen[len - 1]]->in[0];
        const struct csinn_tensor *te = end->data;
        int32_t is_t[FOLD_MAX], rank[FOLD_MAX], v[FOLD_MAX * MAX_DIM];
        int ok = 1;
        memset(v, 0, sizeof(v));
        for (int i = 0; ok && i < len; i++) {
            struct shl_node *l = g->layer[seen[len - 1 - i]];
            const struct csinn_tensor *to = out ? l->in[0]->data : l->out[0]->data; /* what the step makes */
            is_t[i] = l->type == CSINN_OP_TRANSPOSE;
            rank[i] = to->dim_count;
            if (is_t[i]) {
                const struct csinn_transpose_params *tp = l->data;
                if (tp->permute_num != to->dim_count || tp->permute_num > MAX_DIM) ok = 0;
                for (int k = 0; ok && k < tp->permute_num; k++) {
                    if (tp->permute[k] < 0 || tp->permute[k] >= tp->permute_num) ok = 0;
                    else if (out) v[i * MAX_DIM + tp->permute[k]] = k; /* the inverse permutation */
                    else v[i * MAX_DIM + k] = tp->permute[k];
                }
            } else {
                for (int k = 0; k < to->dim_count; k++) v[i * MAX_DIM + k] = to->dim[k];
            }
        }
        int32_t b, r, c;
        if (ok && !te->is_const &&
            shl_mi355x_attention_layout_strides(te->dim, te->dim_count, len, is_t, rank, v, swap, &b, &r, &c, heads, stride) == SHL_MI355X_OK &&
            b == batches && r == rows && c == cols) {
            for (int i = 0; i < len; i++) run[i] = seen[out ? i : len - 1 - i];
            *far = end;
            return len;
        }
    }
    return 0;
}

/* The layout descriptor of a chain attention_chain has described (layers, len, *d; k_swapped: its K is [.., d, t]): which moves
 * around it fold (the longest runs), the tensors the launch then reads and writes (src[0..2], *dst; the chain's own where a side
 * does not fold) and *ld.  Each side folds or stays on its own; sides whose views split the batch index differently cannot share
 * `heads`, and the later of them stays.  Returns the layers folded */
static int attention_layout(struct shl_ref_graph *g, const int *layers, int len, const struct shl_mi355x_attention_desc *d, int k_swapped,
                            int fold[4], int runs[4][FOLD_MAX], struct shl_node *src[3], struct shl_node **dst,
                            struct shl_mi355x_attention_layout_desc *ld)
{
    struct shl_node *qk = g->layer[layers[0]], *pv = g->layer[layers[len - 1]];
    struct shl_node *x[4] = {qk->in[0], qk->in[1], pv->in[1], pv->out[0]};
    const int32_t rows[4] = {d->s, d->t, d->t, d->s}, cols[4] = {d->d, d->d, d->dv, d->dv};
    int32_t *const st[4] = {ld->q_stride, ld->k_stride, ld->v_stride, ld->out_stride};
    int32_t heads[4];
    int total = 0;
    memset(ld, 0, sizeof(*ld));
    ld->heads = d->batches;
    for (int i = 0; i < 4; i++) {
        struct shl_node *far = x[i];
        fold[i] = head_moves(g, x[i], i == 3, i == 1 && k_swapped, d->batches, rows[i], cols[i], runs[i], &far, &heads[i], st[i]);
        if (fold[i] > 0 && heads[i] != d->batches) { /* two pieces: the split every other side must share */
            if (ld->heads == d->batches) ld->heads = heads[i];
            else if (ld->heads != heads[i]) fold[i] = 0, far = x[i];
        }
        if (fold[i] == 0) heads[i] = d->batches, st[i][0] = 0, st[i][1] = rows[i] * cols[i], st[i][2] = cols[i]; /* dense */
        if (i < 3) src[i] = far;
        else *dst = far;
        total += fold[i];
    }
    /* one piece (heads = batches: the index is bi * head) is two pieces under any split */
    for (int i = 0; i < 4; i++)
        if (heads[i] == d->batches && ld->heads != d->batches) st[i][0] = ld->heads * st[i][1];
    /* (an int8 mover under these records copies bytes; a binary16 one applies its rule for infinities and NaNs) */
    for (int i = 0; i < 4; i++)
        if (fold[i] > 0) ld->moved |= 1 << i;
    return total;
}

/* convolution a (its step writes `mid`, a folded activation included) -> add b: the index (0 or 1) of the add's OTHER operand, the
 * skip tensor, -1 when the pair does not fuse.  The add is the same-shape one -- both operands and the sum int8 tensors of one
 * record, or all three binary16 tensors of scale 1, and equal dims -- and reads `mid` once; the plan must be one the fused launch
 * of its dtype takes (`force`) or was measured faster on (shl_mi355x_conv_add_* / shl_mi355x_conv_add_f16_*) */
static int residual_skip_input(struct shl_node *a, struct shl_node *b, struct shl_node *mid, int force)
{
    if (!is_conv_op(a->type) || b->type != CSINN_OP_ADD || session_op(a) == NULL || session_op(b) == NULL) return -1;
    if (b->in_num != 2 || (b->in[0] == mid) == (b->in[1] == mid)) return -1;
    const int k = b->in[0] == mid ? 1 : 0;
    struct csinn_tensor *tm = mid->data, *ts = b->in[k]->data, *to = b->out[0]->data, *in = a->in[0]->data;
    const int f16 = tm->dtype == CSINN_DTYPE_FLOAT16;
    if (f16 ? !one_record_f16(tm) || !one_record_f16(ts) || !one_record_f16(to) : !one_record_i8(tm) || !one_record_i8(ts) || !one_record_i8(to))
        return -1;
    if (ts->is_const) return -1;
    if (tm->dim_count != 4 || !same_dims(tm, ts) || !same_dims(tm, to)) return -1;
    shl_mi355x_conv_plan *pa = shl_mi355x_registry_get(a->data);
    if (pa == NULL) return -1;
    if (f16) return (force ? shl_mi355x_conv_add_f16_fusable(pa, in->dim[0]) : shl_mi355x_conv_add_f16_by_default(pa, in->dim[0])) ? k : -1;
    return (force ? shl_mi355x_conv_add_fusable(pa, in->dim[0]) : shl_mi355x_conv_add_by_default(pa, in->dim[0])) ? k : -1;
}

/* the relu / relu6 layer `r` behind the sum of a fused residual tail joins it: it reads the sum, nothing else does */
static int residual_takes_relu(struct shl_ref_graph *g, struct shl_node *sum, struct shl_node *r)
{
    if ((r->type != CSINN_OP_RELU && r->type != CSINN_OP_RELU6) || session_op(r) == NULL || r->in[0] != sum) return 0;
    const struct csinn_tensor *ts = sum->data;
    return consumers_of(g, sum) == 1 && (ts->dtype == CSINN_DTYPE_FLOAT16 ? one_record_f16(r->out[0]->data) : one_record_i8(r->out[0]->data));
}

/* steps[0 .. n-1] (consecutive, each still one layer; steps[0] a convolution or a depthwise layer with its folded activation) begin
 * with a table activation folded into the convolution's launch: the number of steps it takes and the table in `lut`; 0: the layers stay apart.
 *   2  convolution -> sigmoid | hard_sigmoid | silu | leaky_relu, which alone reads the convolution's output
 *   3  convolution -> sigmoid | hard_sigmoid -> mul(conv_out, gate), the convolution's output on either side of a same-shape mul
 *      and read by exactly those two layers, the gate read by the mul alone: a swish / hard-swish as converters export it
 * (consumers_of counts a graph output as a reader, so no intermediate tensor is one).  Every tensor is an int8 tensor of one
 * record and the convolution's output dims; the plan must be one the fused launch takes (`force`) or was measured faster on --
 * asked of the entry points of the plan's algorithm, shl_mi355x_conv_lut_* (implicit GEMM) or shl_mi355x_dwconv_lut_* (depthwise) */
static int lut_chain(struct shl_ref_graph *g, const struct step *steps, int n, int force, uint8_t lut[256])
{
    if (n < 2) return 0;
    struct shl_node *a = g->layer[steps[0].layer[0]], *b = g->layer[steps[1].layer[0]], *mid = steps[0].out;
    if (!(is_conv_op(a->type) || is_dw_op(a->type)) || session_op(a) == NULL || session_op(b) == NULL || b->in_num < 1 || b->in[0] != mid) return 0;
    const int gate_kind = b->type == CSINN_OP_SIGMOID || b->type == CSINN_OP_HARD_SIGMOID;
    if (!gate_kind && b->type != CSINN_OP_SILU && b->type != CSINN_OP_LEAKY_RELU) return 0;
    struct csinn_tensor *tm = mid->data, *tb = b->out[0]->data, *in = a->in[0]->data;
    if (!one_record_i8(tm) || !one_record_i8(tb) || tm->dim_count != 4 || !same_dims(tm, tb)) return 0;
    shl_mi355x_conv_plan *pa = shl_mi355x_registry_get(a->data);
    if (pa == NULL) return 0;
    const int dw = shl_mi355x_conv_plan_algo(pa) == SHL_MI355X_ALGO_DW;
    if (!(dw ? (force ? shl_mi355x_dwconv_lut_fusable(pa, in->dim[0]) : shl_mi355x_dwconv_lut_by_default(pa, in->dim[0]))
             : (force ? shl_mi355x_conv_lut_fusable(pa, in->dim[0]) : shl_mi355x_conv_lut_by_default(pa, in->dim[0]))))
        return 0;
    const float si = tm->qinfo->scale, so = tb->qinfo->scale;
    const int32_t zi = tm->qinfo->zero_point, zo = tb->qinfo->zero_point;
    const int readers = consumers_of(g, mid);
    if (readers == 1) {
        if (b->type == CSINN_OP_SIGMOID) shl_mi355x_sigmoid_table_i8(si, zi, so, zo, lut);
        else if (b->type == CSINN_OP_HARD_SIGMOID) shl_mi355x_hard_sigmoid_table_i8(si, zi, so, zo, lut);
        else if (b->type == CSINN_OP_SILU) shl_mi355x_silu_table_i8(si, zi, so, zo, lut);
        else shl_mi355x_leaky_relu_table_i8(si, zi, so, zo, ((struct csinn_relu_params *)b->data)->n, lut);
        return 2;
    }
    if (readers != 2 || !gate_kind || n < 3) return 0;
    struct shl_node *c = g->layer[steps[2].layer[0]], *gate = b->out[0];
    if (c->type != CSINN_OP_MUL || session_op(c) == NULL || c->in_num != 2 || consumers_of(g, gate) != 1) return 0;
    const int x_first = c->in[0] == mid && c->in[1] == gate;
    if (!x_first && !(c->in[0] == gate && c->in[1] == mid)) return 0;
    struct csinn_tensor *tc = c->out[0]->data;
    if (!one_record_i8(tc) || !same_dims(tm, tc)) return 0; /* (the same-shape mul: nothing is broadcast) */
    shl_mi355x_gate_mul_table_i8(b->type == CSINN_OP_HARD_SIGMOID ? SHL_MI355X_UNARY_HARD_SIGMOID : SHL_MI355X_UNARY_SIGMOID, si, zi, so, zo,
                                 x_first, tc->qinfo->scale, tc->qinfo->zero_point, lut);
    return 3;
}

/* layer `n` through its exec callback, writing `out` */
static int run_layer(struct dev_session *ds, struct shl_node *n, struct dev_tensor *out)
{
    struct csinn_params_base *params = n->data;
    int (*f)() = params->cb->exec;
    struct dev_tensor *in = lookup(ds, n->in[0]), *in1;
    switch (session_op(n)->call) {
        case CALL_SISO:
            return f(&in->shadow, &out->shadow, params);
        case CALL_DISO: /* add: the second operand is an activation or a resident constant */
            in1 = lookup(ds, n->in[1]);
            return in1 ? f(&in->shadow, &in1->shadow, &out->shadow, params) : CSINN_FALSE;
        case CALL_CONV:
            return f(&in->shadow, &out->shadow, n->in[1]->data, n->in[2]->data, params);
        case CALL_SPLIT: { /* an array of the outputs' shadow tensors */
            struct csinn_tensor **outs = calloc((size_t)n->out_num, sizeof(*outs));
            int rc = outs ? CSINN_TRUE : CSINN_FALSE;
            for (int j = 0; rc == CSINN_TRUE && j < n->out_num; j++) {
                struct dev_tensor *dj = lookup(ds, n->out[j]);
                if (dj) outs[j] = &dj->shadow;
                else rc = CSINN_FALSE;
            }
            if (rc == CSINN_TRUE) rc = f(&in->shadow, outs, params);
            free(outs);
            return rc;
        }
        default: { /* CALL_ARRAY: an array of shadow tensors */
            struct csinn_tensor **ins = calloc((size_t)n->in_num, sizeof(*ins));
            int rc = ins ? CSINN_TRUE : CSINN_FALSE;
            for (int j = 0; rc == CSINN_TRUE && j < n->in_num; j++) {
                struct dev_tensor *dj = lookup(ds, n->in[j]);
                if (dj) ins[j] = &dj->shadow;
                else rc = CSINN_FALSE;
            }
            if (rc == CSINN_TRUE) rc = f(ins, &out->shadow, params);
            free(ins);
            return rc;
        }
    }
}

static int status_of(int st) { return st == SHL_MI355X_OK ? CSINN_TRUE : CSINN_FALSE; }

/* ---- the planner's rules: what merges into one launch, and the launch ---------------------------------------------------------- */

/* what a rule's match sees.  The switches as levels: 0 off, 1 the shape classes the fused launch was measured faster on, 2 every
 * shape the kernel takes (A/B runs) -- see switch_level */
struct planner {
    struct dev_session *ds;
    struct shl_ref_graph *g;
    struct step *steps; /* from position k on: one step per layer, activations folded */
    int ns;
    int fuse;      /* SHL_MI355X_NO_FUSION is not 1; 0 also zeroes every level below (but not the pair and the pool rules) */
    int attention; /* SHL_MI355X_ATTENTION */
    int layout;    /* SHL_MI355X_ATTENTION_LAYOUT; 0 where no core merges */
    int residual;  /* SHL_MI355X_RESIDUAL */
    int act_fuse;  /* SHL_MI355X_ACT_FUSE */
    char *gone;    /* by layer: a move that an attention step stands for (written by the attention rule) */
};

/* One row per fusion, in priority order: at a position the first rule that matches wins, and the steps it takes are no
 * candidates for a later rule -- a merged step is never the first half of another merge.
 *   match   can steps k, k + 1, ... (each still one layer) run as one launch?  The number of steps taken, with *s -- which
 *           arrives as steps[k] -- filled (take(), src[1..], u); 0 with nothing but s->u touched when they stay apart
 *   launch  enqueues the step: in[i] is the device tensor of s->src[i], out that of s->out */
struct rule {
    const char *name; /* as shl_mi355x_session_describe prints it */
    int (*match)(struct planner *p, int k, struct step *s);
    int (*launch)(struct dev_session *ds, struct shl_ref_graph *g, const struct step *s, struct dev_tensor *const *in, struct dev_tensor *out);
};

/* *s stands for steps k .. k + n - 1 */
static int take(const struct planner *p, int k, int n, struct step *s)
{
    for (int i = 0; i < n; i++) s->layer[i] = p->steps[k + i].layer[0];
    s->nlayers = n;
    s->out = p->steps[k + n - 1].out;
    return n;
}

/* steps k and k + 1 as a candidate pair: the layers and the tensor between them, which has one reader */
static int adjacent(const struct planner *p, int k, struct shl_node **a, struct shl_node **b, struct shl_node **mid)
{
    if (k + 1 >= p->ns) return 0;
    *a = p->g->layer[p->steps[k].layer[0]];
    *b = p->g->layer[p->steps[k + 1].layer[0]];
    *mid = p->steps[k].out;
    return consumers_of(p->g, *mid) == 1;
}

/* attention: matmul(q, k, trans_b) -> [mul by a one-element constant] -> [add of a bias or mask broadcast to the scores] ->
 * softmax over the last axis -> matmul(p, v), every intermediate read by the next layer only (attention_chain): one launch of
 * csrc/attention.hip where both products take matmul's mfma form.  The scores and the probabilities stay in LDS, each computed
 * as its own kernel would store it, so the step equals the layers bit for bit.  First in the table: the core's matmuls then are
 * no candidates for a linear step.  With the layout level on, the reshape / transpose runs around the core fold into the launch
 * as strides (attention_layout), the kernel's own rules having the last word; at level 1 a core the dense default leaves apart
 * is "promoted" when all four sides fold and its class was measured faster.  A K without trans_b merges only when its moves fold.
 * Moves behind the core are marked gone and skipped by the loop; those in front were already emitted and are compacted away */
static int match_attention(struct planner *p, int k, struct step *s)
{
    struct shl_ref_graph *g = p->g;
    struct shl_mi355x_attention_desc *ad = &s->u.attention.ad;
    struct shl_mi355x_attention_bias_desc *abd = &s->u.attention.abd;
    struct shl_mi355x_attention_layout_desc *ld = &s->u.attention.ld;
    struct shl_node *bias = NULL, *src[3], *dst = NULL;
    int chain[STEP_LAYERS], avail = 0, k_swapped = 0, fold4[4] = {0, 0, 0, 0}, runs[4][FOLD_MAX], folded = 0, promoted = 0;
    for (; avail < STEP_LAYERS && k + avail < p->ns; avail++) chain[avail] = p->steps[k + avail].layer[0];
    const int force = p->attention == 2;
    int taken = p->attention ? attention_chain(g, chain, avail, force, ad, abd, &bias, &k_swapped) : 0;
    if (taken == 0 && p->layout == 1 && !force) { /* (with the moves on the scales the dense default's verdict may change) */
        taken = attention_chain(g, chain, avail, 1, ad, abd, &bias, &k_swapped);
        promoted = taken > 0;
    }
    if (taken > 0 && p->layout) {
        folded = attention_layout(g, chain, taken, ad, k_swapped, fold4, runs, src, &dst, ld);
        /* the last word belongs to the kernel's own rules, asked with made-up addresses that do not overlap */
        const void *a0 = (const void *)((uintptr_t)1 << 56), *a1 = (const void *)((uintptr_t)1 << 57), *a2 = (const void *)((uintptr_t)1 << 58),
                   *a3 = (const void *)((uintptr_t)1 << 59), *a4 = bias ? (const void *)((uintptr_t)1 << 60) : NULL;
        const struct shl_mi355x_attention_bias_desc *pb = bias ? abd : NULL;
        if (folded > 0 && shl_mi355x_attention_layout_kernel_name(a0, a1, a2, a4, a3, ad, pb, ld)[0] == '\0') folded = 0;
        if (folded > 0 && p->layout == 1 && !shl_mi355x_attention_layout_by_default(a0, a1, a2, a4, a3, ad, pb, ld)) folded = 0;
        if (promoted && !(fold4[0] && fold4[1] && fold4[2] && fold4[3])) folded = 0;
    }
    if (taken == 0 || ((promoted || k_swapped) && (folded <= 0 || (k_swapped && fold4[1] == 0)))) return 0; /* the layers run one by one */
    struct shl_node *qk = g->layer[chain[0]], *pv = g->layer[chain[taken - 1]];
    take(p, k, taken, s);
    s->src[0] = qk->in[0], s->src[1] = qk->in[1], s->src[2] = pv->in[1], s->src[3] = bias;
    memset(s->u.attention.fold, 0, sizeof(s->u.attention.fold));
    if (folded > 0) { /* through strides: the sources' buffers, the last folded layer's output */
        for (int i = 0; i < 4; i++) {
            s->u.attention.fold[i] = fold4[i];
            for (int j = 0; j < fold4[i]; j++) p->gone[runs[i][j]] = 1;
            if (i < 3) s->src[i] = src[i];
        }
        s->out = dst;
        p->ds->nhead_moves += folded;
    }
    if (bias != NULL) p->ds->nattention_bias++;
    return taken;
}

static int launch_attention(struct dev_session *ds, struct shl_ref_graph *g, const struct step *s, struct dev_tensor *const *in, struct dev_tensor *out)
{
    (void)g;
    const int *fold = s->u.attention.fold;
    const struct shl_mi355x_attention_desc *ad = &s->u.attention.ad;
    const struct shl_mi355x_attention_bias_desc *abd = in[3] ? &s->u.attention.abd : NULL;
    if (fold[0] || fold[1] || fold[2] || fold[3])
        return shl_mi355x_attention_layout_forward(ad, abd, &s->u.attention.ld, in[0]->dev, in[1]->dev, in[2]->dev, in[3] ? in[3]->dev : NULL,
                                                   out->dev, ds->stream);
    if (abd) /* a constant bias is resident like any constant operand of an add */
        return shl_mi355x_attention_bias_forward(ad, abd, in[0]->dev, in[1]->dev, in[2]->dev, in[3]->dev, out->dev, ds->stream);
    return shl_mi355x_attention_forward(ad, in[0]->dev, in[1]->dev, in[2]->dev, out->dev, ds->stream);
}

/* linear: matmul -> add of a constant bias [N], the bias on either side of the add (linear_bias_input): the linear layer a
 * converter exports as MatMul + Add, one launch of csrc/matmul.hip's BIAS instantiation.  The add's arithmetic runs on the value
 * the matmul would have stored, so the step equals the two layers bit for bit.  It has no switch of its own:
 * SHL_MI355X_NO_FUSION=1 keeps the two apart (the linear fusion's A/B runs) */
static int match_linear(struct planner *p, int k, struct step *s)
{
    struct shl_node *a, *b, *mid;
    if (!p->fuse || !adjacent(p, k, &a, &b, &mid)) return 0;
    const int kb = linear_bias_input(a, b, mid);
    if (kb < 0) return 0;
    s->u.bias_at = kb;
    s->src[1] = a->in[1], s->src[2] = b->in[kb];
    return take(p, k, 2, s);
}

static int launch_linear(struct dev_session *ds, struct shl_ref_graph *g, const struct step *s, struct dev_tensor *const *in, struct dev_tensor *out)
{
    struct shl_node *n = g->layer[s->layer[0]], *nx = g->layer[s->layer[1]];
    return shl_mi355x_matmul_bias_forward(n->in[0]->data, n->in[1]->data, n->out[0]->data, s->src[2]->data, nx->out[0]->data, n->data,
                                          s->u.bias_at == 0, in[0]->dev, in[1]->dev, in[2]->dev, out->dev, ds->stream);
}

/* residual: convolution (implicit GEMM, int8 or binary16 NHWC; its folded activation included) -> add(conv_out, skip) of equal
 * shapes, the convolution's output on either side (residual_skip_input) -> [relu | relu6, taken only when the sum has that one
 * reader]: the tail of a skip connection as one launch of the convolution (csrc/conv_igemm.hip's instantiations with the
 * post-op).  The add's and the activation's element functions run on the value the convolution would have stored, so the step
 * equals the layers bit for bit.  Level 1: csrc/residual_validate.h:residual_default */
static int match_residual(struct planner *p, int k, struct step *s)
{
    struct shl_node *a, *b, *mid;
    if (!p->residual || !adjacent(p, k, &a, &b, &mid)) return 0;
    const int ks = residual_skip_input(a, b, mid, p->residual == 2);
    if (ks < 0) return 0;
    struct shl_node *r = k + 2 < p->ns ? p->g->layer[p->steps[k + 2].layer[0]] : NULL;
    const int relu = r != NULL && residual_takes_relu(p->g, p->steps[k + 1].out, r);
    s->u.residual.skip_at = ks;
    s->u.residual.act = relu ? (r->type == CSINN_OP_RELU6 ? 2 : 1) : 0;
    s->src[1] = b->in[ks];
    return take(p, k, relu ? 3 : 2, s);
}

/* the add and the activation read what the convolution (+ folded activation) would have written */
static int launch_residual(struct dev_session *ds, struct shl_ref_graph *g, const struct step *s, struct dev_tensor *const *in, struct dev_tensor *out)
{
    struct shl_node *n = g->layer[s->layer[0]], *add = g->layer[s->layer[1]];
    struct csinn_tensor *tskip = s->src[1]->data, *tsum = add->out[0]->data, *tout = s->out->data;
    struct shl_mi355x_residual_desc rd = {s->u.residual.skip_at == 1, tskip->qinfo->scale, tskip->qinfo->zero_point, tsum->qinfo->scale,
                                          tsum->qinfo->zero_point, s->u.residual.act, tout->qinfo->scale, tout->qinfo->zero_point};
    /* (the plan's dtype is the sum's: binary16 has entry points of its own, which read conv_first and act alone) */
    int (*const forward)(const shl_mi355x_conv_plan *, const void *, const void *, void *, int32_t, const struct shl_mi355x_residual_desc *, void *) =
        tsum->dtype == CSINN_DTYPE_FLOAT16 ? shl_mi355x_conv_add_f16_forward : shl_mi355x_conv_add_forward;
    return status_of(forward(shl_mi355x_registry_get(n->data), in[0]->dev, in[1]->dev, out->dev, in[0]->shadow.dim[0], &rd, ds->stream));
}

/* pool_conv: global_avgpool2d -> the convolution / fullyconnected layer on the pooled map: one launch (csrc/conv_gemv.hip) */
static int match_pool_conv(struct planner *p, int k, struct step *s)
{
    struct shl_node *a, *b, *mid;
    if (!adjacent(p, k, &a, &b, &mid) || b->in[0] != mid) return 0;
    if (a->type != CSINN_OP_GLOBAL_AVGPOOL2D || !(is_conv_op(b->type) || b->type == CSINN_OP_FULLYCONNECTED)) return 0;
    struct csinn_tensor *pin = a->in[0]->data, *pmid = mid->data;
    struct csinn_pool_params *pp = a->data;
    shl_mi355x_conv_plan *pb = shl_mi355x_registry_get(b->data);
    if (!(pb && pp->base.layout == CSINN_LAYOUT_NHWC && pin->dim_count == 4 && pin->dtype == CSINN_DTYPE_INT8 && pin->qinfo && pmid->qinfo &&
          pin->quant_channel <= 1 && pmid->quant_channel <= 1 && shl_mi355x_pool_conv_fusable(pb, pin->dim[0], pin->dim[1] * pin->dim[2])))
        return 0;
    return take(p, k, 2, s);
}

static int launch_pool_conv(struct dev_session *ds, struct shl_ref_graph *g, const struct step *s, struct dev_tensor *const *in, struct dev_tensor *out)
{
    struct shl_node *n = g->layer[s->layer[0]], *nx = g->layer[s->layer[1]];
    struct csinn_tensor *pin = n->in[0]->data, *pmid = n->out[0]->data;
    return status_of(shl_mi355x_pool_conv_forward(shl_mi355x_registry_get(nx->data), in[0]->dev, out->dev, in[0]->shadow.dim[0],
                                                  pin->dim[1] * pin->dim[2], pin->qinfo->scale, pin->qinfo->zero_point, pmid->qinfo->scale,
                                                  pmid->qinfo->zero_point, ds->stream));
}

/* conv_pool: 1x1 convolution -> global_avgpool2d, the pooled tensor being all anything reads of it: one launch
 * (csrc/conv1x1_latency.hip: the workgroup of a channel slice holds the whole map) */
static int match_conv_pool(struct planner *p, int k, struct step *s)
{
    struct shl_node *a, *b, *mid;
    if (!adjacent(p, k, &a, &b, &mid) || b->in[0] != mid || !is_conv_op(a->type) || b->type != CSINN_OP_GLOBAL_AVGPOOL2D) return 0;
    struct csinn_tensor *cin = a->in[0]->data, *pmid = mid->data, *pout = b->out[0]->data;
    struct csinn_pool_params *pp = b->data;
    shl_mi355x_conv_plan *pa = shl_mi355x_registry_get(a->data);
    if (!(pa && pp->base.layout == CSINN_LAYOUT_NHWC && pmid->dim_count == 4 && pmid->dtype == CSINN_DTYPE_INT8 && pmid->qinfo && pout->qinfo &&
          pmid->quant_channel <= 1 && pout->quant_channel <= 1 && shl_mi355x_conv_pool_fusable(pa, cin->dim[0])))
        return 0;
    return take(p, k, 2, s);
}

/* the pool reads what the convolution (+ folded activation) would have written */
static int launch_conv_pool(struct dev_session *ds, struct shl_ref_graph *g, const struct step *s, struct dev_tensor *const *in, struct dev_tensor *out)
{
    struct shl_node *n = g->layer[s->layer[0]], *nx = g->layer[s->layer[1]];
    struct csinn_tensor *pmid = nx->in[0]->data, *pout = nx->out[0]->data;
    return status_of(shl_mi355x_conv_pool_forward(shl_mi355x_registry_get(n->data), in[0]->dev, NULL, out->dev, in[0]->shadow.dim[0],
                                                  pmid->qinfo->scale, pmid->qinfo->zero_point, pout->qinfo->scale, pout->qinfo->zero_point,
                                                  ds->stream));
}

/* pair: pointwise -> depthwise 3x3 (latency form, small batches: csrc/pwdw_fused.hip, pwdw_f16_nchw.hip) or depthwise 3x3 ->
 * pointwise (bandwidth form at throughput batches, csrc/dwpw_stream.hip: the requantised depthwise tile is the pointwise MFMA
 * operand; the latency form of this order is parked, attic/README.md); shl_mi355x_pwdw_fusable tells the orders apart by the plans */
static int match_pair(struct planner *p, int k, struct step *s)
{
    struct shl_node *a, *b, *mid;
    if (!adjacent(p, k, &a, &b, &mid) || b->in[0] != mid) return 0;
    if (!((is_conv_op(a->type) && is_dw_op(b->type)) || (is_dw_op(a->type) && is_conv_op(b->type)))) return 0;
    shl_mi355x_conv_plan *pa = shl_mi355x_registry_get(a->data), *pb = shl_mi355x_registry_get(b->data);
    struct csinn_tensor *in = a->in[0]->data;
    return pa && pb && shl_mi355x_pwdw_fusable(pa, pb, in->dim[0]) ? take(p, k, 2, s) : 0;
}

static int launch_pair(struct dev_session *ds, struct shl_ref_graph *g, const struct step *s, struct dev_tensor *const *in, struct dev_tensor *out)
{
    return status_of(shl_mi355x_pwdw_forward(shl_mi355x_registry_get(g->layer[s->layer[0]]->data), shl_mi355x_registry_get(g->layer[s->layer[1]]->data),
                                             in[0]->dev, out->dev, in[0]->shadow.dim[0], ds->stream));
}

/* table: convolution or depthwise layer (int8 NHWC; its folded activation included) -> sigmoid | hard_sigmoid | silu |
 * leaky_relu, or -> sigmoid | hard_sigmoid -> mul(conv_out, gate), a swish / hard-swish gate (lut_chain): one launch of the
 * convolution with the table post-op (csrc/conv_igemm.hip; depthwise: csrc/dwconv.hip, csrc/dwconv_mfma.hip -- MobileNetV3's
 * depthwise -> hard-swish, EfficientNet's depthwise -> swish).  On int8 the layers are a function of the byte the convolution
 * would have stored, ONE 256-entry table built from their records with the layers' own builders, so the step equals the layers
 * bit for bit.  Last in the table: a convolution that is half of a pair, feeds a pool or a residual tail is not taken, and the
 * step is not the first half of a residual merge.  Level 1: csrc/lut_validate.h:lut_default, dw_lut_default */
static int match_table(struct planner *p, int k, struct step *s)
{
    const int n = p->act_fuse ? lut_chain(p->g, &p->steps[k], p->ns - k, p->act_fuse == 2, s->u.lut) : 0;
    return n > 0 ? take(p, k, n, s) : 0;
}

/* the table's input is what the convolution (+ folded activation) would have written */
static int launch_table(struct dev_session *ds, struct shl_ref_graph *g, const struct step *s, struct dev_tensor *const *in, struct dev_tensor *out)
{
    shl_mi355x_conv_plan *plan = shl_mi355x_registry_get(g->layer[s->layer[0]]->data);
    return status_of(shl_mi355x_conv_plan_algo(plan) == SHL_MI355X_ALGO_DW
                         ? shl_mi355x_dwconv_lut_forward(plan, in[0]->dev, out->dev, in[0]->shadow.dim[0], s->u.lut, ds->stream)
                         : shl_mi355x_conv_lut_forward(plan, in[0]->dev, out->dev, in[0]->shadow.dim[0], s->u.lut, ds->stream));
}

static const struct rule rules[N_RULES] = {
    [R_ATTENTION] = {"attention", match_attention, launch_attention},
    [R_LINEAR] = {"linear", match_linear, launch_linear},
    [R_RESIDUAL] = {"residual", match_residual, launch_residual},
    [R_POOL_CONV] = {"pool_conv", match_pool_conv, launch_pool_conv},
    [R_CONV_POOL] = {"conv_pool", match_conv_pool, launch_conv_pool},
    [R_PAIR] = {"pair", match_pair, launch_pair},
    [R_TABLE] = {"table", match_table, launch_table},
};

/* a planner switch, read at plan time: 0 for "0", 2 for "1", 1 when unset (or anything else) */
static int switch_level(const char *name)
{
    const char *v = getenv(name);
    return v && v[0] == '0' ? 0 : v && v[0] == '1' ? 2 : 1;
}

/* Graph-level rewrites; the intermediate tensors then never exist in HBM.  Three passes:
 *   1  conv / depthwise / deconv2d (no activation) -> relu | relu6, the convolution's only consumer, same output record: the
 *      activation moves into the convolution's epilogue (the relu layer gets no step, the convolution's step writes the relu's
 *      output).  What a converter emits for a RISC-V target -- example/c906_mobilenetv1_f16.c is 28 csinn_conv2d + 27
 *      csinn_relu -- runs as 28 launches, not 55
 *   2  depthwise plans learn whether the bandwidth pair takes their consumer
 *   3  rules[], greedily from the front
 * Fills ds->steps. */
static int plan_fusion(struct dev_session *ds, struct shl_ref_graph *g)
{
    struct step *steps = ds->steps = calloc((size_t)g->layer_index, sizeof(*steps));
    struct planner p = {.ds = ds, .g = g, .steps = steps, .gone = calloc((size_t)g->layer_index + 1, 1)};
    if (steps == NULL || p.gone == NULL) {
        free(p.gone);
        return 0;
    }
    p.fuse = switch_level("SHL_MI355X_NO_FUSION") != 2;
    p.attention = p.fuse ? switch_level("SHL_MI355X_ATTENTION") : 0;
    p.layout = p.attention ? switch_level("SHL_MI355X_ATTENTION_LAYOUT") : 0;
    p.residual = p.fuse ? switch_level("SHL_MI355X_RESIDUAL") : 0;
    p.act_fuse = p.fuse ? switch_level("SHL_MI355X_ACT_FUSE") : 0;
    /* one step per layer; an activation that folds joins the convolution's step */
    for (int i = 0; i < g->layer_index; i++) {
        struct shl_node *a = g->layer[i], *b = i + 1 < g->layer_index ? g->layer[i + 1] : NULL;
        struct step *s = &steps[p.ns++];
        *s = (struct step){.layer = {i}, .nlayers = 1, .out = a->out[0], .src = {a->in[0]}};
        const int plain = a->type == CSINN_OP_CONV2D || a->type == CSINN_OP_DEPTHWISE_CONV2D;
        const int deconv = a->type == CSINN_OP_DECONV2D || a->type == CSINN_OP_DEPTHWISE_DECONV2D;
        if (!p.fuse || !(plain || deconv) || b == NULL || (b->type != CSINN_OP_RELU && b->type != CSINN_OP_RELU6)) continue;
        if (b->in[0] != a->out[0] || consumers_of(g, a->out[0]) != 1) continue;
        int (*const fold_activation)(struct csinn_tensor *, struct csinn_tensor *, struct csinn_tensor *, struct csinn_tensor *,
                                     struct csinn_tensor *, struct csinn_conv2d_params *, int) =
            deconv ? shl_mi355x_deconv2d_fold_activation : shl_mi355x_conv2d_fold_activation;
        if (fold_activation(a->in[0]->data, a->out[0]->data, b->out[0]->data, a->in[1]->data, a->in[2]->data, a->data,
                            b->type == CSINN_OP_RELU6) == CSINN_TRUE) {
            s->out = b->out[0];
            ds->nfolded++;
            i++; /* the activation layer is taken */
        }
    }
    /* a depthwise layer whose output does not feed ONE pointwise layer that the bandwidth form takes keeps its latency pair
     * (the pair rule cannot see a layer's consumer: ADVICE r05 -- dw 32 -> pw 16 of MobileNetV2, two consumers, ...) */
    for (int k = 0; k < p.ns; k++) {
        struct shl_node *a = g->layer[steps[k].layer[0]], *b = k + 1 < p.ns ? g->layer[steps[k + 1].layer[0]] : NULL;
        if (!is_dw_op(a->type)) continue;
        shl_mi355x_conv_plan *pa = shl_mi355x_registry_get(a->data);
        if (pa == NULL) continue;
        struct csinn_tensor *in = a->in[0]->data;
        int streams = 0;
        if (b && b->in[0] == steps[k].out && is_conv_op(b->type) && consumers_of(g, steps[k].out) == 1) {
            shl_mi355x_conv_plan *pb = shl_mi355x_registry_get(b->data);
            streams = pb != NULL && shl_mi355x_pwdw_fusable(pa, pb, in->dim[0]);
        }
        shl_mi355x_conv_plan_set_no_stream_consumer(pa, !streams);
    }
    /* the merged steps overwrite the list in place: position nsteps never runs ahead of k */
    for (int k = 0; k < p.ns; k++) {
        struct step s = steps[k];
        if (p.gone[s.layer[0]]) continue; /* a move behind a core that took it */
        int taken = 0;
        for (int r = 0; r < N_RULES && taken == 0; r++)
            if ((taken = rules[r].match(&p, k, &s)) > 0) {
                s.rule = &rules[r];
                ds->count[r]++;
                k += taken - 1;
            }
        steps[ds->nsteps++] = s;
    }
    /* the moves in FRONT of a core were steps before the core was found: compact.  (This relies on a reshape or a transpose
     * never being part of a merged step -- no rule takes one --: a folded move inside a merged step would still run, and
     * nhead_moves would count a layer that did) */
    int kept = 0;
    for (int k = 0; k < ds->nsteps; k++)
        if (!(steps[k].rule == NULL && p.gone[steps[k].layer[0]])) steps[kept++] = steps[k];
    ds->nsteps = kept;
    free(p.gone);
    return 1;
}

/* enqueue every step on the session stream, tensors resident in HBM */
static int enqueue_layers(struct dev_session *ds, struct shl_ref_graph *g)
{
    for (int k = 0; k < ds->nsteps; k++) {
        const struct step *s = &ds->steps[k];
        struct shl_node *n = g->layer[s->layer[0]];
        struct dev_tensor *in[STEP_SOURCES], *out = lookup(ds, s->out);
        int rc = out ? CSINN_TRUE : CSINN_FALSE;
        for (int i = 0; i < STEP_SOURCES; i++) {
            in[i] = s->src[i] ? lookup(ds, s->src[i]) : NULL;
            if (s->src[i] && in[i] == NULL) rc = CSINN_FALSE;
        }
        if (rc == CSINN_TRUE) rc = s->rule ? s->rule->launch(ds, g, s, in, out) : run_layer(ds, n, out);
        if (rc != CSINN_TRUE) {
            shl_debug_error("mi355x: layer %d (%s) failed while building the device graph\n", s->layer[0], n->name ? n->name : "?");
            return CSINN_FALSE;
        }
    }
    return CSINN_TRUE;
}

static int capture(struct dev_session *ds, struct shl_ref_graph *g)
{
    if (ds->graph_exec) {
        shl_mi355x_graph_destroy(ds->graph_exec);
        ds->graph_exec = NULL;
    }
    /* the layers' exec callbacks enqueue on the session's own stream (its context, setup.c) */
    int built = CSINN_FALSE;
    if (shl_mi355x_graph_begin(ds->stream) == SHL_MI355X_OK) {
        built = enqueue_layers(ds, g);
        ds->graph_exec = shl_mi355x_graph_end(ds->stream);
        if (built != CSINN_TRUE && ds->graph_exec) {
            shl_mi355x_graph_destroy(ds->graph_exec);
            ds->graph_exec = NULL;
        }
    }
    return built;
}

/* does the caller's buffer live in HBM?  (graph tensors carry node pointers in `data` while the
 * graph is built -- graph_ref/setup.c:75-268 -- so device residency of inputs / outputs can only be
 * seen on the pointers handed over by csinn_update_input / csinn_update_output) */
static int caller_buffer_is_device(struct dev_tensor *d, struct csinn_tensor *t)
{
    if (t->data == NULL) return 0;
    if (t->mtype == CSINN_MEM_TYPE_DMABUF) return 1;
    if (d->probe_ptr != t->data) {
        d->probe_ptr = t->data;
        d->probe_dev = shl_mi355x_is_device_ptr(t->data);
    }
    return d->probe_dev;
}

/* run in place on the caller's HBM buffer from now on; the captured graph must be rebuilt */
static void rebind(struct dev_tensor *d, void *dev)
{
    if (d->dev && !d->borrowed) shl_mi355x_free(d->dev);
    d->dev = dev;
    d->borrowed = 1;
    d->shadow.data = dev;
}

/* back to a buffer of our own (the caller switched from an HBM buffer to host memory: the borrowed
 * one may be gone, nothing may be copied into it) */
static int unbind(struct dev_tensor *d)
{
    d->dev = shl_mi355x_malloc(d->bytes ? d->bytes : 16);
    d->borrowed = 0;
    d->shadow.data = d->dev;
    return d->dev != NULL;
}

int shl_mi355x_session_setup(struct csinn_session *sess)
{
    /* the reference's shl_gref_session_setup returns void (source/graph_ref/setup.c:688): its
     * "status" is whatever the register holds, so it cannot gate anything here */
    int (*gref_setup)(struct csinn_session *) = shl_gref_runtime_callback(CSINN_SESSION_SETUP);
    if (gref_setup == NULL) return CSINN_FALSE;
    int rc = gref_setup(sess);
    drop_session(sess);
    struct shl_ref_graph *g = shl_gref_get_graph(sess);
    if (g == NULL || g->layer_index == 0) return rc;
    /* SHL_MI355X_HOST_SESSION=1: keep the executor's host path (every layer staged and traced on its own) */
    const char *host_only = getenv("SHL_MI355X_HOST_SESSION");
    if (host_only && host_only[0] == '1') return rc;

    /* device-resident only when every layer runs on the GPU */
    int tensors = g->input_num;
    for (int i = 0; i < g->layer_index; i++) {
        struct shl_node *n = g->layer[i];
        const struct shl_mi355x_op *op = session_op(n);
        const int inputs = op ? inputs_of(op, n) : 0, outputs = op ? outputs_of(op, n) : 0;
        if (inputs == 0 || n->in_num != inputs || outputs == 0 || n->out_num != outputs) {
            shl_debug_info("mi355x: layer %d (%s, op %d) runs on the host path: session stays host-staged\n", i,
                           n->name ? n->name : "?", n->type);
            return rc;
        }
        tensors += outputs + (op->activations ? op->activations : inputs) - op->first_const; /* its outputs + constants it may bring */
    }
    struct dev_session *ds = calloc(1, sizeof(*ds));
    ds->sess = sess;
    ds->t = calloc((size_t)tensors, sizeof(struct dev_tensor));
    ds->cap = ds->t ? tensors : 0;
    ds->stream = shl_mi355x_stream_create();
    int ok = ds->stream != NULL;
    ds->prev_own = shl_mi355x_session_has_own_stream(sess);
    ds->prev_stream = shl_mi355x_session_stream(sess);
    if (ok) shl_mi355x_session_set_stream(sess, ds->stream); /* every exec callback of this session enqueues here */
    for (int i = 0; ok && i < g->input_num; i++) ok = adopt(ds, g->input[i]) != NULL;
    for (int i = 0; ok && i < g->layer_index; i++) {
        struct shl_node *n = g->layer[i];
        const struct shl_mi355x_op *op = session_op(n);
        const int activations = op->activations ? op->activations : n->in_num;
        for (int j = 0; ok && j < activations; j++) {
            if (lookup(ds, n->in[j]) != NULL) continue;
            /* a constant operand: upload it once, keep it resident */
            struct csinn_tensor *c = n->in[j]->data;
            struct dev_tensor *d = j >= op->first_const && c->is_const && c->data ? adopt(ds, n->in[j]) : NULL;
            if (d == NULL || shl_mi355x_upload(d->dev, c->data, d->bytes, ds->stream) != SHL_MI355X_OK) {
                if (j == 0) shl_debug_error("mi355x: layer %d consumes a tensor that no earlier layer produces\n", i);
                else shl_debug_error("mi355x: layer %d: operand %d is neither produced earlier nor constant\n", i, j);
                ok = 0;
            }
        }
        if (!ok) break;
        for (int j = 0; ok && j < n->out_num; j++) ok = adopt(ds, n->out[j]) != NULL;
    }
    for (int i = 0; ok && i < g->output_num; i++) ok = lookup(ds, g->output[i]) != NULL;
    if (ok) ok = plan_fusion(ds, g);
    if (ok) ok = capture(ds, g) == CSINN_TRUE; /* the whole model as one hipGraph */
    if (!ok) {
        shl_debug_error("mi355x: device-resident session setup failed (%s); keeping the host path\n",
                        shl_mi355x_last_error());
        free_session(ds);
        return rc;
    }
    ds->next = g_sessions;
    g_sessions = ds;
    return CSINN_TRUE;
}

int shl_mi355x_session_run(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    if (ds == NULL) {
        int (*gref_run)(struct csinn_session *) = shl_gref_runtime_callback(CSINN_SESSION_RUN);
        return gref_run ? gref_run(sess) : CSINN_FALSE;
    }
    struct shl_ref_graph *g = shl_gref_get_graph(sess);
    int status = CSINN_TRUE, host_outputs = 0, stale = 0;
    /* inputs / outputs the caller keeps in HBM are used in place (first sight of a new pointer
     * re-captures the graph once); host buffers are copied */
    for (int i = 0; i < g->input_num; i++) {
        struct dev_tensor *d = lookup(ds, g->input[i]);
        struct csinn_tensor *t = g->input[i]->data;
        if (t->data == NULL) {
            shl_debug_error("mi355x: graph input %d has no data\n", i);
            return CSINN_FALSE;
        }
        const int on_dev = caller_buffer_is_device(d, t);
        if (on_dev && t->data != d->dev) {
            rebind(d, t->data);
            stale = 1;
        } else if (!on_dev && d->borrowed) {
            if (!unbind(d)) return CSINN_FALSE;
            stale = 1;
        }
    }
    for (int i = 0; i < g->output_num; i++) {
        struct dev_tensor *d = lookup(ds, g->output[i]);
        struct csinn_tensor *t = g->output[i]->data;
        const int on_dev = t->mtype == CSINN_MEM_TYPE_CPU_ACC && caller_buffer_is_device(d, t);
        if (on_dev && t->data != d->dev) {
            rebind(d, t->data);
            stale = 1;
        } else if (!on_dev && d->borrowed) {
            if (!unbind(d)) return CSINN_FALSE;
            stale = 1;
        }
    }
    if (stale && capture(ds, g) != CSINN_TRUE) return CSINN_FALSE;
    for (int i = 0; i < g->input_num; i++) {
        struct dev_tensor *d = lookup(ds, g->input[i]);
        struct csinn_tensor *t = g->input[i]->data;
        if (t->data != d->dev && shl_mi355x_upload(d->dev, t->data, d->bytes, ds->stream) != SHL_MI355X_OK)
            status = CSINN_FALSE;
    }
    if (ds->graph_exec) {
        if (shl_mi355x_graph_launch(ds->graph_exec, ds->stream) != SHL_MI355X_OK) status = CSINN_FALSE;
    } else {
        if (enqueue_layers(ds, g) != CSINN_TRUE) status = CSINN_FALSE;
    }
    for (int i = 0; i < g->output_num; i++) {
        struct dev_tensor *d = lookup(ds, g->output[i]);
        struct csinn_tensor *t = g->output[i]->data;
        if (t->mtype == CSINN_MEM_TYPE_CPU_ACC && t->data == d->dev) continue; /* written in place, in HBM */
        if (t->mtype != CSINN_MEM_TYPE_CPU_ACC) /* a fresh buffer per run that the caller then owns, as
                                                   the executor does (graph_ref/setup.c:1125-1134) */
            t->data = shl_mem_alloc((int64_t)(d->bytes ? d->bytes : 16));
        host_outputs++;
        if (t->data == NULL || shl_mi355x_download(t->data, d->dev, d->bytes, ds->stream) != SHL_MI355X_OK)
            status = CSINN_FALSE;
    }
    /* outputs that stay in HBM stay asynchronous (shl_mi355x_session_stream + stream_sync to wait) */
    if (host_outputs > 0 && shl_mi355x_stream_sync(ds->stream) != SHL_MI355X_OK) status = CSINN_FALSE;
    if (status != CSINN_TRUE) shl_debug_error("mi355x: device session run failed: %s\n", shl_mi355x_last_error());
    return status;
}

void shl_mi355x_session_deinit(struct csinn_session *sess)
{
    drop_session(sess);
    /* the device plans of the session's layers and its staging buffers die with it (the reference's
     * optimised backends leak theirs: "XXX: memory leak", thead_rvv/int8/convolution.c:177) */
    struct shl_ref_graph *g = shl_gref_get_graph(sess);
    if (g)
        for (int i = 0; i < g->layer_index; i++)
            if (g->layer[i] && g->layer[i]->data) shl_mi355x_release_params(g->layer[i]->data);
    shl_mi355x_ctx_release(sess);
    void (*gref_deinit)(struct csinn_session *) = shl_gref_runtime_callback(CSINN_SESSION_DEINIT);
    if (gref_deinit) gref_deinit(sess);
}

/* the planner's counters: how many steps of each rule `sess` has, and what else its plan folded */
static int steps_of(struct csinn_session *sess, int rule)
{
    struct dev_session *ds = find_session(sess);
    return ds ? ds->count[rule] : 0;
}

/* global_avgpool2d layers that run inside the launch of the layer in front of or behind them */
int shl_mi355x_session_fused_pools(struct csinn_session *sess) { return steps_of(sess, R_POOL_CONV) + steps_of(sess, R_CONV_POOL); }
/* depthwise + pointwise pairs that run as one launch */
int shl_mi355x_session_fused_pairs(struct csinn_session *sess) { return steps_of(sess, R_PAIR); }
/* matmul layers that add the constant bias behind them inside their own launch */
int shl_mi355x_session_fused_linears(struct csinn_session *sess) { return steps_of(sess, R_LINEAR); }
/* Q K^T -> [scale] -> [+ bias] -> softmax -> P V chains that run as one launch */
int shl_mi355x_session_fused_attentions(struct csinn_session *sess) { return steps_of(sess, R_ATTENTION); }
/* convolution -> add -> [relu | relu6] tails of skip connections that run as one launch */
int shl_mi355x_session_fused_residuals(struct csinn_session *sess) { return steps_of(sess, R_RESIDUAL); }
/* table activations (gates included) that run inside their convolution's launch */
int shl_mi355x_session_fused_activations(struct csinn_session *sess) { return steps_of(sess, R_TABLE); }

/* relu / relu6 layers that run inside the epilogue of the convolution in front of them */
int shl_mi355x_session_folded_activations(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? ds->nfolded : 0;
}

/* how many of the attention steps carry the add of a bias or mask (shl_mi355x_attention_bias) */
int shl_mi355x_session_fused_attention_biases(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? ds->nattention_bias : 0;
}

/* how many reshape / transpose layers around attention cores run inside their launches (shl_mi355x_attention_layout) */
int shl_mi355x_session_folded_head_moves(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? ds->nhead_moves : 0;
}

/* 2 when `sess` executes as one device-resident hipGraph, 1 when device-resident with every run enqueueing its layers
 * anew (no graph could be captured), 0 when host-staged */
int shl_mi355x_session_is_device_resident(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? (ds->graph_exec ? 2 : 1) : 0;
}

/* the plan of `sess` as text: one line per step, then the folded-activation count */
int shl_mi355x_session_describe(struct csinn_session *sess, char *buf, int len)
{
    struct dev_session *ds = find_session(sess);
    int at = 0;
    if (ds == NULL) return 0;
#define PUT(...) at += snprintf(at < len ? buf + at : NULL, at < len ? (size_t)(len - at) : 0, __VA_ARGS__)
    for (int k = 0; k < ds->nsteps; k++) {
        const struct step *s = &ds->steps[k];
        PUT("%s", s->rule ? s->rule->name : "layer");
        for (int i = 0; i < s->nlayers; i++) PUT("%c%d", i ? ',' : ' ', s->layer[i]);
        PUT(" -> %s", s->out->name ? s->out->name : "?");
        if (s->rule == &rules[R_ATTENTION]) {
            const int *fold = s->u.attention.fold;
            PUT(" fold %d,%d,%d,%d bias %d", fold[0], fold[1], fold[2], fold[3], s->src[3] != NULL);
        }
        PUT("\n");
    }
    PUT("folded %d\n", ds->nfolded);
#undef PUT
    return at + 1;
}

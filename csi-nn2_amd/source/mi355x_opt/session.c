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

/* one unit the session enqueues: a layer, or two layers (an attention core: three to five) that run as one launch.  A relu / relu6 layer folded into the
 * convolution in front of it is no step and no layer of a step: the convolution's step writes the activation's output */
enum step_kind {
    STEP_LAYER,     /* layer a, through its exec callback */
    STEP_PWDW,      /* a pointwise and a depthwise layer, in either order (shl_mi355x_pwdw_forward) */
    STEP_POOL_CONV, /* global_avgpool2d a + the convolution / fullyconnected layer b on the pooled map */
    STEP_CONV_POOL, /* 1x1 convolution a + global_avgpool2d b */
    STEP_MATMUL_BIAS, /* matmul a + the add b of a constant bias [N] to its output (shl_mi355x_matmul_bias) */
    STEP_ATTENTION, /* matmul(q, k^T) a -> [mul by a constant] -> [add of a bias or mask] -> softmax -> matmul(p, v): b, c, d, e
                     * (shl_mi355x_attention; with the add shl_mi355x_attention_bias) */
    STEP_CONV_ADD,  /* convolution a -> same-shape add b of its output and a skip tensor -> [relu | relu6 c] (shl_mi355x_conv_add_forward) */
    STEP_CONV_LUT,  /* convolution or depthwise layer a -> table activation b -> [mul c of a's output and b's: a swish / hard-swish
                     * gate] (shl_mi355x_conv_lut_forward; a depthwise plan: shl_mi355x_dwconv_lut_forward) */
};

struct step {
    enum step_kind kind;
    int a, b, c, d;       /* layer indices in order; -1 from the first unused one on (STEP_LAYER: b, a pair: c).  STEP_CONV_ADD:
                           * a, b, [c], and d = which of the add's operands (0 or 1) is the skip tensor */
    struct shl_node *out; /* the tensor node the step finally writes (a split: the first of them) */
    uint8_t lut[256];     /* STEP_CONV_LUT: the table of b (and c), built at plan time from the layers' records */
    int e;                /* STEP_ATTENTION only: the chain's fifth layer, -1 when it has four or three */
    int fold[4];          /* STEP_ATTENTION only: the reshape / transpose layers in front of q, k, v and behind the output that the
                           * launch stands for (shl_mi355x_attention_layout); all 0: the dense launch */
};

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
    int nfused, nfolded;
    int npool; /* global_avgpool2d layers that run inside their consumer's launch */
    int nlinear; /* matmul layers that add the constant bias behind them in their own launch */
    int nattention; /* Q K^T -> [scale] -> [+ bias] -> softmax -> P V chains that run as one launch */
    int nattention_bias; /* ... those of them with the add of a bias or mask */
    int nhead_moves; /* reshape / transpose layers around attention cores that those launches read and write through strides */
    int nresidual; /* convolution -> add -> [relu | relu6] tails of skip connections that run as one launch */
    int nactivation; /* table activations (gates included) that run inside their convolution's launch */
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

/* matmul a -> add b, the add's other operand a constant whose only dim that is not 1 is the last and equals N ([N], [1,N],
 * [1,1,N], ...): the index (0 or 1) of that constant among the add's inputs, -1 when the pair does not fuse.  The add must be
 * a broadcasting one that the backend takes (one record per tensor, equal dtypes) and reads `mid` once */
static int linear_bias_input(struct shl_node *a, struct shl_node *b, struct shl_node *mid)
{
    if (a->type != CSINN_OP_MATMUL || b->type != CSINN_OP_ADD || session_op(a) == NULL || session_op(b) == NULL) return -1;
    if (a->in_num != 2 || b->in_num != 2 || (b->in[0] == mid) == (b->in[1] == mid)) return -1;
    const int k = b->in[0] == mid ? 1 : 0;
    struct csinn_tensor *c = b->in[k]->data, *tm = mid->data, *out = b->out[0]->data;
    if (!c->is_const || c->data == NULL || c->dim_count < 1 || tm->dim_count < 2 || out->dim_count != tm->dim_count) return -1;
    const int32_t n = tm->dim[tm->dim_count - 1];
    if (c->dim[c->dim_count - 1] != n || n < 2) return -1;
    for (int i = 0; i < c->dim_count - 1; i++)
        if (c->dim[i] != 1) return -1;
    int64_t rows = 1;
    for (int i = 0; i < tm->dim_count; i++) {
        if (out->dim[i] != tm->dim[i]) return -1;
        if (i < tm->dim_count - 1) rows *= tm->dim[i];
    }
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

static int one_record_i8(const struct csinn_tensor *t);
static int one_record_f16(const struct csinn_tensor *t);

/* ---- the head split and merge moves around an attention core (shl_mi355x_attention_layout) ------------------------------------- */
#define FOLD_MAX 4 /* layers of one run */

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
 * exactly one consumer and no graph output) or starts from it (out = 1: the layers that consume x and each other).  want > 0: a
 * run of exactly that many layers (the plan has decided), else the longest the strides express.  Returns the run's length, its
 * layers in graph order in `run`, the tensor at its far end in *far (the source the launch reads / the tensor it writes) and
 * the view's heads and strides; 0 when nothing folds.  rows / cols / batches: what the view must come out as; swap: x is
 * [.., cols, rows] (K without trans_b) */
static int head_moves(struct shl_ref_graph *g, struct shl_node *x, int out, int swap, int want, int32_t batches, int32_t rows,
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
    for (int len = want > 0 ? want : n; len >= 1 && len <= n; len--) {
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
        if (want > 0) break;
    }
    return 0;
}

/* The layout descriptor of a chain attention_chain has described (layers, len, *d; k_swapped: its K is [.., d, t]): which moves
 * around it fold (want: NULL for the longest runs, else the counts the plan stored), the tensors the launch then reads and
 * writes (src[0..2], *dst; the chain's own where a side does not fold) and *ld.  Each side folds or stays on its own; sides
 * whose views split the batch index differently cannot share `heads`, and the later of them stays.  Returns the layers folded */
static int attention_layout(struct shl_ref_graph *g, const int *layers, int len, const struct shl_mi355x_attention_desc *d, int k_swapped,
                            const int *want, int fold[4], int runs[4][FOLD_MAX], struct shl_node *src[3], struct shl_node **dst,
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
        fold[i] = want != NULL && want[i] == 0 ? 0
                                                : head_moves(g, x[i], i == 3, i == 1 && k_swapped, want ? want[i] : 0, d->batches, rows[i], cols[i],
                                                             runs[i], &far, &heads[i], st[i]);
        if (fold[i] > 0 && heads[i] != d->batches) { /* two pieces: the split every other side must share */
            if (ld->heads == d->batches) ld->heads = heads[i];
            else if (ld->heads != heads[i]) fold[i] = 0, far = x[i];
        }
        if (fold[i] == 0) heads[i] = d->batches, st[i][0] = 0, st[i][1] = rows[i] * cols[i], st[i][2] = cols[i]; /* dense */
        if (i < 3) src[i] = far;
        else *dst = far;
        total += fold[i];
    }
    if (want != NULL)
        for (int i = 0; i < 4; i++)
            if (fold[i] != want[i]) return -1;
    /* one piece (heads = batches: the index is bi * head) is two pieces under any split */
    for (int i = 0; i < 4; i++)
        if (heads[i] == d->batches && ld->heads != d->batches) st[i][0] = ld->heads * st[i][1];
    /* (an int8 mover under these records copies bytes; a binary16 one applies its rule for infinities and NaNs) */
    for (int i = 0; i < 4; i++)
        if (fold[i] > 0) ld->moved |= 1 << i;
    return total;
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
    if (tm->dim_count != 4 || ts->dim_count != 4 || to->dim_count != 4) return -1;
    for (int i = 0; i < 4; i++)
        if (ts->dim[i] != tm->dim[i] || to->dim[i] != tm->dim[i]) return -1;
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

static int same_dims(const struct csinn_tensor *x, const struct csinn_tensor *y)
{
    if (x->dim_count != y->dim_count) return 0;
    for (int i = 0; i < x->dim_count; i++)
        if (x->dim[i] != y->dim[i]) return 0;
    return 1;
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
    struct shl_node *a = g->layer[steps[0].a], *b = g->layer[steps[1].a], *mid = steps[0].out;
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
    struct shl_node *c = g->layer[steps[2].a], *gate = b->out[0];
    if (c->type != CSINN_OP_MUL || session_op(c) == NULL || c->in_num != 2 || consumers_of(g, gate) != 1) return 0;
    const int x_first = c->in[0] == mid && c->in[1] == gate;
    if (!x_first && !(c->in[0] == gate && c->in[1] == mid)) return 0;
    struct csinn_tensor *tc = c->out[0]->data;
    if (!one_record_i8(tc) || !same_dims(tm, tc)) return 0; /* (the same-shape mul: nothing is broadcast) */
    shl_mi355x_gate_mul_table_i8(b->type == CSINN_OP_HARD_SIGMOID ? SHL_MI355X_UNARY_HARD_SIGMOID : SHL_MI355X_UNARY_SIGMOID, si, zi, so, zo,
                                 x_first, tc->qinfo->scale, tc->qinfo->zero_point, lut);
    return 3;
}

/* can steps `s` and `next` (adjacent, each still one layer) run as one launch, and as which?  STEP_LAYER: no.
 * residual: 0 no residual tails, 1 those of the measured shape classes, 2 every one the kernel takes */
static enum step_kind merged_kind(struct shl_ref_graph *g, const struct step *s, const struct step *next, int residual)
{
    struct shl_node *a = g->layer[s->a], *b = g->layer[next->a], *mid = s->out;
    /* a linear layer as converters export it: MatMul(x, W) -> Add(., bias[N]), the bias on either side of the add */
    if (consumers_of(g, mid) == 1 && linear_bias_input(a, b, mid) >= 0) return STEP_MATMUL_BIAS;
    /* the tail of a skip connection: convolution -> add(conv_out, skip), the convolution's output on either side of the add */
    if (residual && consumers_of(g, mid) == 1 && residual_skip_input(a, b, mid, residual == 2) >= 0) return STEP_CONV_ADD;
    if (b->in[0] != mid || consumers_of(g, mid) != 1) return STEP_LAYER;
    /* global_avgpool2d -> the convolution / fullyconnected layer on the pooled map: one launch (csrc/conv_gemv.hip) */
    if (a->type == CSINN_OP_GLOBAL_AVGPOOL2D && (is_conv_op(b->type) || b->type == CSINN_OP_FULLYCONNECTED)) {
        struct csinn_tensor *pin = a->in[0]->data, *pmid = mid->data;
        struct csinn_pool_params *pp = a->data;
        shl_mi355x_conv_plan *pb = shl_mi355x_registry_get(b->data);
        const int nhwc = pp->base.layout == CSINN_LAYOUT_NHWC;
        if (pb && nhwc && pin->dim_count == 4 && pin->dtype == CSINN_DTYPE_INT8 && pin->qinfo && pmid->qinfo &&
            pin->quant_channel <= 1 && pmid->quant_channel <= 1 &&
            shl_mi355x_pool_conv_fusable(pb, pin->dim[0], pin->dim[1] * pin->dim[2]))
            return STEP_POOL_CONV;
    }
    /* 1x1 convolution -> global_avgpool2d, the pooled tensor being all anything reads of it: one launch
     * (csrc/conv1x1_latency.hip: the workgroup of a channel slice holds the whole map) */
    if (is_conv_op(a->type) && b->type == CSINN_OP_GLOBAL_AVGPOOL2D) {
        struct csinn_tensor *cin = a->in[0]->data, *pmid = mid->data, *pout = b->out[0]->data;
        struct csinn_pool_params *pp = b->data;
        shl_mi355x_conv_plan *pa = shl_mi355x_registry_get(a->data);
        if (pa && pp->base.layout == CSINN_LAYOUT_NHWC && pmid->dim_count == 4 && pmid->dtype == CSINN_DTYPE_INT8 && pmid->qinfo &&
            pout->qinfo && pmid->quant_channel <= 1 && pout->quant_channel <= 1 &&
            shl_mi355x_conv_pool_fusable(pa, cin->dim[0]))
            return STEP_CONV_POOL;
    }
    /* pointwise -> depthwise (latency form, small batches) or depthwise -> pointwise (bandwidth form, large
     * batches: csrc/dwpw_stream.hip); shl_mi355x_pwdw_fusable tells the orders apart by the plans */
    if ((is_conv_op(a->type) && is_dw_op(b->type)) || (is_dw_op(a->type) && is_conv_op(b->type))) {
        shl_mi355x_conv_plan *pa = shl_mi355x_registry_get(a->data), *pb = shl_mi355x_registry_get(b->data);
        struct csinn_tensor *in = a->in[0]->data;
        if (pa && pb && shl_mi355x_pwdw_fusable(pa, pb, in->dim[0])) return STEP_PWDW;
    }
    return STEP_LAYER;
}

/* Graph-level rewrites; the intermediate tensors then never exist in HBM:
 *   conv / depthwise / deconv2d (no activation) -> relu | relu6, the convolution's only consumer, same output record
 *        the activation moves into the convolution's epilogue (the relu layer gets no step, the convolution's step writes
 *        the relu's output): what a converter emits for a RISC-V target -- example/c906_mobilenetv1_f16.c is
 *        28 csinn_conv2d + 27 csinn_relu -- runs as 28 launches, not 55
 *   1x1 convolution -> depthwise 3x3   one launch of csrc/pwdw_fused.hip (int8 NHWC) / pwdw_f16_nchw.hip (STEP_PWDW)
 *   depthwise 3x3 -> 1x1 convolution   one launch of csrc/dwpw_stream.hip at throughput batches (32 / 64 / 128 / 256 channels:
 *        the requantised depthwise tile is the pointwise MFMA operand); the latency form of this pairing recomputed the
 *        depthwise tile in every channel slice and is parked (attic/README.md)
 *   matmul -> add of a constant bias [N], the matmul's only consumer   one launch of csrc/matmul.hip's BIAS instantiation
 *        (STEP_MATMUL_BIAS): the linear layer a converter exports as MatMul + Add; the add's arithmetic runs on the value the
 *        matmul would have stored, so the step equals the two layers bit for bit
 *   matmul(q, k, trans_b) -> [mul by a one-element constant] -> [add of a bias or mask broadcast to the scores] -> softmax over
 *        the last axis -> matmul(p, v), every intermediate
 *        read by the next layer only   one launch of csrc/attention.hip (STEP_ATTENTION) where both products take matmul's mfma
 *        form: the scores and the probabilities stay in LDS, each computed as its own kernel would store it, so the step equals
 *        the layers bit for bit.  By default only shape classes it was measured faster on (csrc/attention_canon.h:att_default,
 *        with the add att_bias_default); SHL_MI355X_ATTENTION=1 merges every chain the kernel takes, =0 keeps the layers apart
 *   convolution (int8 NHWC, implicit GEMM; its folded activation included) -> add(conv_out, skip) of equal shapes, the convolution's
 *        only consumer -> [relu | relu6, the sum's only consumer]   one launch of the convolution (STEP_CONV_ADD, csrc/conv_igemm.hip's
 *        instantiations with the post-op): the add's and the activation's element functions run on the byte the convolution would
 *        have stored, so the step equals the layers bit for bit.  A convolution that is already half of a pair or feeds a pool is
 *        not taken (those merges come first).  By default only shape classes the fused launch was measured faster on
 *        (csrc/residual_validate.h:residual_default); SHL_MI355X_RESIDUAL=1 merges every tail the kernel takes, =0 none
 *   convolution (int8 NHWC, implicit GEMM; its folded activation included) -> sigmoid | hard_sigmoid | silu | leaky_relu, the
 *        convolution's only consumer, or -> sigmoid | hard_sigmoid -> mul(conv_out, gate), a swish / hard-swish gate   one launch of
 *        the convolution (STEP_CONV_LUT, csrc/conv_igemm.hip's instantiations with the table post-op): on int8 the layers are a
 *        function of the byte the convolution would have stored, ONE 256-entry table built here from their records with the
 *        layers' own builders, so the step equals the layers bit for bit.  Tried after the merges above: a convolution that is
 *        half of a pair, feeds a pool or a residual tail is not taken, and the step is not the first half of a residual merge.
 *        By default only shape classes the fused launch was measured faster on (csrc/lut_validate.h:lut_default);
 *        SHL_MI355X_ACT_FUSE=1 merges every one the kernel takes, =0 none
 *   depthwise layer (int8 NHWC, depth multiplier 1; its folded activation included) -> the same activations and gates   one launch
 *        of the depthwise kernel (STEP_CONV_LUT as well, csrc/dwconv.hip's and csrc/dwconv_mfma.hip's instantiations with the
 *        table post-op; the launch site picks the entry point by the plan's algorithm): MobileNetV3's depthwise -> hard-swish and
 *        EfficientNet's depthwise -> swish.  Same patterns, reader counts, tables, order and switch; a depthwise layer that is
 *        half of a pair is not taken.  The default classes: csrc/lut_validate.h:dw_lut_default
 * Fills ds->steps. */
static int plan_fusion(struct dev_session *ds, struct shl_ref_graph *g)
{
    struct step *steps = ds->steps = calloc((size_t)g->layer_index, sizeof(*steps));
    if (steps == NULL) return 0;
    const char *off = getenv("SHL_MI355X_NO_FUSION");
    const int fold = !(off && off[0] == '1');
    int ns = 0;
    /* one step per layer; an activation that folds joins the convolution's step */
    for (int i = 0; i < g->layer_index; i++) {
        struct shl_node *a = g->layer[i], *b = i + 1 < g->layer_index ? g->layer[i + 1] : NULL;
        struct step *s = &steps[ns++];
        *s = (struct step){STEP_LAYER, i, -1, -1, -1, a->out[0]};
        const int plain = a->type == CSINN_OP_CONV2D || a->type == CSINN_OP_DEPTHWISE_CONV2D;
        const int deconv = a->type == CSINN_OP_DECONV2D || a->type == CSINN_OP_DEPTHWISE_DECONV2D;
        if (!fold || !(plain || deconv) || b == NULL || (b->type != CSINN_OP_RELU && b->type != CSINN_OP_RELU6)) continue;
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
     * (the plan pair test below cannot see a layer's consumer: ADVICE r05 -- dw 32 -> pw 16 of MobileNetV2, two consumers, ...) */
    for (int k = 0; k < ns; k++) {
        struct shl_node *a = g->layer[steps[k].a], *b = k + 1 < ns ? g->layer[steps[k + 1].a] : NULL;
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
    /* merge adjacent steps greedily from the front; a merged step is not the first half of another merge
     * (SHL_MI355X_NO_FUSION=1 also keeps a matmul and its bias add apart: the switch of the linear fusion's A/B runs) */
    /* SHL_MI355X_ATTENTION, read here, at plan time: "0" keeps the chain's layers apart, "1" merges every chain the kernel takes
     * (A/B runs), unset merges the shape classes the fused launch was measured faster on */
    const char *att = getenv("SHL_MI355X_ATTENTION");
    const int attention = fold && !(att && att[0] == '0'), force = att && att[0] == '1';
    /* SHL_MI355X_RESIDUAL likewise: "0" none, "1" every tail the kernel takes, unset the measured shape classes */
    const char *res = getenv("SHL_MI355X_RESIDUAL");
    const int residual = !fold || (res && res[0] == '0') ? 0 : (res && res[0] == '1') ? 2 : 1;
    /* SHL_MI355X_ACT_FUSE likewise, for the table activations */
    const char *af = getenv("SHL_MI355X_ACT_FUSE");
    const int act_fuse = !fold || (af && af[0] == '0') ? 0 : (af && af[0] == '1') ? 2 : 1;
    /* SHL_MI355X_ATTENTION_LAYOUT likewise, for the reshape / transpose runs around a merged core: "0" folds none, "1" every run
     * the kernel takes, unset the classes one layout launch was measured faster on (shl_mi355x_attention_layout_by_default) --
     * unset, a core the dense default leaves apart merges too when all four sides fold and its class was measured faster */
    const char *lay = getenv("SHL_MI355X_ATTENTION_LAYOUT");
    const int layout = !attention || (lay && lay[0] == '0') ? 0 : (lay && lay[0] == '1') ? 2 : 1;
    char *gone = calloc((size_t)g->layer_index + 1, 1); /* layers an attention launch stands for */
    if (gone == NULL) return 0;
    for (int k = 0; k < ns; k++) {
        struct step s = steps[k];
        if (s.kind == STEP_LAYER && gone[s.a]) continue; /* a move behind a core that took it */
        /* the core of an attention block first: its matmuls then are no longer candidates for a pair */
        int chain[5] = {-1, -1, -1, -1, -1}, avail = 0;
        for (; avail < 5 && k + avail < ns; avail++) chain[avail] = steps[k + avail].a;
        struct shl_mi355x_attention_desc ad;
        struct shl_mi355x_attention_bias_desc abd;
        struct shl_mi355x_attention_layout_desc ld;
        struct shl_node *bias = NULL, *src[3], *dst = NULL;
        int k_swapped = 0, fold4[4] = {0, 0, 0, 0}, runs[4][FOLD_MAX], folded = 0;
        int taken = attention ? attention_chain(g, chain, avail, force, &ad, &abd, &bias, &k_swapped) : 0;
        int promoted = 0;
        if (taken == 0 && layout == 1 && !force) { /* (with the moves on the scales the dense default's verdict may change) */
            taken = attention_chain(g, chain, avail, 1, &ad, &abd, &bias, &k_swapped);
            promoted = taken > 0;
        }
        if (taken > 0 && layout) {
            folded = attention_layout(g, chain, taken, &ad, k_swapped, NULL, fold4, runs, src, &dst, &ld);
            /* the last word belongs to the kernel's own rules, asked with made-up addresses that do not overlap */
            const void *a0 = (const void *)((uintptr_t)1 << 56), *a1 = (const void *)((uintptr_t)1 << 57), *a2 = (const void *)((uintptr_t)1 << 58),
                       *a3 = (const void *)((uintptr_t)1 << 59), *a4 = bias ? (const void *)((uintptr_t)1 << 60) : NULL;
            const struct shl_mi355x_attention_bias_desc *pb = bias ? &abd : NULL;
            if (folded > 0 && shl_mi355x_attention_layout_kernel_name(a0, a1, a2, a4, a3, &ad, pb, &ld)[0] == '\0') folded = 0;
            if (folded > 0 && layout == 1 && !shl_mi355x_attention_layout_by_default(a0, a1, a2, a4, a3, &ad, pb, &ld)) folded = 0;
            if (promoted && !(folded > 0 && fold4[0] && fold4[1] && fold4[2] && fold4[3])) folded = 0;
        }
        if ((promoted || k_swapped) && (folded <= 0 || (k_swapped && fold4[1] == 0))) taken = 0; /* the layers run one by one */
        if (taken > 0) {
            steps[ds->nsteps] = (struct step){STEP_ATTENTION, chain[0], chain[1], chain[2], taken >= 4 ? chain[3] : -1, steps[k + taken - 1].out};
            steps[ds->nsteps].e = taken == 5 ? chain[4] : -1;
            if (folded > 0) {
                for (int i = 0; i < 4; i++) {
                    steps[ds->nsteps].fold[i] = fold4[i];
                    for (int j = 0; j < fold4[i]; j++) gone[runs[i][j]] = 1;
                }
                steps[ds->nsteps].out = dst;
                ds->nhead_moves += folded;
            }
            ds->nsteps++;
            ds->nattention++;
            if (bias != NULL) ds->nattention_bias++;
            k += taken - 1; /* the chain's other steps are taken */
            continue;
        }
        enum step_kind kind = k + 1 < ns ? merged_kind(g, &s, &steps[k + 1], residual) : STEP_LAYER;
        if (kind == STEP_MATMUL_BIAS && !fold) kind = STEP_LAYER;
        if (kind != STEP_LAYER) {
            k++; /* the second step is taken */
            const int skip_at = kind == STEP_CONV_ADD ? residual_skip_input(g->layer[s.a], g->layer[steps[k].a], s.out, residual == 2) : -1;
            s = (struct step){kind, s.a, steps[k].a, -1, skip_at, steps[k].out};
            if (kind == STEP_CONV_ADD && k + 1 < ns && residual_takes_relu(g, s.out, g->layer[steps[k + 1].a])) {
                k++; /* ... and the activation behind the sum */
                s.c = steps[k].a;
                s.out = steps[k].out;
            }
            if (kind == STEP_PWDW) ds->nfused++;
            else if (kind == STEP_MATMUL_BIAS) ds->nlinear++;
            else if (kind == STEP_CONV_ADD) ds->nresidual++;
            else ds->npool++;
        } else if (act_fuse) {
            const int lut_taken = lut_chain(g, &steps[k], ns - k, act_fuse == 2, s.lut);
            if (lut_taken > 0) {
                s.kind = STEP_CONV_LUT;
                s.b = steps[k + 1].a;
                s.c = lut_taken == 3 ? steps[k + 2].a : -1;
                s.out = steps[k + lut_taken - 1].out;
                ds->nactivation++;
                k += lut_taken - 1; /* the activation's (and the mul's) steps are taken */
            }
        }
        steps[ds->nsteps++] = s;
    }
    /* the moves in FRONT of a core were steps before the core was found: mark and compact.  (This relies on a reshape or a
     * transpose never being part of a merged step -- no step kind above takes one --: a folded move inside a merged step would
     * still run, and nhead_moves would count a layer that did) */
    int kept = 0;
    for (int k = 0; k < ds->nsteps; k++)
        if (!(steps[k].kind == STEP_LAYER && gone[steps[k].a])) steps[kept++] = steps[k];
    ds->nsteps = kept;
    free(gone);
    return 1;
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

/* enqueue every step on the session stream, tensors resident in HBM */
static int enqueue_layers(struct dev_session *ds, struct shl_ref_graph *g)
{
    for (int k = 0; k < ds->nsteps; k++) {
        const struct step *s = &ds->steps[k];
        struct shl_node *n = g->layer[s->a], *nx = s->b >= 0 ? g->layer[s->b] : NULL;
        struct dev_tensor *in = lookup(ds, n->in[0]), *out = lookup(ds, s->out);
        const int batch = in->shadow.dim[0];
        int rc;
        switch (s->kind) {
            case STEP_POOL_CONV: {
                struct csinn_tensor *pin = n->in[0]->data, *pmid = n->out[0]->data;
                rc = status_of(shl_mi355x_pool_conv_forward(shl_mi355x_registry_get(nx->data), in->dev, out->dev, batch,
                                                            pin->dim[1] * pin->dim[2], pin->qinfo->scale, pin->qinfo->zero_point,
                                                            pmid->qinfo->scale, pmid->qinfo->zero_point, ds->stream));
                break;
            }
            case STEP_CONV_POOL: { /* the pool reads what the convolution (+ folded activation) would have written */
                struct csinn_tensor *pmid = nx->in[0]->data, *pout = nx->out[0]->data;
                rc = status_of(shl_mi355x_conv_pool_forward(shl_mi355x_registry_get(n->data), in->dev, NULL, out->dev, batch,
                                                            pmid->qinfo->scale, pmid->qinfo->zero_point, pout->qinfo->scale,
                                                            pout->qinfo->zero_point, ds->stream));
                break;
            }
            case STEP_MATMUL_BIAS: {
                const int kb = linear_bias_input(n, nx, n->out[0]);
                struct dev_tensor *b = lookup(ds, n->in[1]), *bias = kb >= 0 ? lookup(ds, nx->in[kb]) : NULL;
                rc = b && bias ? shl_mi355x_matmul_bias_forward(n->in[0]->data, n->in[1]->data, n->out[0]->data, nx->in[kb]->data,
                                                                nx->out[0]->data, n->data, kb == 0, in->dev, b->dev, bias->dev,
                                                                out->dev, ds->stream)
                               : CSINN_FALSE;
                break;
            }
            case STEP_ATTENTION: {
                const int chain[5] = {s->a, s->b, s->c, s->d, s->e}, len = s->d < 0 ? 3 : s->e < 0 ? 4 : 5;
                struct shl_node *pv = g->layer[chain[len - 1]], *bias = NULL;
                struct shl_mi355x_attention_desc ad;
                struct shl_mi355x_attention_bias_desc abd;
                struct dev_tensor *kk = lookup(ds, n->in[1]), *v = lookup(ds, pv->in[1]);
                int k_swapped = 0;
                if (!kk || !v || attention_chain(g, chain, len, 1, &ad, &abd, &bias, &k_swapped) != len) { /* (the plan has decided) */
                    rc = CSINN_FALSE;
                } else if (s->fold[0] || s->fold[1] || s->fold[2] || s->fold[3]) { /* through strides: the sources' buffers, the last folded layer's output */
                    struct shl_mi355x_attention_layout_desc ld;
                    struct shl_node *src[3], *dst = NULL;
                    int fold4[4], runs[4][FOLD_MAX];
                    struct dev_tensor *b = bias ? lookup(ds, bias) : NULL, *sq, *sk, *sv;
                    if (attention_layout(g, chain, len, &ad, k_swapped, s->fold, fold4, runs, src, &dst, &ld) <= 0 || dst != s->out ||
                        (bias && !b) || !(sq = lookup(ds, src[0])) || !(sk = lookup(ds, src[1])) || !(sv = lookup(ds, src[2])))
                        rc = CSINN_FALSE;
                    else
                        rc = shl_mi355x_attention_layout_forward(&ad, bias ? &abd : NULL, &ld, sq->dev, sk->dev, sv->dev, b ? b->dev : NULL,
                                                                 out->dev, ds->stream);
                } else if (k_swapped) {
                    rc = CSINN_FALSE; /* (a K without trans_b is merged only with its moves folded) */
                } else if (bias != NULL) { /* a constant bias is resident like any constant operand of an add */
                    struct dev_tensor *b = lookup(ds, bias);
                    rc = b ? shl_mi355x_attention_bias_forward(&ad, &abd, in->dev, kk->dev, v->dev, b->dev, out->dev, ds->stream) : CSINN_FALSE;
                } else {
                    rc = shl_mi355x_attention_forward(&ad, in->dev, kk->dev, v->dev, out->dev, ds->stream);
                }
                break;
            }
            case STEP_CONV_ADD: { /* the add and the activation read what the convolution (+ folded activation) would have written */
                struct shl_node *relu = s->c >= 0 ? g->layer[s->c] : NULL;
                const int ks = s->d; /* the add's operand that is the skip tensor */
                struct dev_tensor *skip = ks == 0 || ks == 1 ? lookup(ds, nx->in[ks]) : NULL;
                if (skip == NULL) {
                    rc = CSINN_FALSE;
                    break;
                }
                struct csinn_tensor *tskip = nx->in[ks]->data, *tsum = nx->out[0]->data, *tout = relu ? relu->out[0]->data : tsum;
                struct shl_mi355x_residual_desc rd = {ks == 1, tskip->qinfo->scale, tskip->qinfo->zero_point, tsum->qinfo->scale,
                                                      tsum->qinfo->zero_point, relu ? (relu->type == CSINN_OP_RELU6 ? 2 : 1) : 0,
                                                      tout->qinfo->scale, tout->qinfo->zero_point};
                /* (the plan's dtype is the sum's: binary16 has entry points of its own, which read conv_first and act alone) */
                rc = status_of(tsum->dtype == CSINN_DTYPE_FLOAT16
                                   ? shl_mi355x_conv_add_f16_forward(shl_mi355x_registry_get(n->data), in->dev, skip->dev, out->dev, batch, &rd,
                                                                     ds->stream)
                                   : shl_mi355x_conv_add_forward(shl_mi355x_registry_get(n->data), in->dev, skip->dev, out->dev, batch, &rd,
                                                                 ds->stream));
                break;
            }
            case STEP_CONV_LUT: { /* the table's input is what the convolution (+ folded activation) would have written */
                shl_mi355x_conv_plan *plan = shl_mi355x_registry_get(n->data);
                rc = status_of(shl_mi355x_conv_plan_algo(plan) == SHL_MI355X_ALGO_DW
                                   ? shl_mi355x_dwconv_lut_forward(plan, in->dev, out->dev, batch, s->lut, ds->stream)
                                   : shl_mi355x_conv_lut_forward(plan, in->dev, out->dev, batch, s->lut, ds->stream));
                break;
            }
            case STEP_PWDW:
                rc = status_of(shl_mi355x_pwdw_forward(shl_mi355x_registry_get(n->data), shl_mi355x_registry_get(nx->data), in->dev,
                                                       out->dev, batch, ds->stream));
                break;
            default:
                rc = run_layer(ds, n, out);
        }
        if (rc != CSINN_TRUE) {
            shl_debug_error("mi355x: layer %d (%s) failed while building the device graph\n", s->a, n->name ? n->name : "?");
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

/* number of global_avgpool2d layers of `sess` that run inside the launch of the layer in front of or behind them */
int shl_mi355x_session_fused_pools(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? ds->npool : 0;
}

/* number of depthwise + pointwise pairs that run as one launch in `sess` */
int shl_mi355x_session_fused_pairs(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? ds->nfused : 0;
}

/* number of relu / relu6 layers of `sess` that run inside the epilogue of the convolution in front of them */
int shl_mi355x_session_folded_activations(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? ds->nfolded : 0;
}

/* number of matmul layers of `sess` that add the constant bias behind them inside their own launch */
int shl_mi355x_session_fused_linears(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? ds->nlinear : 0;
}

/* number of Q K^T -> [scale] -> [+ bias] -> softmax -> P V chains of `sess` that run as one launch */
int shl_mi355x_session_fused_attentions(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? ds->nattention : 0;
}

/* how many reshape / transpose layers around those cores run inside their launches (shl_mi355x_attention_layout) */
int shl_mi355x_session_folded_head_moves(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? ds->nhead_moves : 0;
}

/* ... and how many of those carry the add of a bias or mask (shl_mi355x_attention_bias) */
int shl_mi355x_session_fused_attention_biases(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? ds->nattention_bias : 0;
}

/* number of convolution -> add -> [relu | relu6] tails of skip connections of `sess` that run as one launch */
int shl_mi355x_session_fused_residuals(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? ds->nresidual : 0;
}

/* number of table activations (gates included) of `sess` that run inside their convolution's launch */
int shl_mi355x_session_fused_activations(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? ds->nactivation : 0;
}

/* 2 when `sess` executes as one device-resident hipGraph, 1 when device-resident with every run enqueueing its layers
 * anew (no graph could be captured), 0 when host-staged */
int shl_mi355x_session_is_device_resident(struct csinn_session *sess)
{
    struct dev_session *ds = find_session(sess);
    return ds ? (ds->graph_exec ? 2 : 1) : 0;
}

"""The head split and merge moves folded into the attention launch inside a session (-m gpu).  test_attention_session's block --
three projections, a reshape and a transpose(0,2,1,3) to heads on each of q, k and v, the core, a transpose and a reshape back,
a projection, the residual -- under SHL_MI355X_ATTENTION=1 and SHL_MI355X_ATTENTION_LAYOUT=1 runs as one captured hipGraph whose
core AND eight movers are ONE step (shl_mi355x_session_fused_attentions == 1, shl_mi355x_session_folded_head_moves == 8), matches
the oracle chain as the existing test does, and equals, bit for bit, the same net under SHL_MI355X_ATTENTION_LAYOUT=0; the other
planner counters do not move.  Nets that must keep moves apart: a second consumer of qh (6 folded), an int8 transpose whose output
record differs from its input's (6), a transpose(0,1,3,2) the strides cannot express (6), p as a graph output and a second
consumer of the scaled scores (nothing merges, nothing folds).  K as ONNX exports it -- transpose(0,2,3,1) into a product
without trans_b -- folds 8 and stays apart without the fold; a BERT-style net with a padding mask folds 8 around a biased core.
Unset, the planner folds exactly the classes csrc/attention_canon.h:att_layout_default admits."""
import numpy as np
import pytest

import matmul_cases as mc
from cases import pkg
from pool_cases import _q
from test_attention_bias_session import block
from test_attention_session import attention_net
from test_concat_session import matches, planner_counts

FORMATS = [("int8", "NHWC"), ("f16", "NCHW")]
CORE, LAYOUT = "SHL_MI355X_ATTENTION", "SHL_MI355X_ATTENTION_LAYOUT"
ENV = ("SHL_MI355X_HOST_SESSION", "SHL_MI355X_MATMUL_FORM", "SHL_MI355X_NO_FUSION", CORE, LAYOUT, "SHL_MI355X_TRANSPOSE_FORM",
       "SHL_MI355X_ADD_FORM", "SHL_MI355X_MUL_FORM")


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt


def _counts(opt, sess):
    return (opt.shl_mi355x_session_fused_attentions(sess), opt.shl_mi355x_session_fused_attention_biases(sess),
            opt.shl_mi355x_session_folded_head_moves(sess))


def _clean(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


def _built(fe, opt, net, monkeypatch, core, layout):
    """the net built under the two switches (None: unset); its counters"""
    for var, value in ((CORE, core), (LAYOUT, layout)):
        if value is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, value)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    return sess, _counts(opt, sess)


def _same_as_unfolded(fe, opt, make, monkeypatch, want_counts, oracle=None):
    """the net under both switches at 1 has want_counts, and equals -- on two inputs and a replay -- the same net under
    SHL_MI355X_ATTENTION_LAYOUT=0 bit for bit, with the other planner counters equal; oracle: the dtype whose oracle chain the
    output must match as well"""
    net = make()
    sess, counts = _built(fe, opt, net, monkeypatch, "1", "1")
    assert counts == want_counts
    got = [net.run(fe, net.input(k))["out"] for k in (0, 1, 0)]  # the graph replay reads fresh data
    assert not np.array_equal(mc.bits(got[0]), mc.bits(got[1])), "the two inputs must tell runs apart"
    mc.assert_same(got[2], got[0], "the replay on the first input")
    if oracle is not None:
        for k in (0, 1):
            want = net.oracle(net.input(k))["out"]
            assert got[k].shape == want.shape and matches(got[k], want, oracle), "input %d: the output differs from the oracle chain" % k
    apart = make()
    apart_sess, apart_counts = _built(fe, opt, apart, monkeypatch, "1", "0")
    assert apart_counts[2] == 0
    assert planner_counts(opt, sess) == planner_counts(opt, apart_sess)
    assert opt.shl_mi355x_session_fused_linears(sess) == opt.shl_mi355x_session_fused_linears(apart_sess)
    for k in (0, 1):
        mc.assert_same(apart.run(fe, apart.input(k))["out"], got[k], "input %d: the moves folded vs the moves as layers" % k)
    apart.close(fe)
    net.close(fe)
    return apart_counts


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", FORMATS)
def test_block_runs_as_one_hipgraph_with_the_eight_moves_in_the_attention_launch(gpu, dtype, layout, monkeypatch):
    fe, hip, opt = gpu
    _clean(monkeypatch)
    apart_counts = _same_as_unfolded(fe, opt, lambda: attention_net(dtype, layout), monkeypatch, (1, 0, 8), oracle=dtype)
    assert apart_counts == (1, 0, 0)
    # the core's own switch still keeps everything apart
    net = attention_net(dtype, layout)
    _, counts = _built(fe, opt, net, monkeypatch, "0", "1")
    assert counts == (0, 0, 0)
    net.close(fe)
    monkeypatch.setenv("SHL_MI355X_NO_FUSION", "1")
    net = attention_net(dtype, layout)
    _, counts = _built(fe, opt, net, monkeypatch, "1", "1")
    assert counts == (0, 0, 0)
    net.close(fe)


def _qh_read_twice(dtype, layout):
    net = attention_net(dtype, layout)
    net.tensors["qh2"] = net.tensors["qh"]
    net.layers.insert(len(net.layers) - 2, ("softmax", "qh_again", "qh", "qh2", dict(axis=3)))
    net.outputs.append("qh2")
    return net


def _k_requantised(dtype, layout):
    """the transpose to heads of k writes under another record than it reads (int8: it requantises, so it is no layout)"""
    net = attention_net(dtype, layout)
    shape, (scale, zp) = net.tensors["kh"]
    net.tensors["kh"] = (shape, _q(scale, zp + 1))
    return net


def _q_inner_swapped(dtype, layout):
    """q reaches the core through reshape [1,H,D,S] -> transpose(0,1,3,2): a view whose inner stride is not 1"""
    net = attention_net(dtype, layout)
    _, h, s, hd = net.shape("qh")
    net.tensors["qs"] = ((1, h, hd, s), net.tensors["qs"][1])
    at = next(i for i, l in enumerate(net.layers) if l[1] == "q_heads")
    net.layers[at] = ("transpose", "q_heads", "qs", "qh", dict(perm=(0, 1, 3, 2)))
    return net


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", FORMATS)
def test_moves_that_are_no_layout_stay_layers_and_the_other_sides_fold(gpu, dtype, layout, monkeypatch):
    fe, hip, opt = gpu
    _clean(monkeypatch)
    makers = [_qh_read_twice, _q_inner_swapped] + ([_k_requantised] if dtype == "int8" else [])
    for make in makers:
        _same_as_unfolded(fe, opt, lambda: make(dtype, layout), monkeypatch, (1, 0, 6))
    for kw in (dict(p_is_output=True), dict(second_consumer=True)):  # nothing merges, so nothing folds
        net = attention_net(dtype, layout, **kw)
        _, counts = _built(fe, opt, net, monkeypatch, "1", "1")
        assert counts == (0, 0, 0), kw
        net.close(fe)


def _k_as_onnx(dtype, layout):
    """K through transpose(0,2,3,1) into a product without trans_b"""
    net = attention_net(dtype, layout)
    _, h, s, hd = net.shape("kh")
    net.tensors["kh"] = ((1, h, hd, s), net.tensors["kh"][1])
    for i, l in enumerate(net.layers):
        if l[1] == "k_heads":
            net.layers[i] = ("transpose", "k_heads", "ks", "kh", dict(perm=(0, 2, 3, 1)))
        if l[1] == "qk":
            net.layers[i] = ("matmul", "qk", ("qh", "kh"), "s", {})
    return net


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", FORMATS)
def test_k_as_onnx_exports_it_folds_and_stays_apart_without_the_fold(gpu, dtype, layout, monkeypatch):
    fe, hip, opt = gpu
    _clean(monkeypatch)
    apart_counts = _same_as_unfolded(fe, opt, lambda: _k_as_onnx(dtype, layout), monkeypatch, (1, 0, 8), oracle=dtype)
    assert apart_counts == (0, 0, 0), "a chain without trans_b merges only where K's move folds"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", FORMATS)
def test_bert_style_net_with_a_mask_folds_around_the_biased_core(gpu, dtype, layout, monkeypatch):
    fe, hip, opt = gpu
    _clean(monkeypatch)
    bert = lambda: block(dtype, layout, 2, 80, 2, 64, (2, 1, 1, 80), bias_first=True, mask=True)
    apart_counts = _same_as_unfolded(fe, opt, bert, monkeypatch, (1, 1, 8), oracle=dtype)
    assert apart_counts == (1, 1, 0)


def _default(batches, s, t, d):
    """csrc/attention_canon.h:att_layout_default restated (profiles/attention_layout_notes.md)"""
    groups = batches * ((s + 31) // 32)
    return (49 <= t <= 197 and 32 <= d <= 64 and groups >= 21) or (d <= 32 and t >= 768 and groups <= 256)


@pytest.mark.gpu
def test_unasked_the_planner_folds_only_the_classes_measured_faster(gpu, monkeypatch):
    """both switches unset; the nets are built and captured, not run.  One shape inside each admitted class and its nearest
    neighbours outside.  Inside the short class the dense default leaves the core apart, and the moves bring it in; outside it
    neither merges.  (fused attentions, folded moves)"""
    fe, hip, opt = gpu
    _clean(monkeypatch)
    for n, tokens, h, hd, want in ((1, 197, 4, 64, (1, 8)),     # 28 workgroups of ViT's 197 keys
                                   (1, 197, 2, 64, (0, 0)),     # 14: below the smallest grid measured
                                   (1, 198, 4, 64, (0, 0)),     # not measured
                                   (1, 384, 4, 64, (0, 0)),     # an encoder of 384 tokens: 0.98 in binary16
                                   (16, 49, 3, 32, (1, 8)),     # Swin windows, 96 workgroups (k < 64 needs more than 65536 outputs)
                                   (1, 80, 2, 64, (0, 0)),      # the block of the tests above: 6 workgroups
                                   (1, 768, 2, 32, (1, 8)),     # the long class: the dense default merges it, the moves fold
                                   (1, 767, 2, 32, (0, 0))):
        assert _default(n * h, tokens, tokens, hd) == (want[1] == 8)
        # (attention_net has two heads on one batch: other grids through the block with a mask)
        net = attention_net("int8", "NHWC", tokens=tokens, hd=hd) if (n, h) == (1, 2) else \
            block("int8", "NHWC", n, tokens, h, hd, (n, 1, 1, tokens), mask=True)
        sess, counts = _built(fe, opt, net, monkeypatch, None, None)
        assert (counts[0], counts[2]) == want, (n, tokens, h, hd, counts)
        net.close(fe)
    # ... and with the core asked for but the layout left to the default, only the class decides about the moves
    net = attention_net("int8", "NHWC")
    _, counts = _built(fe, opt, net, monkeypatch, "1", None)
    assert counts == (1, 0, 0)
    net.close(fe)

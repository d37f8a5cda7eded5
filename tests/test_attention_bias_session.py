"""The biased attention core inside a session (-m gpu).  Three nets, each one captured hipGraph, whose chain matmul(q, k,
trans_b) -> mul by a constant -> add of a constant bias or mask -> softmax -> matmul(p, v) runs as ONE step under
SHL_MI355X_ATTENTION=1 (shl_mi355x_session_fused_attentions == shl_mi355x_session_fused_attention_biases == 1):

  linear     linear_cases.attention_bias -- 17 tokens, 2 heads of 32, batch 2, a constant [1,2,17,17] on the scaled scores -- with
             `out` as its only graph output (its p is one as well, which keeps any chain apart) and under
             SHL_MI355X_MATMUL_FORM=mfma: K = 32 on 2 x 2 x 17 x 17 scores is the chain form's by matmul's own rule, and the
             fused kernel exists against the mfma form only.  The switch holds for both sessions, so they run the same products
  swin       a window block: S = T = 49, 3 heads of 32, 4 windows, a constant relative position bias [1,3,49,49]; the chain form's
             by the same rule, under the same switch
  bert       80 tokens, 2 heads of 64, batch 2, a constant padding mask [2,1,1,80] of zeros and large negatives, given as the
             add's FIRST input; both products are the mfma form's unasked

Every net equals, bit for bit and on two inputs, the same net under SHL_MI355X_ATTENTION=0, whose other planner counters are the
same; the layers-apart net is held to LinearNet.oracle under test_linear_session.py's criteria (int8 bit for bit, binary16 within
1e-3).  Without the matmul switch the first two keep their layers; so do a net whose sum is a graph output, one whose sum is read
twice, one whose operands have equal shapes (the session runs that add through shl_mi355x_add, whose binary16 NaN rule is
another), and every net under SHL_MI355X_NO_FUSION=1.  Unasked, nothing outside att_bias_default's classes is merged; the two
classes inside it -- a DETR encoder layer at batch 1, Swin windows at batch 8 -- are, and equal their layers apart."""
import numpy as np
import pytest

import linear_cases
import matmul_cases as mc
from cases import pkg
from pool_cases import _q
from test_concat_session import matches, planner_counts

FORMATS = [("int8", "NHWC"), ("f16", "NCHW")]
SWITCH, FORM = "SHL_MI355X_ATTENTION", "SHL_MI355X_MATMUL_FORM"
ENV = ("SHL_MI355X_HOST_SESSION", FORM, "SHL_MI355X_NO_FUSION", SWITCH, "SHL_MI355X_ADD_FORM", "SHL_MI355X_MUL_FORM")


def block(dtype, layout, n, tokens, h, hd, bias_shape, bias_first=False, mask=False, extra=None):
    """test_attention_session.attention_net's layers and data rules (binary16: q, k and every partial sum of q k^T exact, only
    non-negative terms behind the softmax) on n batches of `tokens` tokens and h heads of hd channels, with a constant of
    bias_shape added to the scaled scores.  mask: the constant is 0 or a large negative (int8: -128 under a record that
    saturates the sum; binary16: -10000); else a non-negative bias.  extra: "sum_out" -- the sum is a graph output --,
    "sum_twice" -- a second softmax reads it"""
    q = lambda s, z: _q(2.0 ** s, z)
    rng = np.random.default_rng(211)
    s, c = tokens, h * hd
    flat, split, heads, scores = (n, s, c), (n, s, h, hd), (n, h, s, hd), (n, h, s, s)
    t = {"x": (flat, q(-4, -5)), "out": (flat, q(-3, 7)), "proj": (flat, q(-5, 3)),
         "s": (scores, q(-1, 5)), "sc": (scores, q(-4, -9)), "sb": (scores, q(-4, -20)), "p": (scores, _q(1.0 / 256, -128)),
         "p2": (scores, _q(1.0 / 256, -128)),
         "oh": (heads, q(-4, 3)), "os": (split, q(-4, 3)), "o": (flat, q(-4, 3))}
    for name, zp, e in (("q", -3, -5), ("k", 0, -5), ("v", 3, -4)):
        t[name] = (flat, q(e, zp))
        t[name + "s"] = (split, q(e, zp))
        t[name + "h"] = (heads, q(e, zp))
    signed, positive = (-1, 1, 1.0 / 8), (0, 2, 1.0 / 16)
    if mask:
        keep = rng.random(bias_shape) < 0.7
        ab = np.where(keep, 0, -128).astype(np.int8) if dtype == "int8" else np.where(keep, 0.0, -10000.0).astype(np.float16)
        ab_q = q(-1, 0)  # -128 is -64: -1024 LSB of the sum
    else:
        ab = rng.integers(-128, 128, bias_shape, dtype=np.int8) if dtype == "int8" else (rng.integers(0, 33, bias_shape) / 16.0).astype(np.float16)
        ab_q = q(-5, 0)
    consts = {"Wq": (mc._weights(rng, (c, c), dtype, signed), q(-11, 0)), "Wk": (mc._weights(rng, (c, c), dtype, signed), q(-11, 5)),
              "Wv": (mc._weights(rng, (c, c), dtype, positive), q(-10, 0)), "Wo": (mc._weights(rng, (c, c), dtype, positive), q(-10, -128)),
              "scale": (np.array([64], np.int8) if dtype == "int8" else np.array([0.125], np.float16), q(-9, 0)),
              "ab": (ab, ab_q)}
    L = []
    for name in "qkv":
        L += [("matmul", name, ("x", "W" + name), name, {}),
              ("reshape", name + "_split", name, name + "s", {}),
              ("transpose", name + "_heads", name + "s", name + "h", dict(perm=(0, 2, 1, 3)))]
    L += [("matmul", "qk", ("qh", "kh"), "s", dict(trans_b=True)),
          ("mulc", "scaled", "s", "sc", dict(const="scale")),
          ("addc", "attn_bias", "sc", "sb", dict(const="ab", first=bias_first)),
          ("softmax", "softmax", "sb", "p", dict(axis=3)),
          ("matmul", "pv", ("p", "vh"), "oh", {})]
    if extra == "sum_twice":
        L += [("softmax", "softmax2", "sb", "p2", dict(axis=3))]
    L += [("transpose", "o_tokens", "oh", "os", dict(perm=(0, 2, 1, 3))),
          ("reshape", "o_merge", "os", "o", {}),
          ("matmul", "proj", ("o", "Wo"), "proj", {}),
          ("add", "residual", ("proj", "x"), "out", {})]
    outputs = ["out"] + {"sum_out": ["sb"], "sum_twice": ["p2"]}.get(extra, [])
    return linear_cases.LinearNet(dtype, layout, 213, "x", t, L, outputs, consts, x_grid=(0, 4, 1.0 / 2))


def linear_net(dtype, layout):
    net = linear_cases.attention_bias(dtype, layout)
    net.outputs = ["out"]  # its p as a graph output would keep the chain apart
    return net


NETS = {"linear": (linear_net, "mfma"),
        "swin": (lambda dtype, layout, **kw: block(dtype, layout, 4, 49, 3, 32, (1, 3, 49, 49), **kw), "mfma"),
        "bert": (lambda dtype, layout, **kw: block(dtype, layout, 2, 80, 2, 64, (2, 1, 1, 80), bias_first=True, mask=True, **kw), None)}


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt


def _counts(opt, sess):
    return opt.shl_mi355x_session_fused_attentions(sess), opt.shl_mi355x_session_fused_attention_biases(sess)


def _others(opt, sess):
    return planner_counts(opt, sess) + (opt.shl_mi355x_session_fused_linears(sess), opt.shl_mi355x_session_fused_residuals(sess),
                                        opt.shl_mi355x_session_fused_activations(sess))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", FORMATS)
@pytest.mark.parametrize("which", sorted(NETS))
def test_net_runs_as_one_hipgraph_with_one_biased_attention(gpu, which, dtype, layout, monkeypatch):
    fe, hip, opt = gpu
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    make, form = NETS[which]
    if form:
        monkeypatch.setenv(FORM, form)
    monkeypatch.setenv(SWITCH, "1")
    net = make(dtype, layout)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    assert _counts(opt, sess) == (1, 1)
    got = [net.run(fe, net.input(k)) for k in (0, 1, 0)]  # the graph replay reads fresh data
    assert not np.array_equal(mc.bits(got[0]["out"]), mc.bits(got[1]["out"])), "the two inputs must tell runs apart"
    mc.assert_same(got[2]["out"], got[0]["out"], "%s %s: the same input again" % (which, dtype))
    # the same net with the layers kept apart: the same bits, the same other counters; and the oracle chain's values
    monkeypatch.setenv(SWITCH, "0")
    apart = make(dtype, layout)
    apart_sess = apart.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(apart_sess) == 2
    assert _counts(opt, apart_sess) == (0, 0)
    assert _others(opt, sess) == _others(opt, apart_sess)
    for k in (0, 1):
        res = apart.run(fe, apart.input(k))["out"]
        mc.assert_same(res, got[k]["out"], "%s %s input %d: fused vs the layers apart" % (which, dtype, k))
        want = apart.oracle(apart.input(k))
        assert matches(res, want["out"], dtype), "%s %s input %d: the layers apart differ from the oracle chain" % (which, dtype, k)
        assert np.unique(mc.bits(want["p"])).size > 8 and np.unique(mc.bits(want["out"])).size > 8
        assert not np.array_equal(mc.bits(want["sb"]), mc.bits(want["sc"])), "the bias must change the softmax's input"
    apart.close(fe)
    net.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", FORMATS)
def test_chains_the_launch_does_not_stand_for_keep_their_layers(gpu, dtype, layout, monkeypatch):
    """built and captured, not run"""
    fe, hip, opt = gpu
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    bert = NETS["bert"][0]

    def fused(net):
        sess = net.build(fe, pkg.API_MI355X)
        assert opt.shl_mi355x_session_is_device_resident(sess) == 2
        res = _counts(opt, sess)
        net.close(fe)
        return res
    monkeypatch.setenv(SWITCH, "1")
    assert fused(bert(dtype, layout)) == (1, 1)
    assert fused(bert(dtype, layout, extra="sum_out")) == (0, 0)    # the sum is a graph output
    assert fused(bert(dtype, layout, extra="sum_twice")) == (0, 0)  # ... is read twice
    assert fused(block(dtype, layout, 2, 80, 2, 64, (2, 2, 80, 80))) == (0, 0)  # operands of equal shape: shl_mi355x_add's layer
    assert fused(linear_cases.attention_bias(dtype, layout)) == (0, 0)  # the chain form's, and p is a graph output
    assert fused(linear_net(dtype, layout)) == (0, 0)                   # the chain form's
    assert fused(NETS["swin"][0](dtype, layout)) == (0, 0)              # the chain form's
    monkeypatch.setenv("SHL_MI355X_NO_FUSION", "1")
    assert fused(bert(dtype, layout)) == (0, 0)
    monkeypatch.delenv("SHL_MI355X_NO_FUSION")
    monkeypatch.setenv(SWITCH, "0")
    assert fused(bert(dtype, layout)) == (0, 0)
    # unasked: only the classes of csrc/attention_canon.h:att_bias_default, which 80 keys on heads of 64 are not among
    monkeypatch.delenv(SWITCH)
    assert fused(bert(dtype, layout)) == (0, 0)


DEFAULTS = {"detr_b1": lambda dtype, layout: block(dtype, layout, 1, 850, 8, 32, (1, 1, 1, 850), mask=True),      # 216 workgroups
            "swin_b8": lambda dtype, layout: block(dtype, layout, 512, 49, 3, 32, (1, 3, 49, 49), bias_first=True)}  # 3072


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", FORMATS)
@pytest.mark.parametrize("which", sorted(DEFAULTS))
def test_the_classes_fused_unasked_run_and_equal_the_layers_apart(gpu, which, dtype, layout, monkeypatch):
    """a DETR encoder layer at batch 1 and a Swin stage-1 block at batch 8: what att_bias_default fuses with SHL_MI355X_ATTENTION
    unset (profiles/attention_bias_notes.md).  One captured graph with one biased attention, which equals the same net under
    SHL_MI355X_ATTENTION=0 bit for bit on two inputs.  (The CPU oracle is not the arbiter at these sizes: test_attention_bias.py
    and the three nets above carry it)"""
    fe, hip, opt = gpu
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    net = DEFAULTS[which](dtype, layout)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    assert _counts(opt, sess) == (1, 1)
    got = [net.run(fe, net.input(k))["out"] for k in (0, 1)]
    assert not np.array_equal(mc.bits(got[0]), mc.bits(got[1])), "the two inputs must tell runs apart"
    monkeypatch.setenv(SWITCH, "0")
    apart = DEFAULTS[which](dtype, layout)
    apart_sess = apart.build(fe, pkg.API_MI355X)
    assert _counts(opt, apart_sess) == (0, 0) and _others(opt, sess) == _others(opt, apart_sess)
    for k in (0, 1):
        mc.assert_same(apart.run(fe, apart.input(k))["out"], got[k], "%s %s input %d: fused by default vs the layers apart" % (which, dtype, k))
    apart.close(fe)
    net.close(fe)

"""The fused attention core inside a session (-m gpu): an attention block on 80 tokens of C = 128 channels, 2 heads of 64 --
three matmuls against constant weights, reshape / transpose to heads, matmul(q, k, trans_b), mul by a constant scale, softmax
over the last axis, matmul(p, v), transpose / reshape back, a matmul against a constant, add of the residual; only `out` is a
graph output -- runs, under SHL_MI355X_ATTENTION=1 (80 keys on heads of 64 are not among the shapes the fused launch was measured
faster on, which are all the planner merges unasked), as one hipGraph whose four core layers are ONE step
(shl_mi355x_session_fused_attentions == 1), matches the oracle chain (int8 bit for bit: every matmul's records lie inside the plan-time proof; binary16 within 1e-3) and equals, bit for
bit, the same net built under SHL_MI355X_ATTENTION=0; the other planner counters do not move.  matmul_cases.attention_block
(K = 32 at 17 tokens is the chain form's, and p is a graph output) and a net whose scaled scores have a second consumer keep
their layers apart.  Also behind the genuine front-end and graph executor."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import matmul_cases as mc
from cases import pkg
from pool_cases import _q
from test_concat_session import matches, planner_counts

FORMATS = [("int8", "NHWC"), ("f16", "NCHW")]
SWITCH = "SHL_MI355X_ATTENTION"


def attention_net(dtype="int8", layout="NCHW", second_consumer=False, tokens=80, hd=64, records=None, p_is_output=False):
    """matmul_cases.attention_block's layers at S = 80, C = 128, 2 heads of 64 (K = 64 and 80: both products are the mfma
    form's).  int8: every record is a power of two inside the plan-time proof.  binary16: x is a multiple of 1/2 in [0, 2] and
    Wq, Wk are -1/8, 0 or 1/8, so q, k (multiples of 2^-4 up to 32) are exact in binary16 and every partial sum of q k^T (a
    multiple of 2^-8 below 2^16) is exact in float32: the scores and p are the same bits in any order of summation; Wv and Wo
    are 0, 1/16 or 1/8, so everything behind the softmax is a sum of non-negative terms.  second_consumer: the scaled scores
    also feed a second softmax (a graph output), behind the chain.  records: int8 records by tensor or constant name that replace
    the ones below (which suit 80 tokens: on 768 keys they leave p nearly flat).  p_is_output: p is a graph output as well, which
    keeps the layers apart"""
    q = lambda s, z: _q(2.0 ** s, z)
    rng = np.random.default_rng(171)
    s, h = tokens, 2
    c = h * hd
    flat, split, heads = (1, s, c), (1, s, h, hd), (1, h, s, hd)
    t = {"x": (flat, q(-4, -5)), "out": (flat, q(-3, 7)), "proj": (flat, q(-5, 3)),
         "s": ((1, h, s, s), q(-1, 5)), "sc": ((1, h, s, s), q(-4, -9)), "p": ((1, h, s, s), _q(1.0 / 256, -128)),
         "p2": ((1, h, s, s), _q(1.0 / 256, -128)),
         "oh": (heads, q(-4, 3)), "os": (split, q(-4, 3)), "o": (flat, q(-4, 3))}
    for n, zp, e in (("q", -3, -5), ("k", 0, -5), ("v", 3, -4)):
        t[n] = (flat, q(e, zp))
        t[n + "s"] = (split, q(e, zp))
        t[n + "h"] = (heads, q(e, zp))
    signed, positive = (-1, 1, 1.0 / 8), (0, 2, 1.0 / 16)
    consts = {"Wq": (mc._weights(rng, (c, c), dtype, signed), q(-11, 0)), "Wk": (mc._weights(rng, (c, c), dtype, signed), q(-11, 5)),
              "Wv": (mc._weights(rng, (c, c), dtype, positive), q(-10, 0)), "Wo": (mc._weights(rng, (c, c), dtype, positive), q(-10, -128)),
              "scale": (np.array([64], np.int8) if dtype == "int8" else np.array([0.125], np.float16), q(-9, 0))}
    for name, rec in (records or {}).items():
        if name in consts:
            consts[name] = (consts[name][0], rec)
        else:
            t[name] = (t[name][0], rec)
    L = []
    for n in "qkv":
        L += [("matmul", n, ("x", "W" + n), n, {}),
              ("reshape", n + "_split", n, n + "s", {}),
              ("transpose", n + "_heads", n + "s", n + "h", dict(perm=(0, 2, 1, 3)))]
    L += [("matmul", "qk", ("qh", "kh"), "s", dict(trans_b=True)),
          ("mulc", "scaled", "s", "sc", dict(const="scale")),
          ("softmax", "softmax", "sc", "p", dict(axis=3)),
          ("matmul", "pv", ("p", "vh"), "oh", {})]
    if second_consumer:
        L += [("softmax", "softmax2", "sc", "p2", dict(axis=3))]
    L += [("transpose", "o_tokens", "oh", "os", dict(perm=(0, 2, 1, 3))),
          ("reshape", "o_merge", "os", "o", {}),
          ("matmul", "proj", ("o", "Wo"), "proj", {}),
          ("add", "residual", ("proj", "x"), "out", {})]
    return mc.MatmulNet(dtype, layout, 173, "x", t, L, ["out"] + (["p2"] if second_consumer else []) + (["p"] if p_is_output else []), consts, x_grid=(0, 4, 1.0 / 2))


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", FORMATS)
def test_block_runs_as_one_hipgraph_with_one_fused_attention(gpu, dtype, layout, monkeypatch):
    fe, hip, opt = gpu
    for var in ("SHL_MI355X_HOST_SESSION", "SHL_MI355X_MATMUL_FORM", "SHL_MI355X_NO_FUSION", SWITCH):
        monkeypatch.delenv(var, raising=False)
    net = attention_net(dtype, layout)
    if dtype == "int8":  # the comparison is bit for bit because the proof holds for every matmul
        for kind, name, src, dst, info in net.layers:
            if kind == "matmul":
                case = net._matmul_case(src, dst, info, a=np.zeros(net.shape(src[0]), np.int8),
                                        b=np.zeros(net.shape(src[1]), np.int8) if src[1] not in net.consts else None)
                assert mc.is_exact(dict(case, k=case["a"].shape[-1])), name
    monkeypatch.setenv(SWITCH, "1")
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    assert opt.shl_mi355x_session_fused_attentions(sess) == 1
    want = {k: net.oracle(net.input(k)) for k in (0, 1)}
    got = [net.run(fe, net.input(k)) for k in (0, 1, 0)]  # the graph replay reads fresh data
    for k, g in zip((0, 1, 0), got):
        assert g["out"].shape == want[k]["out"].shape
        assert matches(g["out"], want[k]["out"], dtype), "%s %s input %d: the output differs from the oracle chain" % (dtype, layout, k)
    assert not np.array_equal(want[0]["out"], want[1]["out"]), "the two inputs must tell runs apart"
    for name in ("p", "out"):
        spread = np.unique(mc.bits(want[0][name])).size
        assert spread > 8, "%s of the oracle chain holds %d different values: it would tell nothing" % (name, spread)
    # the same net with the layers kept apart: the same bits, the same other counters
    monkeypatch.setenv(SWITCH, "0")
    apart = attention_net(dtype, layout)
    apart_sess = apart.build(fe, pkg.API_MI355X)
    monkeypatch.delenv(SWITCH)
    assert opt.shl_mi355x_session_is_device_resident(apart_sess) == 2
    assert opt.shl_mi355x_session_fused_attentions(apart_sess) == 0
    assert planner_counts(opt, sess) == planner_counts(opt, apart_sess)
    assert opt.shl_mi355x_session_fused_linears(sess) == opt.shl_mi355x_session_fused_linears(apart_sess)
    for k, g in zip((0, 1, 0), got):
        mc.assert_same(apart.run(fe, apart.input(k))["out"], g["out"], "%s input %d: fused vs the layers apart" % (dtype, k))
    apart.close(fe)
    net.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", FORMATS)
def test_chains_the_kernel_does_not_take_keep_their_layers(gpu, dtype, layout, monkeypatch):
    fe, hip, opt = gpu
    for var in ("SHL_MI355X_HOST_SESSION", "SHL_MI355X_MATMUL_FORM", "SHL_MI355X_NO_FUSION", SWITCH):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv(SWITCH, "1")
    for net in (mc.attention_block(dtype, layout),                     # K = 32 at 17 tokens: the chain form; p a graph output
                attention_net(dtype, layout, second_consumer=True)):   # the scaled scores are read twice
        sess = net.build(fe, pkg.API_MI355X)
        assert opt.shl_mi355x_session_is_device_resident(sess) == 2
        assert opt.shl_mi355x_session_fused_attentions(sess) == 0
        net.close(fe)
    monkeypatch.setenv("SHL_MI355X_NO_FUSION", "1")
    net = attention_net(dtype, layout)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_fused_attentions(sess) == 0
    net.close(fe)


@pytest.mark.gpu
def test_unasked_the_planner_merges_only_the_shapes_measured_faster(gpu, monkeypatch):
    """csrc/attention_canon.h:att_default -- heads of at most 32 on at least 768 keys (profiles/attention_notes.md); the nets are
    built and captured, not run"""
    fe, hip, opt = gpu
    for var in ("SHL_MI355X_HOST_SESSION", "SHL_MI355X_MATMUL_FORM", "SHL_MI355X_NO_FUSION", SWITCH):
        monkeypatch.delenv(var, raising=False)
    for kw, want in ((dict(), 0), (dict(tokens=768, hd=32), 1), (dict(tokens=767, hd=32), 0), (dict(tokens=768, hd=64), 0)):
        net = attention_net("int8", "NHWC", **kw)
        sess = net.build(fe, pkg.API_MI355X)
        assert opt.shl_mi355x_session_is_device_resident(sess) == 2
        assert opt.shl_mi355x_session_fused_attentions(sess) == want, kw
        net.close(fe)


# on 768 keys the 80-token net's constant of 64 x 2^-9 leaves the int8 probabilities nearly flat (the oracle chain: two to four
# distinct values a row); twice the constant gives rows of 4 to 8 and 70 distinct values in all
RECORDS_768 = {"scale": _q(2.0 ** -8, 0)}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", FORMATS)
def test_the_class_fused_unasked_runs_and_equals_the_layers_apart(gpu, dtype, layout, monkeypatch):
    """768 tokens on 2 heads of 32: what csrc/attention_canon.h:att_default fuses with SHL_MI355X_ATTENTION unset.  The session
    is one captured graph with one fused attention, and every run of it equals, bit for bit, the same net under
    SHL_MI355X_ATTENTION=0 -- and the net whose p is a graph output, which hands out the layers-apart probabilities.  The CPU
    oracle is not the arbiter here (P V's proof cannot hold on 768 keys under p's record, and the gate does not compose through
    the projection): test_attention_sweeps.py carries the CPU reference for this shape"""
    fe, hip, opt = gpu
    for var in ("SHL_MI355X_HOST_SESSION", "SHL_MI355X_MATMUL_FORM", "SHL_MI355X_NO_FUSION", SWITCH):
        monkeypatch.delenv(var, raising=False)
    kw = dict(tokens=768, hd=32, records=RECORDS_768)
    net = attention_net(dtype, layout, **kw)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    assert opt.shl_mi355x_session_fused_attentions(sess) == 1
    got = [net.run(fe, net.input(k)) for k in (0, 1, 0)]  # the graph replay reads fresh data
    assert not np.array_equal(mc.bits(got[0]["out"]), mc.bits(got[1]["out"])), "the two inputs must tell runs apart"
    monkeypatch.setenv(SWITCH, "0")
    apart = attention_net(dtype, layout, **kw)
    apart_sess = apart.build(fe, pkg.API_MI355X)
    monkeypatch.delenv(SWITCH)
    assert opt.shl_mi355x_session_is_device_resident(apart_sess) == 2
    assert opt.shl_mi355x_session_fused_attentions(apart_sess) == 0
    assert planner_counts(opt, sess) == planner_counts(opt, apart_sess)
    assert opt.shl_mi355x_session_fused_linears(sess) == opt.shl_mi355x_session_fused_linears(apart_sess)
    for k, g in zip((0, 1, 0), got):
        assert g["out"].shape == net.shape("out")
        mc.assert_same(apart.run(fe, apart.input(k))["out"], g["out"], "%s input %d: fused by default vs the layers apart" % (dtype, k))
    apart.close(fe)
    # p as a graph output keeps the layers apart whatever the switch says: the same output again, and the probabilities themselves
    shown = attention_net(dtype, layout, p_is_output=True, **kw)
    shown_sess = shown.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_fused_attentions(shown_sess) == 0
    res = shown.run(fe, shown.input(0))
    mc.assert_same(res["out"], got[0]["out"], dtype + ": fused by default vs the net whose p is a graph output")
    spread = np.unique(mc.bits(res["p"])).size
    assert spread > 8, "the layers-apart p holds %d different values: it would tell nothing" % spread
    shown.close(fe)
    net.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("moves", ["0", "1"])
def test_the_fused_step_survives_the_recapture_around_a_callers_hbm_buffer(gpu, moves, monkeypatch):
    """update_input with a device pointer rebinds the graph input, and the session captures its steps again from what the plan
    stored -- the core's descriptors and, with the moves folded, the layout's.  The int8 block runs on two inputs from host
    buffers, then on fresh copies of them from the caller's HBM buffer: the same bytes, and the oracle chain's"""
    fe, hip, opt = gpu
    for var in ("SHL_MI355X_HOST_SESSION", "SHL_MI355X_MATMUL_FORM", "SHL_MI355X_NO_FUSION"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.setenv("SHL_MI355X_ATTENTION_LAYOUT", moves)
    net = attention_net("int8", "NHWC")
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2
    assert opt.shl_mi355x_session_fused_attentions(sess) == 1
    assert opt.shl_mi355x_session_folded_head_moves(sess) == (8 if moves == "1" else 0)
    from_host = [net.run(fe, net.input(k))["out"] for k in (0, 1)]
    dev = cases.HipDevice(hip)
    d_in = dev.alloc(net.input(0).nbytes)
    scale, zp = net.rec("x")
    feed = pkg.make_tensor(fe, net._keep, net.shape("x"), pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, sess=sess, scales=(scale,), zps=(zp,), device_ptr=d_in)
    got = pkg.make_tensor(fe, net._keep, (1,), pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, sess=sess)
    for k in (1, 0):
        dev.upload(d_in, net.input(k))
        fe.csinn_update_input(0, feed, sess)
        assert fe.csinn_session_run(sess) == pkg.CSINN_TRUE  # (the first of them captures again)
        assert opt.shl_mi355x_session_is_device_resident(sess) == 2
        fe.csinn_get_output(0, got, sess)
        shape = net.shape("out")
        res = np.ctypeslib.as_array(C.cast(got.contents.data, C.POINTER(C.c_int8)), (int(np.prod(shape)),)).copy().reshape(shape)
        fe.shl_mem_free(got.contents.data)
        assert np.array_equal(res, from_host[k]), "input %d: from the caller's HBM buffer vs from a host buffer" % k
        assert np.array_equal(res, net.oracle(net.input(k))["out"]), "input %d: the output differs from the oracle chain" % k
    assert not np.array_equal(from_host[0], from_host[1]), "the two inputs must tell runs apart"
    dev.free(d_in)
    net.close(fe)


DROPIN = r"""
import os
import sys
os.environ["SHL_MI355X_ATTENTION"] = "1"
sys.path.insert(0, %(tests)r)
import numpy as np
import cases, matmul_cases as mc
from cases import pkg
from test_attention_session import attention_net
fe = cases.load_reference_frontend()          # genuine libshl_ref_x86.so: its own gref builds the graph
hip, opt = pkg.load_backend(fe)
bad = 0
for dtype, layout in (("int8", "NHWC"), ("f16", "NCHW")):
    net = attention_net(dtype, layout)
    sess = net.build(fe, pkg.API_MI355X)
    mode, fused = opt.shl_mi355x_session_is_device_resident(sess), opt.shl_mi355x_session_fused_attentions(sess)
    for k in range(2):
        x = net.input(k)
        w, g = net.oracle(x)["out"], net.run(fe, x)["out"]
        if dtype == "int8":
            ok = bool(np.array_equal(g, w))
        else:
            ok = bool(np.all(np.abs(g.astype(np.float32) - w.astype(np.float32)) <= 1e-3 * np.maximum(np.abs(w.astype(np.float32)), 1e-3)))
        print(dtype, layout, "input", k, "device mode", mode, "fused attentions", fused, "ok", ok)
        bad += int(not ok) + int(mode != 2) + int(fused != 1)
print("ATTENTIONNET_OK" if bad == 0 else "ATTENTIONNET_FAIL")
"""


@pytest.mark.gpu
@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_block_drops_in_behind_the_genuine_graph_executor(gpu):
    """The reference's own gref records the layers; the backend's planner merges the four core layers there as well."""
    code = DROPIN % dict(tests=os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "ATTENTIONNET_OK" in res.stdout, res.stdout + res.stderr

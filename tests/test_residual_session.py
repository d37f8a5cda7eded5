"""The fused residual tail inside a session (-m gpu; tests/residual_nets.py): a ResNet basic block, a MobileNetV2
inverted-residual block and a bottleneck whose add follows the projection shortcut's convolution each run, under
SHL_MI355X_RESIDUAL=1, as one hipGraph with ONE fused tail (shl_mi355x_session_fused_residuals == 1), match the oracle chain and
the genuine library's outputs (tests/golden/residual_nets.npz) byte for byte and equal the same net built under
SHL_MI355X_RESIDUAL=0; the other planner counters do not move.  A convolution output with two consumers, a broadcast add and
NCHW / binary16 copies of the basic block keep their layers apart, and so does SHL_MI355X_NO_FUSION=1."""
import os

import numpy as np
import pytest

import residual_cases
import residual_nets as rn
from cases import pkg
from test_concat_session import matches, planner_counts

SWITCH = "SHL_MI355X_RESIDUAL"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "residual_nets.npz")


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt


def _clean(monkeypatch):
    for var in ("SHL_MI355X_HOST_SESSION", "SHL_MI355X_NO_FUSION", "SHL_MI355X_RESIDUAL_FORM", "SHL_MI355X_IGEMM", SWITCH):
        monkeypatch.delenv(var, raising=False)


def counters(opt, sess):
    return planner_counts(opt, sess) + (opt.shl_mi355x_session_fused_linears(sess), opt.shl_mi355x_session_fused_attentions(sess))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(rn.FUSING))
def test_block_runs_as_one_hipgraph_with_one_fused_tail(gpu, name, monkeypatch):
    fe, hip, opt = gpu
    _clean(monkeypatch)
    golden = np.load(GOLDEN)
    monkeypatch.setenv(SWITCH, "1")
    net = rn.FUSING[name]()
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    assert opt.shl_mi355x_session_fused_residuals(sess) == 1
    want = {k: net.oracle(net.input(k))["out"] for k in (0, 1)}
    got = [net.run(fe, net.input(k))["out"] for k in (0, 1, 0)]  # the graph replay reads fresh data
    for k, g in zip((0, 1, 0), got):
        assert np.array_equal(g, want[k]), "%s input %d: the output differs from the oracle chain" % (name, k)
        assert np.array_equal(g, golden["%s_%d" % (name, k)]), "%s input %d: the output differs from the genuine library's" % (name, k)
    assert not np.array_equal(want[0], want[1]) and np.unique(want[0]).size > 8
    monkeypatch.setenv(SWITCH, "0")
    apart = rn.FUSING[name]()
    apart_sess = apart.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(apart_sess) == 2
    assert opt.shl_mi355x_session_fused_residuals(apart_sess) == 0
    assert counters(opt, sess) == counters(opt, apart_sess)
    for k, g in zip((0, 1, 0), got):
        assert np.array_equal(apart.run(fe, apart.input(k))["out"], g), "%s input %d: fused vs the layers apart" % (name, k)
    apart.close(fe)
    net.close(fe)
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.setenv("SHL_MI355X_NO_FUSION", "1")
    plain = rn.FUSING[name]()
    assert opt.shl_mi355x_session_fused_residuals(plain.build(fe, pkg.API_MI355X)) == 0
    plain.close(fe)


@pytest.mark.gpu
def test_unasked_only_measured_shape_classes_fuse(gpu, monkeypatch):
    """what the planner does by default is what shl_mi355x_conv_add_by_default says of the convolution's plan"""
    fe, hip, opt = gpu
    _clean(monkeypatch)
    net = rn.basic_block()
    sess = net.build(fe, pkg.API_MI355X)
    plan = residual_cases.make_plan(hip, net.cv["conv"])
    assert opt.shl_mi355x_session_fused_residuals(sess) == hip.shl_mi355x_conv_add_by_default(plan, 1)
    hip.shl_mi355x_conv_plan_destroy(plan)
    assert np.array_equal(net.run(fe, net.input(0))["out"], net.oracle(net.input(0))["out"])
    net.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["two_consumers", "broadcast", "nchw", "f16"])
def test_nets_outside_the_scope_keep_their_layers(gpu, which, monkeypatch):
    fe, hip, opt = gpu
    _clean(monkeypatch)
    monkeypatch.setenv(SWITCH, "1")
    dtype = "f16" if which == "f16" else "int8"
    net = {"two_consumers": lambda: rn.basic_block(export_conv=True), "broadcast": rn.broadcast_block,
           "nchw": lambda: rn.basic_block("int8", "NCHW"), "f16": lambda: rn.basic_block("f16", "NCHW")}[which]()
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2
    assert opt.shl_mi355x_session_fused_residuals(sess) == 0
    for k in (0, 1):
        x = net.input(k)
        want = net.oracle(x, getattr(net, "consts", None))
        got = net.run(fe, x)
        for out in net.outputs:
            assert matches(got[out], want[out], dtype), "%s input %d: %s differs from the oracle chain" % (which, k, out)
    net.close(fe)

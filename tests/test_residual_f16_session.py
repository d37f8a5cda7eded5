"""The binary16 fused residual tail inside a session (-m gpu; tests/residual_f16_nets.py): a ResNet basic block, a bottleneck
tail, a MobileNetV2 inverted-residual block and a bottleneck whose add follows the projection shortcut's convolution, all
binary16 NHWC, each run under SHL_MI355X_RESIDUAL=1 as one hipGraph with ONE fused tail (shl_mi355x_session_fused_residuals
== 1), equal the same net built under SHL_MI355X_RESIDUAL=0 bit for bit and match the oracle chain within the sessions' binary16
tolerance; the other planner counters do not move.  Unasked, the planner does what shl_mi355x_conv_add_f16_by_default says.  A
convolution output with two consumers, a broadcast add and the NCHW copy keep their layers apart, and so does
SHL_MI355X_NO_FUSION=1."""
import numpy as np
import pytest

import residual_f16_cases
import residual_f16_nets as fn
from cases import pkg
from test_concat_session import matches, planner_counts

SWITCH = "SHL_MI355X_RESIDUAL"


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(fn.FUSING))
def test_block_runs_as_one_hipgraph_with_one_fused_tail(gpu, name, monkeypatch):
    fe, hip, opt = gpu
    _clean(monkeypatch)
    make = fn.FUSING[name][0]
    monkeypatch.setenv(SWITCH, "1")
    net = make()
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    assert opt.shl_mi355x_session_fused_residuals(sess) == 1
    want = {k: net.oracle(net.input(k))["out"] for k in (0, 1)}
    got = [net.run(fe, net.input(k))["out"] for k in (0, 1, 0)]  # the graph replay reads fresh data
    for k, g in zip((0, 1, 0), got):
        assert matches(g, want[k], "f16"), "%s input %d: the output differs from the oracle chain" % (name, k)
    assert not np.array_equal(want[0], want[1]) and np.unique(want[0]).size > 8
    monkeypatch.setenv(SWITCH, "0")
    apart = make()
    apart_sess = apart.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(apart_sess) == 2
    assert opt.shl_mi355x_session_fused_residuals(apart_sess) == 0
    assert counters(opt, sess) == counters(opt, apart_sess)
    for k, g in zip((0, 1, 0), got):
        assert np.array_equal(bits(apart.run(fe, apart.input(k))["out"]), bits(g)), "%s input %d: fused vs the layers apart" % (name, k)
    apart.close(fe)
    net.close(fe)
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.setenv("SHL_MI355X_NO_FUSION", "1")
    plain = make()
    assert opt.shl_mi355x_session_fused_residuals(plain.build(fe, pkg.API_MI355X)) == 0
    plain.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(fn.FUSING))
def test_unasked_only_measured_shape_classes_fuse(gpu, name, monkeypatch):
    """what the planner does by default is what shl_mi355x_conv_add_f16_by_default says of the convolution's plan"""
    fe, hip, opt = gpu
    _clean(monkeypatch)
    make, conv = fn.FUSING[name]
    net = make()
    sess = net.build(fe, pkg.API_MI355X)
    plan = residual_f16_cases.make_plan(hip, net.cv[conv])
    assert opt.shl_mi355x_session_fused_residuals(sess) == hip.shl_mi355x_conv_add_f16_by_default(plan, 1)
    hip.shl_mi355x_conv_plan_destroy(plan)
    assert matches(net.run(fe, net.input(0))["out"], net.oracle(net.input(0))["out"], "f16")
    net.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["two_consumers", "broadcast", "nchw"])
def test_nets_outside_the_scope_keep_their_layers(gpu, which, monkeypatch):
    fe, hip, opt = gpu
    _clean(monkeypatch)
    monkeypatch.setenv(SWITCH, "1")
    net = {"two_consumers": lambda: fn.basic_block(export_conv=True), "broadcast": fn.broadcast_block,
           "nchw": lambda: fn.basic_block("NCHW")}[which]()
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2
    assert opt.shl_mi355x_session_fused_residuals(sess) == 0
    for k in (0, 1):
        x = net.input(k)
        want = net.oracle(x, getattr(net, "consts", None))
        got = net.run(fe, x)
        for out in net.outputs:
            assert matches(got[out], want[out], "f16"), "%s input %d: %s differs from the oracle chain" % (which, k, out)
    net.close(fe)

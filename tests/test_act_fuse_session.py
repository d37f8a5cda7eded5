"""Table activations folded into their convolutions inside a session (-m gpu; tests/act_fuse_cases.py): a YOLO-style stack
(3x3 s2 conv -> silu -> 1x1 conv -> leaky_relu -> 3x3 conv -> silu -> add(skip)) and a MobileNetV3-style block (1x1 expand ->
hard_sigmoid -> mul -> depthwise 3x3 -> 1x1 project -> sigmoid -> mul, the convolution's output on either side of the mul)
each run as one hipGraph under SHL_MI355X_ACT_FUSE=1, =0 and unset: the outputs are equal byte for byte across the three and
equal to the oracle replay, shl_mi355x_session_fused_activations is 3 and 2 under =1 and 0 under =0 and under
SHL_MI355X_NO_FUSION=1, and the other planner counters do not move.  An intermediate tensor that is a graph output too, a
convolution output with a third reader and a broadcasting mul keep their layers apart."""
import numpy as np
import pytest

import act_fuse_cases as ac
from cases import pkg
from test_concat_session import planner_counts

SWITCH = "SHL_MI355X_ACT_FUSE"


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt


def _clean(monkeypatch):
    for var in ("SHL_MI355X_HOST_SESSION", "SHL_MI355X_NO_FUSION", "SHL_MI355X_ACT_FORM", "SHL_MI355X_IGEMM", "SHL_MI355X_RESIDUAL", SWITCH):
        monkeypatch.delenv(var, raising=False)


def counters(opt, sess):
    return planner_counts(opt, sess) + (opt.shl_mi355x_session_fused_linears(sess), opt.shl_mi355x_session_fused_attentions(sess),
                                        opt.shl_mi355x_session_fused_residuals(sess))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ac.FUSING))
def test_net_runs_as_one_hipgraph_with_its_activations_fused(gpu, name, monkeypatch):
    fe, hip, opt = gpu
    _clean(monkeypatch)
    make, expected = ac.FUSING[name]
    runs = {}
    for setting in ("1", "0", None):
        if setting is None:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, setting)
        net = make()
        sess = net.build(fe, pkg.API_MI355X)
        assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
        fused = opt.shl_mi355x_session_fused_activations(sess)
        if setting == "1":
            assert fused == expected
        elif setting == "0":
            assert fused == 0
        else:
            assert 0 <= fused <= expected
        runs[setting] = (counters(opt, sess), [net.run(fe, net.input(k))["out"] for k in (0, 1, 0)])  # the replay reads fresh data
        net.close(fe)
    net = make()
    want = {k: net.oracle(net.input(k))["out"] for k in (0, 1)}
    assert not np.array_equal(want[0], want[1]) and np.unique(want[0]).size > 8
    for setting, (counts, got) in runs.items():
        assert counts == runs["0"][0], "SHL_MI355X_ACT_FUSE=%s moved another planner counter" % setting
        for k, g in zip((0, 1, 0), got):
            assert np.array_equal(g, want[k]), "%s under %s=%s, input %d: the output differs from the oracle chain" % (name, SWITCH, setting, k)
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.setenv("SHL_MI355X_NO_FUSION", "1")
    plain = make()
    assert opt.shl_mi355x_session_fused_activations(plain.build(fe, pkg.API_MI355X)) == 0
    assert np.array_equal(plain.run(fe, plain.input(1))["out"], want[1])
    plain.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(ac.APART))
def test_nets_outside_the_patterns_keep_their_layers(gpu, which, monkeypatch):
    fe, hip, opt = gpu
    _clean(monkeypatch)
    monkeypatch.setenv(SWITCH, "1")
    net = ac.APART[which]()
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2
    assert opt.shl_mi355x_session_fused_activations(sess) == 0
    for k in (0, 1):
        x = net.input(k)
        want, got = net.oracle(x), net.run(fe, x)
        for out in net.outputs:
            assert np.array_equal(got[out], want[out]), "%s input %d: %s differs from the oracle chain" % (which, k, out)
    net.close(fe)

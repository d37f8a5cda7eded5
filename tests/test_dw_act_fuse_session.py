"""Table activations folded into their DEPTHWISE layers inside a session (-m gpu; tests/dw_act_cases.py): a MobileNetV3 block
(1x1 expand -> hard_sigmoid -> mul -> depthwise 3x3 -> hard_sigmoid -> mul(gate, dw) -> 1x1 project -> add(skip)) and an
EfficientNet block (1x1 -> silu -> depthwise 5x5 stride 2 -> silu -> 1x1) each run as one hipGraph under SHL_MI355X_ACT_FUSE=1,
=0 and unset: the outputs are equal byte for byte across the three and equal to the oracle replay, and
shl_mi355x_session_fused_activations under =1 is 2 in both -- 1 from the expand convolution's implicit-GEMM step, as before, and
1 more from the depthwise step -- and 0 under =0; the other planner counters do not move.  A depthwise output that is a graph
output too, has a third reader, is gated through a broadcasting mul (an SE gate) or belongs to a pw -> dw pair keeps its
activation apart."""
import numpy as np
import pytest

import dw_act_cases as dc
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
    for var in ("SHL_MI355X_HOST_SESSION", "SHL_MI355X_NO_FUSION", "SHL_MI355X_ACT_FORM", "SHL_MI355X_IGEMM", "SHL_MI355X_RESIDUAL",
                "SHL_MI355X_PWDW", "SHL_MI355X_DWMFMA", SWITCH):
        monkeypatch.delenv(var, raising=False)


def counters(opt, sess):
    return planner_counts(opt, sess) + (opt.shl_mi355x_session_fused_linears(sess), opt.shl_mi355x_session_fused_attentions(sess),
                                        opt.shl_mi355x_session_fused_residuals(sess))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(dc.FUSING))
def test_block_runs_as_one_hipgraph_with_its_depthwise_activation_fused(gpu, name, monkeypatch):
    fe, hip, opt = gpu
    _clean(monkeypatch)
    make, expected, igemm_alone = dc.FUSING[name]
    assert (expected, igemm_alone) == (2, 1)  # the expand convolution's activation, and the depthwise layer's on top of it
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
            assert fused == expected and fused - igemm_alone == 1
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


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(dc.APART))
def test_nets_outside_the_patterns_keep_their_layers(gpu, which, monkeypatch):
    fe, hip, opt = gpu
    _clean(monkeypatch)
    monkeypatch.setenv(SWITCH, "1")
    net = dc.APART[which]()
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2
    assert opt.shl_mi355x_session_fused_activations(sess) == 0
    for k in (0, 1):
        x = net.input(k)
        want, got = net.oracle(x), net.run(fe, x)
        for out in net.outputs:
            assert np.array_equal(got[out], want[out]), "%s input %d: %s differs from the oracle chain" % (which, k, out)
    net.close(fe)


@pytest.mark.gpu
def test_depthwise_layer_that_is_half_of_a_pair_is_no_candidate(gpu, monkeypatch):
    """pw -> dw -> silu: the pair merge comes first, the activation stays a launch of its own"""
    fe, hip, opt = gpu
    _clean(monkeypatch)
    monkeypatch.setenv(SWITCH, "1")
    net = dc.paired_dw()
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_fused_pairs(sess) == 1 and opt.shl_mi355x_session_fused_activations(sess) == 0
    x = net.input(0)
    want = net.oracle(x)["out"]
    assert np.array_equal(net.run(fe, x)["out"], want)
    net.close(fe)

"""The reductions inside a session (-m gpu): a TensorFlow-style squeeze-and-excite block (mean over H and W), a CBAM block
(global_maxpool2d next to global_avgpool2d, max and mean over the channel axis) and a ReID tail (global_maxpool2d -> flatten ->
fullyconnected, reduce_max over the classes as a second output) from reduce_cases.py stay device-resident, are captured as one
hipGraph and match the oracle chain (convolutions and fullyconnected through the C oracle, the reductions through the numpy
restatement): int8 bit for bit, binary16 within 1e-3.  The fusion planner takes the same decisions as on the same graph
without the reduction layers.  Also behind the genuine front-end and graph executor."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import reduce_cases as rc
from cases import pkg
from test_concat_session import matches, planner_counts

FORMATS = [("int8", "NHWC"), ("f16", "NCHW")]


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", FORMATS)
@pytest.mark.parametrize("which", sorted(rc.NETS))
def test_network_runs_as_one_hipgraph_and_matches_the_oracle_chain(gpu, which, dtype, layout, monkeypatch):
    fe, hip, opt = gpu
    monkeypatch.delenv("SHL_MI355X_HOST_SESSION", raising=False)
    monkeypatch.delenv("SHL_MI355X_REDUCE_FORM", raising=False)
    net = rc.NETS[which](dtype, layout)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    want = {k: net.oracle(net.input(k)) for k in (0, 1)}
    for k in (0, 1, 0):  # the graph replay reads fresh data
        got = net.run(fe, net.input(k))
        for name in net.outputs:
            assert got[name].shape == want[k][name].shape
            assert matches(got[name], want[k][name], dtype), "%s %s %s input %d: output %s differs from the oracle chain" % (
                which, dtype, layout, k, name)
    for name in net.outputs:
        assert not np.array_equal(want[0][name], want[1][name]), "the two inputs must tell runs apart"
    # what the planner folds and fuses is what it folds and fuses in the same graph without the reduction layers (each one's
    # input a graph output, its output a graph input): they neither hide a consumer nor add one
    bare = rc.NETS[which](dtype, layout, cut=True)
    bare_sess = bare.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(bare_sess) >= 1
    assert bare.layer_count == net.layer_count - rc.CUT_LAYERS[which]
    want_counts = planner_counts(opt, bare_sess)
    assert want_counts[0] >= 1, "the graph holds a conv -> relu pair that folds"
    assert planner_counts(opt, sess) == want_counts
    bare.close(fe)
    net.close(fe)


DROPIN = r"""
import sys
sys.path.insert(0, %(tests)r)
import numpy as np
import cases, reduce_cases as rc
from cases import pkg
fe = cases.load_reference_frontend()          # genuine libshl_ref_x86.so: its own gref builds the graph
hip, opt = pkg.load_backend(fe)
bad = 0
for which in sorted(rc.NETS):
    for dtype, layout in (("int8", "NHWC"), ("f16", "NCHW")):
        net = rc.NETS[which](dtype, layout)
        sess = net.build(fe, pkg.API_MI355X)
        mode = opt.shl_mi355x_session_is_device_resident(sess)
        for k in range(2):
            x = net.input(k)
            want, got = net.oracle(x), net.run(fe, x)
            for name in net.outputs:
                g, w = got[name], want[name]
                if dtype == "int8":
                    ok = bool(np.array_equal(g, w))
                else:
                    ok = bool(np.all(np.abs(g.astype(np.float32) - w.astype(np.float32)) <= 1e-3 * np.maximum(np.abs(w.astype(np.float32)), 1e-3)))
                print(which, dtype, layout, "input", k, "output", name, "device mode", mode, "ok", ok)
                bad += int(not ok) + int(mode != 2)
print("REDUCENETS_OK" if bad == 0 else "REDUCENETS_FAIL")
"""


@pytest.mark.gpu
@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_networks_drop_in_behind_the_genuine_graph_executor(gpu):
    """The reference's csinn_mean / _max / _reduce_max / _global_maxpool2d and its gref record the layers; the backend's
    callbacks run them device-resident (one that fell through to the C reference would drop the whole session to the host
    path: mode 0)."""
    code = DROPIN % dict(tests=os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "REDUCENETS_OK" in res.stdout, res.stdout + res.stderr

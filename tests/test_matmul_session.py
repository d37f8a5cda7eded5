"""matmul inside a session (-m gpu): an attention block (S = 17 tokens, 2 heads of 32, C = 64: three matmuls against constant
weights, reshape / transpose to heads, matmul(q, k, trans_b), mul by a constant scale, softmax over the last axis of the 4-d
scores -- which the softmax kernel takes as it is, no transpose around it --, matmul(p, v), transpose / reshape back, a matmul
against a constant, add of the residual) and a conv -> flatten -> matmul classifier tail from matmul_cases.py stay
device-resident, are captured as one hipGraph and match the oracle chain (matmul through chain_ref, the other layers through
their existing oracles): int8 bit for bit -- every matmul's records lie inside the plan-time proof --, binary16 within 1e-3.
The fusion planner takes the same decisions as on the same graph without the matmul layers.  Also behind the genuine front-end
and graph executor."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import matmul_cases as mc
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
@pytest.mark.parametrize("which", sorted(mc.NETS))
def test_network_runs_as_one_hipgraph_and_matches_the_oracle_chain(gpu, which, dtype, layout, monkeypatch):
    fe, hip, opt = gpu
    monkeypatch.delenv("SHL_MI355X_HOST_SESSION", raising=False)
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM", raising=False)
    net = mc.NETS[which](dtype, layout)
    if dtype == "int8":  # the comparison is bit for bit because the proof holds for every matmul the mfma form takes
        for kind, name, src, dst, info in net.layers:
            if kind == "matmul":
                case = net._matmul_case(src, dst, info, a=np.zeros(net.shape(src[0]), np.int8),
                                        b=np.zeros(net.shape(src[1]), np.int8) if src[1] not in net.consts else None)
                k = case["a"].shape[-2 if case["trans_a"] else -1]
                assert mc.is_exact(dict(case, k=k)), name
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
        spread = np.unique(mc.bits(want[0][name])).size
        assert spread > 8, "output %s of the oracle chain holds %d different values: it would tell nothing" % (name, spread)
    # what the planner folds and fuses is what it folds and fuses in the same graph without the matmul layers (each one's
    # activation inputs graph outputs, its output a graph input): they neither hide a consumer nor add one
    bare = mc.NETS[which](dtype, layout, cut=True)
    bare_sess = bare.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(bare_sess) >= 1
    assert bare.layer_count == net.layer_count - mc.CUT_LAYERS[which]
    want_counts = planner_counts(opt, bare_sess)
    if which == "classifier_tail":
        assert want_counts[0] >= 1, "the graph holds a conv -> relu pair that folds"
    assert planner_counts(opt, sess) == want_counts
    bare.close(fe)
    net.close(fe)


DROPIN = r"""
import sys
sys.path.insert(0, %(tests)r)
import numpy as np
import cases, matmul_cases as mc
from cases import pkg
fe = cases.load_reference_frontend()          # genuine libshl_ref_x86.so: its own gref builds the graph
hip, opt = pkg.load_backend(fe)
bad = 0
for which in sorted(mc.NETS):
    for dtype, layout in (("int8", "NHWC"), ("f16", "NCHW")):
        net = mc.NETS[which](dtype, layout)
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
print("MATMULNETS_OK" if bad == 0 else "MATMULNETS_FAIL")
"""


@pytest.mark.gpu
@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_networks_drop_in_behind_the_genuine_graph_executor(gpu):
    """The reference's csinn_matmul and its gref record the layers; the backend's callbacks run them device-resident (one that
    fell through to the C reference would drop the whole session to the host path: mode 0)."""
    code = DROPIN % dict(tests=os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "MATMULNETS_OK" in res.stdout, res.stdout + res.stderr

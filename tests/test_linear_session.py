"""Linear layers inside a session (-m gpu): an MLP and an attention block with biases (linear_cases.py) -- MatMul against a
constant followed by Add of a constant bias, the bias given second or first, an attention bias on the scores, hard-swish --
stay device-resident, are captured as one hipGraph and match the oracle chain: int8 bit for bit (every matmul's records lie
inside the plan-time proof), binary16 within 1e-3.  Each matmul + bias pair runs as ONE launch (session_fused_linears);
SHL_MI355X_NO_FUSION=1 keeps them apart and gives the same bits.  Also behind the genuine front-end and graph executor."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import linear_cases as lc
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


@pytest.fixture(scope="module")
def oracle():
    """the oracle chain of each (network, format, input), computed once"""
    memo = {}

    def get(which, dtype, layout, k):
        key = (which, dtype, layout, k)
        if key not in memo:
            net = lc.NETS[which](dtype, layout)
            memo[key] = net.oracle(net.input(k))
        return memo[key]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", FORMATS)
@pytest.mark.parametrize("which", sorted(lc.NETS))
def test_network_runs_as_one_hipgraph_with_fused_linears_and_matches_the_oracle_chain(gpu, oracle, which, dtype, layout, monkeypatch):
    fe, hip, opt = gpu
    for name in ("SHL_MI355X_HOST_SESSION", "SHL_MI355X_MATMUL_FORM", "SHL_MI355X_ADD_FORM", "SHL_MI355X_NO_FUSION"):
        monkeypatch.delenv(name, raising=False)
    net = lc.NETS[which](dtype, layout)
    if dtype == "int8":  # the comparison is bit for bit because the proof holds for every matmul the mfma form takes
        for kind, name, src, dst, info in net.layers:
            if kind == "matmul":
                case = net._matmul_case(src, dst, info, a=np.zeros(net.shape(src[0]), np.int8),
                                        b=np.zeros(net.shape(src[1]), np.int8) if src[1] not in net.consts else None)
                k = case["a"].shape[-2 if case["trans_a"] else -1]
                assert mc.is_exact(dict(case, k=k)), name
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    assert opt.shl_mi355x_session_fused_linears(sess) == lc.FUSED_LINEARS[which]
    want = {k: oracle(which, dtype, layout, k) for k in (0, 1)}
    fused = {}
    for k in (0, 1, 0):  # the graph replay reads fresh data
        got = fused[k] = net.run(fe, net.input(k))
        for name in net.outputs:
            assert got[name].shape == want[k][name].shape
            assert matches(got[name], want[k][name], dtype), "%s %s %s input %d: output %s differs from the oracle chain" % (
                which, dtype, layout, k, name)
    for name in net.outputs:
        assert not np.array_equal(want[0][name], want[1][name]), "the two inputs must tell runs apart"
        assert not np.array_equal(mc.bits(fused[0][name]), mc.bits(fused[1][name]))
        spread = np.unique(mc.bits(want[0][name])).size
        assert spread > 8, "output %s of the oracle chain holds %d different values: it would tell nothing" % (name, spread)
    counts = planner_counts(opt, sess)
    net.close(fe)
    # the same graph without the fusion: no fused linear, the same bits in both dtypes, the other counters unchanged
    monkeypatch.setenv("SHL_MI355X_NO_FUSION", "1")
    bare = lc.NETS[which](dtype, layout)
    bare_sess = bare.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(bare_sess) == 2
    assert opt.shl_mi355x_session_fused_linears(bare_sess) == 0
    assert planner_counts(opt, bare_sess) == counts
    for k in (0, 1):
        got = bare.run(fe, bare.input(k))
        for name in bare.outputs:
            mc.assert_same(got[name], fused[k][name], "%s %s input %d output %s: unfused vs fused" % (which, dtype, k, name))
    bare.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", FORMATS)
@pytest.mark.parametrize("which", sorted(mc.NETS))
def test_a_residual_add_is_no_fused_linear(gpu, which, dtype, layout, monkeypatch):
    """matmul_cases' networks end a matmul in an add of two ACTIVATIONS (or in nothing): nothing to fuse, counters as before"""
    fe, hip, opt = gpu
    monkeypatch.delenv("SHL_MI355X_NO_FUSION", raising=False)
    net = mc.NETS[which](dtype, layout)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2
    assert opt.shl_mi355x_session_fused_linears(sess) == 0
    net.close(fe)


DROPIN = r"""
import sys
sys.path.insert(0, %(tests)r)
import numpy as np
import cases, linear_cases as lc
from cases import pkg
fe = cases.load_reference_frontend()          # genuine libshl_ref_x86.so: its own gref builds the graph
hip, opt = pkg.load_backend(fe)
bad = 0
for which in sorted(lc.NETS):
    for dtype, layout in (("int8", "NHWC"), ("f16", "NCHW")):
        net = lc.NETS[which](dtype, layout)
        sess = net.build(fe, pkg.API_MI355X)
        mode, linears = opt.shl_mi355x_session_is_device_resident(sess), opt.shl_mi355x_session_fused_linears(sess)
        x = net.input(0)
        want, got = net.oracle(x), net.run(fe, x)
        for name in net.outputs:
            g, w = got[name], want[name]
            if dtype == "int8":
                ok = bool(np.array_equal(g, w))
            else:
                ok = bool(np.all(np.abs(g.astype(np.float32) - w.astype(np.float32)) <= 1e-3 * np.maximum(np.abs(w.astype(np.float32)), 1e-3)))
            print(which, dtype, layout, "output", name, "device mode", mode, "fused linears", linears, "ok", ok)
            bad += int(not ok) + int(mode != 2) + int(linears != lc.FUSED_LINEARS[which])
print("LINEARNETS_OK" if bad == 0 else "LINEARNETS_FAIL")
"""


@pytest.mark.gpu
@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_networks_drop_in_behind_the_genuine_graph_executor(gpu):
    """The reference's csinn_matmul / csinn_add and its gref record the layers; the backend's callbacks run them
    device-resident (a broadcasting add that fell through to the C reference would drop the whole session to the host path:
    mode 0), and the planner fuses the same pairs."""
    code = DROPIN % dict(tests=os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "LINEARNETS_OK" in res.stdout, res.stdout + res.stderr

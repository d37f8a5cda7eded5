"""Concat inside a session (-m gpu): BranchNet (concat_cases.py) -- a Fire module and an Inception block of four branches,
each ending in a concat -- stays device-resident, is captured as one hipGraph, and matches the oracle chain (convolutions
through the C oracle, pools and concat through the numpy restatements): int8 bit for bit, binary16 within 1e-3.  The
fusion planner takes the same decisions as on the same graph without its concats.  Also with a constant concat input,
and behind the genuine front-end and graph executor."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import concat_cases
from cases import pkg


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt


def matches(got, want, dtype):
    if dtype == "int8":
        return np.array_equal(got, want)
    g, w = got.astype(np.float32), want.astype(np.float32)
    return bool(np.all(np.abs(g - w) <= 1e-3 * np.maximum(np.abs(w), 1e-3)))


def planner_counts(opt, sess):
    return (opt.shl_mi355x_session_folded_activations(sess), opt.shl_mi355x_session_fused_pairs(sess),
            opt.shl_mi355x_session_fused_pools(sess))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", [("int8", "NHWC"), ("f16", "NCHW")])
def test_branchnet_runs_device_resident_and_matches_the_oracle_chain(gpu, dtype, layout):
    fe, hip, opt = gpu
    net = concat_cases.BranchNet(dtype, layout)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    for k in (0, 1, 0):  # the graph replay reads fresh data
        x = net.input(k)
        got, want = net.run(fe, x), net.oracle(x)
        assert got.shape == want.shape
        assert matches(got, want, dtype), "BranchNet %s %s input %d differs from the oracle chain" % (dtype, layout, k)
    assert not np.array_equal(net.oracle(net.input(0)), net.oracle(net.input(1))), "the two inputs must tell runs apart"
    # what the planner folds and fuses is what it folds and fuses in the same graph without its concats (every concat
    # input a graph output, every concat output a graph input): a concat neither hides a consumer nor adds one
    bare = concat_cases.BranchNet(dtype, layout, concats=False)
    bare_sess = bare.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(bare_sess) >= 1
    assert bare.layer_count == net.layer_count - 2
    want_counts = planner_counts(opt, bare_sess)
    assert want_counts[0] >= 1, "the graph holds a conv -> relu pair that folds"
    assert planner_counts(opt, sess) == want_counts
    bare.close(fe)
    net.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", [("int8", "NHWC"), ("f16", "NCHW")])
def test_a_constant_concat_input_is_uploaded_once_and_matches_the_oracle(gpu, dtype, layout):
    fe, hip, opt = gpu
    net = concat_cases.BranchNet(dtype, layout, const_input=True)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2
    for k in (0, 1, 0):
        x = net.input(k)
        assert matches(net.run(fe, x), net.oracle(x), dtype), "input %d differs from the oracle chain" % k
    # the constant matters: the oracle without it gives another answer
    other = concat_cases.BranchNet(dtype, layout, const_input=True)
    other.konst = np.zeros_like(other.konst)
    assert not np.array_equal(other.oracle(net.input(0)), net.oracle(net.input(0)))
    net.close(fe)


DROPIN = r"""
import sys
sys.path.insert(0, %(tests)r)
import numpy as np
import cases, concat_cases
from cases import pkg
fe = cases.load_reference_frontend()          # genuine libshl_ref_x86.so: its own gref builds the graph
hip, opt = pkg.load_backend(fe)
bad = 0
for dtype, layout in (("int8", "NHWC"), ("f16", "NCHW")):
    net = concat_cases.BranchNet(dtype, layout); sess = net.build(fe, pkg.API_MI355X)
    mode = opt.shl_mi355x_session_is_device_resident(sess)
    for k in range(2):
        x = net.input(k)
        want, got = net.oracle(x), net.run(fe, x)
        if dtype == "int8":
            ok = bool(np.array_equal(got, want))
        else:
            ok = bool(np.all(np.abs(got.astype(np.float32) - want.astype(np.float32)) <= 1e-3 * np.maximum(np.abs(want.astype(np.float32)), 1e-3)))
        print(dtype, layout, "input", k, "device mode", mode, "ok", ok)
        bad += int(not ok) + int(mode != 2)
print("BRANCHNET_OK" if bad == 0 else "BRANCHNET_FAIL")
"""


@pytest.mark.gpu
@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_branchnet_drop_in_behind_the_genuine_graph_executor(gpu):
    """The reference's csinn_concat and its gref record the layers; the backend's callback runs them device-resident (a
    concat that fell through to the C reference would drop the whole session to the host path: mode 0)."""
    code = DROPIN % dict(tests=os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "BRANCHNET_OK" in res.stdout, res.stdout + res.stderr

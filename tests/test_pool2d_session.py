"""Windowed pools inside a session (-m gpu): PoolNet (pool_cases.py) -- ResNet's stem pool, a residual block whose
shortcut is the pooled tensor, an average pool -- stays device-resident, is captured as one hipGraph, and matches
the oracle chain (convolutions through the C oracle, pools through the numpy restatement): int8 bit for bit,
binary16 within 1e-3.  Also behind the genuine front-end and graph executor."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import pool_cases
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


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", [("int8", "NHWC"), ("f16", "NCHW")])
def test_poolnet_runs_device_resident_and_matches_the_oracle_chain(gpu, dtype, layout):
    fe, hip, opt = gpu
    net = pool_cases.PoolNet(dtype, layout)
    sess = net.build(fe, pkg.API_MI355X)
    mode = opt.shl_mi355x_session_is_device_resident(sess)
    assert mode >= 1, "the session fell back to the host path"
    assert mode == 2, "the session was not captured as a hipGraph"
    for k in (0, 1, 0):  # the graph replay reads fresh data
        x = net.input(k)
        got, want = net.run(fe, x), net.oracle(x)
        assert got.shape == want.shape
        assert matches(got, want, dtype), "PoolNet %s %s input %d differs from the oracle chain" % (dtype, layout, k)
    assert not np.array_equal(net.oracle(net.input(0)), net.oracle(net.input(1))), "the two inputs must tell runs apart"
    net.close(fe)


DROPIN = r"""
import sys
sys.path.insert(0, %(tests)r)
import numpy as np
import cases, pool_cases
from cases import pkg
fe = cases.load_reference_frontend()          # genuine libshl_ref_x86.so: its own gref builds the graph
hip, opt = pkg.load_backend(fe)
bad = 0
for dtype, layout in (("int8", "NHWC"), ("f16", "NCHW")):
    net = pool_cases.PoolNet(dtype, layout); sess = net.build(fe, pkg.API_MI355X)
    mode = opt.shl_mi355x_session_is_device_resident(sess)
    for k in range(2):
        x = net.input(k)
        want, got = net.oracle(x), net.run(fe, x)
        if dtype == "int8":
            ok = bool(np.array_equal(got, want))
        else:
            ok = bool(np.all(np.abs(got.astype(np.float32) - want.astype(np.float32)) <= 1e-3 * np.maximum(np.abs(want.astype(np.float32)), 1e-3)))
        print(dtype, layout, "input", k, "device mode", mode, "ok", ok)
        bad += int(not ok) + int(mode < 1)
print("POOLNET_OK" if bad == 0 else "POOLNET_FAIL")
"""


@pytest.mark.gpu
@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_poolnet_drop_in_behind_the_genuine_graph_executor(gpu):
    """The reference's csinn_maxpool2d / csinn_avgpool2d and its gref record the layers; the backend's callbacks run them
    device-resident (a pool that fell through to the C reference would drop the whole session to the host path)."""
    code = DROPIN % dict(tests=os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "POOLNET_OK" in res.stdout, res.stdout + res.stderr

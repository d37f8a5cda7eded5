"""Resize inside a session (-m gpu): PyramidNet (resize_cases.py) -- the top-down path of a feature pyramid: a nearest 2x
upsample added to a lateral, a bilinear upsample concatenated with a finer map -- stays device-resident, is captured as one
hipGraph and matches the oracle chain (convolutions, the pool and softmax through the C oracle, resize, add and concat
through the numpy restatements): int8 bit for bit, binary16 within 1e-3, the project's contract for chains with MFMA
convolutions."""
import numpy as np
import pytest

import cases
import resize_cases
from cases import pkg

NETS = [("int8", "NHWC", 0), ("int8", "NHWC", 1), ("f16", "NCHW", 0), ("f16", "NCHW", 1)]


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


@pytest.fixture(scope="module")
def oracle():
    """the oracle chain's answers, computed once per (net, input)"""
    memo = {}

    def get(dtype, layout, variant, k):
        key = (dtype, layout, variant, k)
        if key not in memo:
            net = resize_cases.PyramidNet(dtype, layout, variant)
            memo[key] = net.oracle(net.input(k))
            memo[key].setflags(write=False)
        return memo[key]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout,variant", NETS)
def test_pyramidnet_runs_as_one_hipgraph_and_matches_the_oracle_chain(gpu, oracle, dtype, layout, variant, monkeypatch):
    fe, hip, opt = gpu
    monkeypatch.delenv("SHL_MI355X_HOST_SESSION", raising=False)
    net = resize_cases.PyramidNet(dtype, layout, variant)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    for k in (0, 1, 0):  # the graph replay reads fresh data
        got, want = net.run(fe, net.input(k)), oracle(dtype, layout, variant, k)
        assert got.shape == want.shape
        assert matches(got, want, dtype), "PyramidNet %s %s variant %d input %d differs from the oracle chain" % (dtype, layout, variant, k)
    assert not np.array_equal(oracle(dtype, layout, variant, 0), oracle(dtype, layout, variant, 1)), "the inputs must tell runs apart"
    net.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout,variant", NETS)
def test_the_host_staged_session_gives_the_same_answer(gpu, oracle, dtype, layout, variant, monkeypatch):
    fe, hip, opt = gpu
    monkeypatch.setenv("SHL_MI355X_HOST_SESSION", "1")  # read per setup
    net = resize_cases.PyramidNet(dtype, layout, variant)
    sess = net.build(fe, pkg.API_MI355X)
    monkeypatch.delenv("SHL_MI355X_HOST_SESSION")
    assert opt.shl_mi355x_session_is_device_resident(sess) == 0
    for k in (0, 1):
        assert matches(net.run(fe, net.input(k)), oracle(dtype, layout, variant, k), dtype), "input %d" % k
    net.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", [("int8", "NHWC"), ("f16", "NCHW")])
def test_pyramidnet_runs_on_the_callers_hbm_buffers(gpu, oracle, dtype, layout):
    """update_input / update_output with device pointers: the graph is captured again around the caller's buffers"""
    fe, hip, opt = gpu
    net = resize_cases.PyramidNet(dtype, layout, 0)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2
    dev = cases.HipDevice(hip)
    want0, want1 = oracle(dtype, layout, 0, 0), oracle(dtype, layout, 0, 1)
    assert matches(net.run(fe, net.input(0)), want0, dtype), "host run"
    x1 = net.input(1)
    dt = pkg.DTYPE_INT8 if dtype == "int8" else pkg.DTYPE_FLOAT16
    act_l = pkg.LAYOUT_NHWC if layout == "NHWC" else pkg.LAYOUT_NCHW
    d_in, d_out = dev.alloc(x1.nbytes), dev.alloc(want1.nbytes)
    dev.upload(d_in, x1)
    keep = pkg.Keep()
    fe.csinn_update_input(0, pkg.make_tensor(fe, keep, x1.shape, dt, act_l, sess=sess, device_ptr=d_in), sess)
    fe.csinn_update_output(0, pkg.make_tensor(fe, keep, want1.shape, dt, act_l, sess=sess, device_ptr=d_out), sess)
    for _ in range(2):
        assert fe.csinn_session_run(sess) == pkg.CSINN_TRUE       # enqueues only
    pkg.check(hip.shl_mi355x_stream_sync(opt.shl_mi355x_session_stream(sess)), hip, "sync")
    assert matches(dev.download(d_out, want1.shape, want1.dtype), want1, dtype), "in-place device run"
    dev.free(d_in)
    dev.free(d_out)
    net.close(fe)

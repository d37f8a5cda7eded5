"""Transposed convolution inside a session (-m gpu): DecoderNet (deconv_cases.py) -- one level of a U-Net: conv, maxpool,
conv, an up-convolution with its relu, the skip concat, conv, a 4x4 stride-2 deconvolution, sigmoid -- stays
device-resident, is captured as one hipGraph with the deconv -> relu pair folded, and matches the oracle chain: int8 bit for
bit, binary16 within 1e-3, the project's contract for chains with MFMA convolutions."""
import numpy as np
import pytest

import cases
import deconv_cases as dc
from cases import pkg

NETS = [("int8", "NHWC"), ("f16", "NCHW")]


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt


@pytest.fixture(scope="module")
def oracle():
    """the oracle chain's answers, computed once per (net, input)"""
    memo = {}

    def get(dtype, layout, k):
        key = (dtype, layout, k)
        if key not in memo:
            net = dc.DecoderNet(dtype, layout)
            memo[key] = net.oracle(net.input(k))
            memo[key].setflags(write=False)
        return memo[key]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", NETS)
def test_decoder_runs_as_one_hipgraph_and_matches_the_oracle_chain(gpu, oracle, dtype, layout, monkeypatch):
    fe, hip, opt = gpu
    monkeypatch.delenv("SHL_MI355X_HOST_SESSION", raising=False)
    monkeypatch.delenv("SHL_MI355X_DECONV_FORM", raising=False)
    net = dc.DecoderNet(dtype, layout)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    assert opt.shl_mi355x_session_folded_activations(sess) == 1, "deconv2d -> relu was not folded"
    for k in (0, 1, 0):  # the graph replay reads fresh data
        got, want = net.run(fe, net.input(k)), oracle(dtype, layout, k)
        assert got.shape == want.shape
        assert dc.matches(got, want, dtype), "DecoderNet %s %s input %d differs from the oracle chain" % (dtype, layout, k)
    assert not np.array_equal(oracle(dtype, layout, 0), oracle(dtype, layout, 1)), "the inputs must tell runs apart"
    net.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", NETS)
def test_the_host_staged_session_gives_the_same_answer(gpu, oracle, dtype, layout, monkeypatch):
    fe, hip, opt = gpu
    monkeypatch.setenv("SHL_MI355X_HOST_SESSION", "1")  # read per setup
    net = dc.DecoderNet(dtype, layout)
    sess = net.build(fe, pkg.API_MI355X)
    monkeypatch.delenv("SHL_MI355X_HOST_SESSION")
    assert opt.shl_mi355x_session_is_device_resident(sess) == 0
    for k in (0, 1):
        assert dc.matches(net.run(fe, net.input(k)), oracle(dtype, layout, k), dtype), "input %d" % k
    net.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", NETS)
def test_decoder_runs_on_the_callers_hbm_buffers(gpu, oracle, dtype, layout):
    """update_input / update_output with device pointers: the graph is captured again around the caller's buffers"""
    fe, hip, opt = gpu
    net = dc.DecoderNet(dtype, layout)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2
    dev = cases.HipDevice(hip)
    want1 = oracle(dtype, layout, 1)
    x1 = net.input(1)
    dt = pkg.DTYPE_INT8 if dtype == "int8" else pkg.DTYPE_FLOAT16
    act_l = pkg.LAYOUT_NHWC if layout == "NHWC" else pkg.LAYOUT_NCHW
    d_in, d_out = dev.alloc(x1.nbytes), dev.alloc(want1.nbytes)
    dev.upload(d_in, x1)
    keep = pkg.Keep()
    fe.csinn_update_input(0, pkg.make_tensor(fe, keep, x1.shape, dt, act_l, sess=sess, device_ptr=d_in), sess)
    fe.csinn_update_output(0, pkg.make_tensor(fe, keep, want1.shape, dt, act_l, sess=sess, device_ptr=d_out), sess)
    assert fe.csinn_session_run(sess) == pkg.CSINN_TRUE  # enqueues only
    pkg.check(hip.shl_mi355x_stream_sync(opt.shl_mi355x_session_stream(sess)), hip, "sync")
    assert dc.matches(dev.download(d_out, want1.shape, want1.dtype), want1, dtype), "in-place device run"
    dev.free(d_in)
    dev.free(d_out)
    net.close(fe)

"""Windowed max / average pooling on the GPU (-m gpu): every case of pool_cases.pool_cases() through the C ABI, the
operator API on host tensors and the operator API on DMABUF tensors, bit for bit against the genuine library's golden
outputs and the numpy restatement; the literal one-output-per-thread form against the same (which proves that the
integer-domain max of the other two forms commutes with the dequantisation); refusals that must write nothing."""
import ctypes as C

import numpy as np
import pytest

import cases
import pool_cases
from cases import pkg

CASES = pool_cases.pool_cases()
IDS = [c["name"] for c in CASES]
GOLD = pool_cases.golden()
_NUMPY = {}


def numpy_ref(case):
    """computed once per case, shared by the routes"""
    if case["name"] not in _NUMPY:
        _NUMPY[case["name"]] = pool_cases.bits(pool_cases.pool_numpy(case))
    return _NUMPY[case["name"]]


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt, cases.HipDevice(hip)


def check(got, case, route):
    pool_cases.assert_same(got, GOLD[case["name"]], "%s, %s vs reference golden" % (case["name"], route))
    pool_cases.assert_same(got, numpy_ref(case), "%s, %s vs numpy restatement" % (case["name"], route))


def cabi_run(hip, dev, case, poison=None):
    x = case["x"]
    out = np.zeros(case["out_shape"], dtype=x.dtype)
    if poison is not None:
        out.view(np.uint8)[...] = poison
    d_in, d_out = dev.alloc(x.nbytes), dev.alloc(out.nbytes)
    dev.upload(d_in, x)
    dev.upload(d_out, out)
    d = pool_cases.pool_desc(case)
    rc = hip.shl_mi355x_pool2d(d_in, d_out, C.byref(d), None)
    out = dev.download(d_out, out.shape, out.dtype)
    dev.free(d_in)
    dev.free(d_out)
    if poison is not None:
        return rc, out
    pkg.check(rc, hip, "shl_mi355x_pool2d")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pool_matches_the_reference_through_every_route(gpu, case, monkeypatch):
    fe, hip, _, dev = gpu
    monkeypatch.delenv("SHL_MI355X_POOL_FORM", raising=False)
    check(cabi_run(hip, dev, case), case, "C ABI")
    check(pool_cases.pool_run(fe, pkg.API_MI355X, case), case, "csinn_* on host tensors")
    check(pool_cases.pool_run(fe, pkg.API_MI355X, case, device=dev), case, "csinn_* on DMABUF tensors")
    # the literal form, whatever form the rules choose for this case
    monkeypatch.setenv("SHL_MI355X_POOL_FORM", "generic")
    assert hip.shl_mi355x_pool2d_kernel_name(C.byref(pool_cases.pool_desc(case))) == b"pool2d_generic"
    check(cabi_run(hip, dev, case), case, "C ABI, literal form")


@pytest.mark.gpu
def test_every_form_is_exercised(gpu, monkeypatch):
    _, hip, _, _ = gpu
    monkeypatch.delenv("SHL_MI355X_POOL_FORM", raising=False)
    seen = {}
    for case in CASES:
        name = hip.shl_mi355x_pool2d_kernel_name(C.byref(pool_cases.pool_desc(case))).decode()
        seen.setdefault((name, case["kind"], case["dtype"]), []).append(case["name"])
    for form in ("pool2d_nhwc_vec", "pool2d_nchw_row", "pool2d_generic"):
        for kind in ("max", "avg"):
            for dtype in ("int8", "f16"):
                assert (form, kind, dtype) in seen, (form, kind, dtype)


BASE = dict(kind="max", dtype="int8", layout="NHWC", n=1, c=16, h=4, w=4, ho=2, wo=2, kernel=(2, 2), stride=(2, 2),
            pad=(0, 0, 0, 0), ceil_mode=0, cip=0, in_q=(0.0625, -5), out_q=(0.0625, -5), out_shape=(1, 2, 2, 16),
            x=np.arange(256, dtype=np.uint8).view(np.int8).reshape(1, 4, 4, 16))
POISON = 0x5A


def refused(gpu, case, **kw):
    fe, hip, _, dev = gpu
    for device in (None, dev):
        rc, out = pool_cases.pool_run(fe, pkg.API_MI355X, case, device=device, poison=POISON, **kw)
        assert rc != pkg.CSINN_TRUE, "accepted"
        assert np.all(out.view(np.uint8) == POISON), "a refused call wrote to its output"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["max", "avg"])
def test_a_window_outside_the_image_is_refused(gpu, kind):
    # three output rows for a 2x2 stride-2 window on four input rows: the last window starts below the image
    case = dict(BASE, kind=kind, ho=3, out_shape=(1, 3, 2, 16))
    refused(gpu, case)
    _, hip, _, dev = gpu
    rc, out = cabi_run(hip, dev, case, poison=POISON)
    assert rc == -2 and np.all(out.view(np.uint8) == POISON)
    assert b"holds no input element" in hip.shl_mi355x_last_error()
    # NCHW, and a left pad as wide as the window
    x = np.ascontiguousarray(BASE["x"].transpose(0, 3, 1, 2))
    refused(gpu, dict(BASE, kind=kind, layout="NCHW", x=x, pad=(0, 2, 0, 0), wo=3, out_shape=(1, 16, 2, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["max", "avg"])
def test_fp16_with_a_scale_other_than_one_is_refused(gpu, kind):
    x = np.ones((1, 4, 4, 8), np.float16)
    case = dict(BASE, kind=kind, dtype="f16", c=8, x=x, out_shape=(1, 2, 2, 8), in_q=(1.0, 0), out_q=(0.5, 0))
    refused(gpu, case)
    refused(gpu, dict(case, out_q=(1.0, 0)), in_q=(2.0, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["max", "avg"])
def test_a_3d_tensor_is_refused(gpu, kind):
    x = np.ones((4, 4, 16), np.int8)
    refused(gpu, dict(BASE, kind=kind), x=x, out_shape=(2, 2, 16))


@pytest.mark.gpu
def test_per_channel_activation_records_are_refused(gpu):
    fe, hip, _, _ = gpu
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, pkg.API_MI355X, keep)
    x, out = BASE["x"], np.full(BASE["out_shape"], POISON, np.int8)
    t_in = pkg.make_tensor(fe, keep, x.shape, pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, data=x, scales=(0.5,) * 16, zps=(0,) * 16,
                           sess=sess)
    t_out = pkg.make_tensor(fe, keep, out.shape, pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, data=out, scales=(0.5,), sess=sess)
    p = pkg.pool_params(fe, keep, pkg.API_MI355X, pkg.LAYOUT_NHWC, (2, 2), (2, 2), sess=sess)
    assert fe.csinn_maxpool2d_init(t_in, t_out, p) == pkg.CSINN_TRUE
    assert fe.csinn_maxpool2d(t_in, t_out, p) != pkg.CSINN_TRUE
    assert np.all(out.view(np.uint8) == POISON)

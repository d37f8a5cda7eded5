"""Sigmoid family, leaky_relu and mul on the GPU (-m gpu): every case of eltwise_cases.eltwise_cases() through the C ABI on
device buffers, through csinn_<op> on host tensors (the staging path) and on DMABUF tensors, bit for bit against the genuine
library's golden outputs (binary16 compared on bits, the exhaustive cases included); an input one element off the 16-byte
grid; the literal mul form over the geometry list; bytes around the output must stay."""
import ctypes as C

import numpy as np
import pytest

import cases
import eltwise_cases
from cases import pkg

CASES = eltwise_cases.eltwise_cases()
IDS = [c["name"] for c in CASES]
BY = {c["name"]: c for c in CASES}
GOLD = eltwise_cases.golden()
POISON = 0x5A


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt, cases.HipDevice(hip)


def check(got, case, route):
    eltwise_cases.assert_same(got, GOLD[case["name"]], "%s, %s vs reference golden" % (case["name"], route))


def cabi_run(hip, opt, dev, case, skew=(0, 0, 0), want_form=None):
    """device buffers through shl_mi355x_unary_lut_i8 / _unary_f16 / _mul.  skew = (first input, second input, output): that
    buffer starts so many ELEMENTS into a larger allocation.  Bytes around the output are poisoned and must stay."""
    x = case["x"]
    es = x.itemsize

    def put(arr, k):
        raw = np.full(arr.nbytes + 64, POISON, np.uint8)
        raw[k * es:k * es + arr.nbytes] = arr.view(np.uint8).ravel()
        p = dev.alloc(raw.nbytes)
        dev.upload(p, raw)
        return p
    d_x = put(x, skew[0])
    frame = np.full(x.nbytes + 64, POISON, np.uint8)
    d_out = dev.alloc(frame.nbytes)
    dev.upload(d_out, frame)
    bufs = [d_x, d_out]
    p_x, p_out = d_x + skew[0] * es, d_out + skew[2] * es
    if case["op"] == "mul":
        d_y = put(case["y"], skew[1])
        bufs.append(d_y)
        desc = eltwise_cases.mul_desc(case)
        if want_form is not None:
            assert hip.shl_mi355x_mul_kernel_name(C.byref(desc), p_x, d_y + skew[1] * es, p_out).decode() == want_form
        rc = hip.shl_mi355x_mul(p_x, d_y + skew[1] * es, p_out, C.byref(desc), None)
    elif case["dtype"] == "int8":
        if want_form is not None:
            assert hip.shl_mi355x_unary_lut_i8_kernel_name(p_x, p_out).decode() == want_form
        table = (C.c_uint8 * 256)()
        a = (case["in_q"][0], case["in_q"][1], case["out_q"][0], case["out_q"][1])
        if case["op"] == "leaky_relu":
            opt.shl_mi355x_leaky_relu_table_i8(*a, case["n"], table)
        else:
            getattr(opt, "shl_mi355x_%s_table_i8" % case["op"])(*a, table)
        rc = hip.shl_mi355x_unary_lut_i8(p_x, p_out, x.size, table, None)
    else:
        rc = hip.shl_mi355x_unary_f16(p_x, p_out, x.size, eltwise_cases.KIND[case["op"]], case["n"], None)
    frame = dev.download(d_out, frame.shape, np.uint8)
    for p in bufs:
        dev.free(p)
    pkg.check(rc, hip, "C ABI call of " + case["op"])
    lo = skew[2] * es
    assert np.all(frame[:lo] == POISON) and np.all(frame[lo + x.nbytes:] == POISON), "wrote outside the output"
    return frame[lo:lo + x.nbytes].view(x.dtype).reshape(x.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_eltwise_matches_the_reference_through_every_route(gpu, case, monkeypatch):
    fe, hip, opt, dev = gpu
    monkeypatch.delenv("SHL_MI355X_MUL_FORM", raising=False)
    check(cabi_run(hip, opt, dev, case), case, "C ABI")
    check(eltwise_cases.eltwise_run(fe, pkg.API_MI355X, case), case, "csinn on host tensors")
    check(eltwise_cases.eltwise_run(fe, pkg.API_MI355X, case, device=dev), case, "csinn on DMABUF tensors")
    check(eltwise_cases.eltwise_run(fe, pkg.API_MI355X, case, device=dev, in_skew=1), case, "csinn, the input one element in")


GEOMETRY = [n for n in IDS if n.startswith("mul_") and "_grid_" not in n and "_all_by_" not in n]


@pytest.mark.gpu
@pytest.mark.parametrize("name", GEOMETRY)
def test_the_literal_mul_form_over_the_geometry_list(gpu, name, monkeypatch):
    fe, hip, opt, dev = gpu
    monkeypatch.setenv("SHL_MI355X_MUL_FORM", "generic")
    check(cabi_run(hip, opt, dev, BY[name], want_form="mul_generic"), BY[name], "C ABI, literal form")
    check(eltwise_cases.eltwise_run(fe, pkg.API_MI355X, BY[name], device=dev), BY[name], "csinn, literal form")


@pytest.mark.gpu
@pytest.mark.parametrize("name,aligned", [("silu_i8_count4101", "unary_lut_i8_vec"), ("sigmoid_i8_count17", "unary_lut_i8_vec"),
                                          ("mul_i8_nhwc_gate_c16", "mul_vec"), ("mul_f16_nhwc_channels", "mul_vec"),
                                          ("mul_i8_same_tail", "mul_vec"), ("mul_i8_nchw_hw37", "mul_row"),
                                          ("mul_f16_nchw_gate", "mul_row")])
def test_a_pointer_off_the_16_byte_grid_takes_the_unaligned_form(gpu, name, aligned, monkeypatch):
    """through the C ABI: each buffer in turn one element into a larger allocation, then all of them 16 bytes in"""
    _, hip, opt, dev = gpu
    monkeypatch.delenv("SHL_MI355X_MUL_FORM", raising=False)
    case = BY[name]
    mul = case["op"] == "mul"
    off = "mul_generic" if mul else "unary_lut_i8_byte"
    check(cabi_run(hip, opt, dev, case, want_form=aligned), case, "aligned")
    check(cabi_run(hip, opt, dev, case, skew=(1, 0, 0), want_form=off), case, "the first input one element in")
    check(cabi_run(hip, opt, dev, case, skew=(0, 0, 1), want_form=off), case, "the output one element in")
    if mul:  # b read in pieces must be aligned; a row form's or a scalar's b may lie anywhere
        check(cabi_run(hip, opt, dev, case, skew=(0, 1, 0), want_form=aligned if aligned == "mul_row" else off), case,
              "the second input one element in")
    per16 = 16 // case["x"].itemsize
    check(cabi_run(hip, opt, dev, case, skew=(per16,) * 3, want_form=aligned), case, "everything 16 bytes in")


@pytest.mark.gpu
def test_refusals_on_the_device_write_nothing(gpu):
    fe, hip, opt, dev = gpu
    case = dict(BY["mul_i8_nhwc_gate_c16"])
    case["y"] = np.zeros((2, 1, 1, 8), np.int8)   # breaks the rule
    rc, out = eltwise_cases.eltwise_run(fe, pkg.API_MI355X, case, device=dev, poison=POISON)
    assert rc != pkg.CSINN_TRUE and np.all(out.view(np.uint8) == POISON)
    rc, out = eltwise_cases.eltwise_run(fe, pkg.API_MI355X, BY["silu_f16_count8"], device=dev, poison=POISON, out_q=(0.5, 0))
    assert rc != pkg.CSINN_TRUE and np.all(out.view(np.uint8) == POISON)
    # the output aliasing the input, on the device
    p = dev.alloc(256)
    dev.upload(p, np.full(256, POISON, np.uint8))
    table = (C.c_uint8 * 256)()
    assert hip.shl_mi355x_unary_lut_i8(p, p + 32, 64, table, None) == -2 and b"overlaps" in hip.shl_mi355x_last_error()
    assert np.all(dev.download(p, (256,), np.uint8) == POISON)
    dev.free(p)

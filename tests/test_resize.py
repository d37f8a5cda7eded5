"""Resize on the GPU (-m gpu): every case of resize_cases.resize_cases() through the C ABI on device buffers, through
csinn_resize on host tensors (the staging path) and on DMABUF tensors, bit for bit against the genuine library's golden
outputs (binary16 compared on bits); an input one element off the 16-byte grid; the literal form over the geometry cases;
every size ratio of a 24 x 24 sweep against the restatement; bytes around the output must stay."""
import ctypes as C

import numpy as np
import pytest

import cases
import resize_cases
from cases import pkg

CASES = resize_cases.resize_cases()
IDS = [c["name"] for c in CASES]
BY = {c["name"]: c for c in CASES}
GOLD = resize_cases.golden()
POISON = 0x5A
VEC, ROW, GEN = "resize_nhwc_vec", "resize_nchw_row", "resize_generic"


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt, cases.HipDevice(hip)


def check(got, case, route):
    resize_cases.assert_same(got, GOLD[case["name"]], "%s, %s vs reference golden" % (case["name"], route))


def cabi_run(hip, dev, case, skew=(0, 0), want_form=None):
    """device buffers through shl_mi355x_resize.  skew = (input, output): that buffer starts so many ELEMENTS into a larger
    allocation.  Bytes around the output are poisoned and must stay."""
    x = case["x"]
    es = x.itemsize
    out_bytes = int(np.prod(case["out_shape"])) * es
    raw = np.full(x.nbytes + 64, POISON, np.uint8)
    raw[skew[0] * es:skew[0] * es + x.nbytes] = x.view(np.uint8).ravel()
    d_x = dev.alloc(raw.nbytes)
    dev.upload(d_x, raw)
    frame = np.full(out_bytes + 64, POISON, np.uint8)
    d_out = dev.alloc(frame.nbytes)
    dev.upload(d_out, frame)
    p_x, p_out = d_x + skew[0] * es, d_out + skew[1] * es
    desc = resize_cases.resize_desc(case)
    if want_form is not None:
        assert hip.shl_mi355x_resize_kernel_name(C.byref(desc), p_x, p_out).decode() == want_form
    rc = hip.shl_mi355x_resize(p_x, p_out, C.byref(desc), None)
    frame = dev.download(d_out, frame.shape, np.uint8)
    dev.free(d_x)
    dev.free(d_out)
    pkg.check(rc, hip, "C ABI call of resize")
    lo = skew[1] * es
    assert np.all(frame[:lo] == POISON) and np.all(frame[lo + out_bytes:] == POISON), "wrote outside the output"
    return frame[lo:lo + out_bytes].view(x.dtype).reshape(case["out_shape"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_resize_matches_the_reference_through_every_route(gpu, case, monkeypatch):
    fe, hip, opt, dev = gpu
    monkeypatch.delenv("SHL_MI355X_RESIZE_FORM", raising=False)
    check(cabi_run(hip, dev, case), case, "C ABI")
    check(resize_cases.resize_run(fe, pkg.API_MI355X, case), case, "csinn on host tensors")
    check(resize_cases.resize_run(fe, pkg.API_MI355X, case, device=dev), case, "csinn on DMABUF tensors")
    check(resize_cases.resize_run(fe, pkg.API_MI355X, case, device=dev, in_skew=1), case, "csinn, the input one element in")


GEOMETRY = [n for n in IDS if "_to_" in n and "_all_" not in n and "x28x28x" not in n and "x14x14_" not in n]


@pytest.mark.gpu
@pytest.mark.parametrize("name", GEOMETRY)
def test_the_literal_form_over_the_geometry_cases(gpu, name, monkeypatch):
    fe, hip, opt, dev = gpu
    monkeypatch.setenv("SHL_MI355X_RESIZE_FORM", "generic")
    check(cabi_run(hip, dev, BY[name], want_form=GEN), BY[name], "C ABI, literal form")
    check(resize_cases.resize_run(fe, pkg.API_MI355X, BY[name], device=dev), BY[name], "csinn, literal form")


@pytest.mark.gpu
@pytest.mark.parametrize("name,aligned", [("nearest_3x5_to_7x11_i8_nhwc_c32", VEC), ("bilinear_ac_13x17_to_29x37_i8_nhwc_c16", VEC),
                                          ("nearest_ac_3x5_to_6x10_f16_nhwc_c8", VEC), ("bilinear_3x5_to_7x11_f16_nhwc_c16", VEC),
                                          ("nearest_13x17_to_29x37_i8_nchw_c3", ROW), ("bilinear_3x5_to_6x10_i8_nchw_c3", ROW),
                                          ("nearest_3x5_to_7x11_f16_nchw_c3", ROW), ("bilinear_ac_13x17_to_29x37_f16_nchw_c3", ROW)])
def test_a_pointer_off_the_grid_takes_the_unaligned_form(gpu, name, aligned, monkeypatch):
    """through the C ABI: each buffer in turn one element into a larger allocation, then both of them 16 bytes in.  The row
    form gathers its input element by element, so only its output has to sit on the (4-byte) grid"""
    _, hip, opt, dev = gpu
    monkeypatch.delenv("SHL_MI355X_RESIZE_FORM", raising=False)
    case = BY[name]
    check(cabi_run(hip, dev, case, want_form=aligned), case, "aligned")
    check(cabi_run(hip, dev, case, skew=(1, 0), want_form=GEN if aligned == VEC else ROW), case, "the input one element in")
    check(cabi_run(hip, dev, case, skew=(0, 1), want_form=GEN), case, "the output one element in")
    per16 = 16 // case["x"].itemsize
    check(cabi_run(hip, dev, case, skew=(per16, per16), want_form=aligned), case, "everything 16 bytes in")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(resize_cases.MODES))
def test_index_arithmetic_at_every_ratio(gpu, mode):
    """n x n -> m x m for n, m in 1 .. 24, int8, one channel, both align_corners values where defined: one small launch per
    pair through the C ABI, against the restatement that tests/test_resize_cpu.py ties to the genuine library at the same
    sizes.  The inputs of all sizes sit in one upload, the outputs come back in one download per n."""
    _, hip, opt, dev = gpu
    q = resize_cases.RECORD_PAIRS["conv"]
    sizes = range(1, 25)
    d_in, d_out = dev.alloc(24 * 24), dev.alloc(2 * 24 * 24 * 24 + 64)
    for n in sizes:
        x = ((np.arange(n * n, dtype=np.int64) * 37 + 11) % 251 - 125).astype(np.int8).reshape(1, n, n, 1)
        dev.upload(d_in, x)
        want, at = [], 0
        for m in sizes:
            for align in (False, True):
                if align and m == 1:
                    continue
                case = dict(mode=mode, align=align, dtype="int8", layout="NHWC", n=1, c=1, h=n, w=n, ho=m, wo=m, in_q=q[0],
                            out_q=q[1], x=x, out_shape=(1, m, m, 1))
                desc = resize_cases.resize_desc(case)
                pkg.check(hip.shl_mi355x_resize(d_in, d_out + at, C.byref(desc), None), hip, "resize %d -> %d" % (n, m))
                want.append(resize_cases.resize_numpy(case).ravel())
                at += m * m
        want = np.concatenate(want)
        got = dev.download(d_out, want.shape, np.int8)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s from %dx%d: %d outputs differ, first at flat index %d" % (mode, n, n, bad.size, bad[0])
    dev.free(d_in)
    dev.free(d_out)


@pytest.mark.gpu
def test_refusals_on_the_device_write_nothing(gpu):
    fe, hip, opt, dev = gpu
    for name, override in (("bilinear_5x4_to_1x1_i8_nhwc_c16", dict(align=True)),
                           ("nearest_3x5_to_7x11_i8_nhwc_c16", dict(mode=pkg.RESIZE_NEAREST_BICUBIC)),
                           ("bilinear_3x5_to_7x11_f16_nchw_c3", dict(out_shape=(1, 4, 7, 11))),
                           ("bilinear_3x5_to_7x11_f16_nhwc_c8", dict(out_q=(0.5, 0)))):
        rc, out = resize_cases.resize_run(fe, pkg.API_MI355X, BY[name], device=dev, poison=POISON, **override)
        assert rc != pkg.CSINN_TRUE and np.all(out.view(np.uint8) == POISON), name
    # the output aliasing the input, on the device
    case = BY["nearest_2x2_to_4x4_i8_nhwc_c16"]
    p = dev.alloc(1024)
    dev.upload(p, np.full(1024, POISON, np.uint8))
    desc = resize_cases.resize_desc(case)
    assert hip.shl_mi355x_resize(p, p + 48, C.byref(desc), None) == -2 and b"overlaps" in hip.shl_mi355x_last_error()
    assert np.all(dev.download(p, (1024,), np.uint8) == POISON)
    dev.free(p)

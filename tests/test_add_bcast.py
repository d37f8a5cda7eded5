"""The broadcasting add on the GPU (-m gpu): every case of add_bcast_cases.add_cases() through the C ABI on device buffers,
through csinn_add on host tensors (the staging path) and on DMABUF tensors, bit for bit against the genuine library's golden
outputs (binary16 compared on bits, the exhaustive cases included); the literal form over the geometry list; pointers off
the 16-byte grid; bytes around the output must stay; refusals write nothing."""
import ctypes as C

import numpy as np
import pytest

import add_bcast_cases
import cases
from cases import pkg

CASES = add_bcast_cases.add_cases()
IDS = [c["name"] for c in CASES]
BY = {c["name"]: c for c in CASES}
GOLD = add_bcast_cases.golden()
POISON = 0x5A


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt, cases.HipDevice(hip)


def check(got, case, route):
    add_bcast_cases.assert_same(got, GOLD[case["name"]], "%s, %s vs reference golden" % (case["name"], route))


def cabi_run(hip, dev, case, skew=(0, 0, 0), want_form=None):
    """device buffers through shl_mi355x_add_bcast.  skew = (a, b, output): that buffer starts so many ELEMENTS into a larger
    allocation.  Bytes around the output are poisoned and must stay."""
    x = case["x"]
    es = x.itemsize

    def put(arr, k):
        raw = np.full(arr.nbytes + 64, POISON, np.uint8)
        raw[k * es:k * es + arr.nbytes] = arr.view(np.uint8).ravel()
        p = dev.alloc(raw.nbytes)
        dev.upload(p, raw)
        return p
    d_x, d_y = put(x, skew[0]), put(case["y"], skew[1])
    frame = np.full(x.nbytes + 64, POISON, np.uint8)
    d_out = dev.alloc(frame.nbytes)
    dev.upload(d_out, frame)
    p_x, p_y, p_out = d_x + skew[0] * es, d_y + skew[1] * es, d_out + skew[2] * es
    desc = add_bcast_cases.add_desc(case)
    if want_form is not None:
        assert hip.shl_mi355x_add_bcast_kernel_name(C.byref(desc), p_x, p_y, p_out).decode() == want_form
    rc = hip.shl_mi355x_add_bcast(p_x, p_y, p_out, C.byref(desc), None)
    frame = dev.download(d_out, frame.shape, np.uint8)
    for p in (d_x, d_y, d_out):
        dev.free(p)
    pkg.check(rc, hip, "shl_mi355x_add_bcast")
    lo = skew[2] * es
    assert np.all(frame[:lo] == POISON) and np.all(frame[lo + x.nbytes:] == POISON), "wrote outside the output"
    return frame[lo:lo + x.nbytes].view(x.dtype).reshape(x.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_add_matches_the_reference_through_every_route(gpu, case, monkeypatch):
    fe, hip, opt, dev = gpu
    monkeypatch.delenv("SHL_MI355X_ADD_FORM", raising=False)
    check(cabi_run(hip, dev, case), case, "C ABI")
    check(add_bcast_cases.add_run(fe, pkg.API_MI355X, case), case, "csinn on host tensors")
    check(add_bcast_cases.add_run(fe, pkg.API_MI355X, case, device=dev), case, "csinn on DMABUF tensors")
    check(add_bcast_cases.add_run(fe, pkg.API_MI355X, case, device=dev, in_skew=1), case, "csinn, the full operand one element in")


GEOMETRY = [n for n in IDS if "_grid_" not in n and "_all_by_" not in n]


@pytest.mark.gpu
@pytest.mark.parametrize("name", GEOMETRY)
def test_the_literal_form_over_the_geometry_list(gpu, name, monkeypatch):
    fe, hip, opt, dev = gpu
    monkeypatch.setenv("SHL_MI355X_ADD_FORM", "generic")
    check(cabi_run(hip, dev, BY[name], want_form="add_generic"), BY[name], "C ABI, literal form")
    check(add_bcast_cases.add_run(fe, pkg.API_MI355X, BY[name], device=dev), BY[name], "csinn, literal form")


@pytest.mark.gpu
@pytest.mark.parametrize("name,aligned", [("add_i8_bias_n16", "add_vec"), ("add_f16_bias_2x17x64", "add_vec"),
                                          ("add_i8_posemb_2x17x64", "add_vec"), ("add_f16_scalar_tail", "add_vec"),
                                          ("add_i8_nchw_hw37", "add_row"), ("add_f16_nchw_channels", "add_row"),
                                          ("add_i8_attn_bias_2x2x17x17", "add_generic")])
def test_a_pointer_off_the_16_byte_grid_takes_the_unaligned_form(gpu, name, aligned, monkeypatch):
    """through the C ABI: each buffer in turn one element into a larger allocation, then all of them 16 bytes in"""
    _, hip, opt, dev = gpu
    monkeypatch.delenv("SHL_MI355X_ADD_FORM", raising=False)
    case = BY[name]
    off = "add_generic"
    check(cabi_run(hip, dev, case, want_form=aligned), case, "aligned")
    check(cabi_run(hip, dev, case, skew=(1, 0, 0), want_form=off), case, "a one element in")
    check(cabi_run(hip, dev, case, skew=(0, 0, 1), want_form=off), case, "the output one element in")
    # b read in pieces must be aligned; a row form's or a scalar's b may lie anywhere
    b_free = aligned == "add_row" or case["y"].size == 1
    check(cabi_run(hip, dev, case, skew=(0, 1, 0), want_form=aligned if b_free else off), case, "b one element in")
    per16 = 16 // case["x"].itemsize
    check(cabi_run(hip, dev, case, skew=(per16,) * 3, want_form=aligned), case, "everything 16 bytes in")


@pytest.mark.gpu
def test_refusals_on_the_device_write_nothing(gpu):
    fe, hip, opt, dev = gpu
    run = lambda case, **kw: add_bcast_cases.add_run(fe, pkg.API_MI355X, case, device=dev, poison=POISON, **kw)
    base = BY["add_i8_nhwc_gate_c16"]
    both = dict(base, x=np.zeros((2, 3, 1, 16), np.int8))                          # both operands need broadcasting
    rc, out = run(both, out_shape=(2, 3, 5, 16))
    assert rc != pkg.CSINN_TRUE and np.all(out.view(np.uint8) == POISON)
    rule = dict(base, y=np.zeros((2, 1, 1, 8), np.int8))                           # a dim that is neither equal nor 1
    rc, out = run(rule)
    assert rc != pkg.CSINN_TRUE and np.all(out.view(np.uint8) == POISON)
    five = dict(base, x=np.zeros((2, 3, 2, 3, 2), np.int8), y=np.zeros((2, 1, 2, 1, 2), np.int8))  # five groups
    rc, out = run(five)
    assert rc != pkg.CSINN_TRUE and np.all(out.view(np.uint8) == POISON)
    rc, out = run(BY["add_f16_bias_n16"], out_q=(0.5, 0))                         # binary16 scale != 1
    assert rc != pkg.CSINN_TRUE and np.all(out.view(np.uint8) == POISON)
    # the output overlapping an operand, on the device
    p = dev.alloc(1024)
    dev.upload(p, np.full(1024, POISON, np.uint8))
    desc = add_bcast_cases.add_desc(BY["add_i8_bias_n16"])                        # 480 elements + 16
    for a, b, o in ((p, p + 512, p + 479), (p + 512, p, p + 15), (p, p + 512, p + 527)):
        assert hip.shl_mi355x_add_bcast(a, b, o, C.byref(desc), None) == -2 and b"overlaps" in hip.shl_mi355x_last_error()
        assert hip.shl_mi355x_add_bcast_kernel_name(C.byref(desc), a, b, o) == b""
    assert np.all(dev.download(p, (1024,), np.uint8) == POISON)
    dev.free(p)

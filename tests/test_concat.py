"""Concat on the GPU (-m gpu): every case of concat_cases.concat_cases() through the C ABI on device buffers, through
csinn_concat on host tensors (the packed staging path), on DMABUF tensors and on a mix of both, bit for bit against the
genuine library's golden outputs (binary16 compared on bits); the literal one-element-per-thread form against the same
golden; pointers one element off the 16-byte grid; refusals that must write nothing."""
import ctypes as C

import numpy as np
import pytest

import cases
import concat_cases
from cases import pkg

CASES = concat_cases.concat_cases()
IDS = [c["name"] for c in CASES]
GOLD = concat_cases.golden()
VEC, GEN = "concat_vec", "concat_generic"
POISON = 0x5A


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt, cases.HipDevice(hip)


def check(got, case, route):
    concat_cases.assert_same(got, GOLD[case["name"]], "%s, %s vs reference golden" % (case["name"], route))


def cabi_run(hip, dev, case, in_skew=None, out_skew=0, want_form=None):
    """device buffers through shl_mi355x_concat.  in_skew[i] / out_skew: that buffer starts so many ELEMENTS into a larger
    allocation.  Bytes around the output are poisoned and must stay."""
    es = case["xs"][0].itemsize
    in_skew = in_skew or [0] * len(case["xs"])
    bufs, ptrs, made = [], [], {}
    for i, x in enumerate(case["xs"]):
        k = case["alias"][i]
        if k not in made:
            raw = np.full(x.nbytes + 64, POISON, np.uint8)
            raw[in_skew[i] * es:in_skew[i] * es + x.nbytes] = x.view(np.uint8).ravel()
            p = dev.alloc(raw.nbytes)
            dev.upload(p, raw)
            bufs.append(p)
            made[k] = p + in_skew[i] * es
        ptrs.append(made[k])
    nbytes = int(np.prod(case["out_shape"])) * es
    frame = np.full(nbytes + 64, POISON, np.uint8)
    d_out = dev.alloc(frame.nbytes)
    dev.upload(d_out, frame)
    args = concat_cases.CabiArgs(case, ptrs)
    if want_form is not None:
        assert args.name(hip, d_out + out_skew * es) == want_form
    rc = args.run(hip, d_out + out_skew * es)
    frame = dev.download(d_out, frame.shape, np.uint8)
    for p in bufs + [d_out]:
        dev.free(p)
    pkg.check(rc, hip, "shl_mi355x_concat")
    lo = out_skew * es
    assert np.all(frame[:lo] == POISON) and np.all(frame[lo + nbytes:] == POISON), "wrote outside the output"
    return frame[lo:lo + nbytes].view(case["xs"][0].dtype).reshape(case["out_shape"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_concat_matches_the_reference_through_every_route(gpu, case, monkeypatch):
    fe, hip, _, dev = gpu
    monkeypatch.delenv("SHL_MI355X_CONCAT_FORM", raising=False)
    check(cabi_run(hip, dev, case), case, "C ABI")
    check(concat_cases.concat_run(fe, pkg.API_MI355X, case), case, "csinn_concat on host tensors")
    check(concat_cases.concat_run(fe, pkg.API_MI355X, case, device=dev), case, "csinn_concat on DMABUF tensors")
    # the literal form, whatever form the rules choose for this case
    monkeypatch.setenv("SHL_MI355X_CONCAT_FORM", "generic")
    check(cabi_run(hip, dev, case, want_form=GEN), case, "C ABI, literal form")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["records_one_differs", "count9_f16_generic", "same_tensor_twice_i8", "count17_i8_vec"])
def test_host_and_dmabuf_inputs_mix(gpu, name, monkeypatch):
    fe, _, _, dev = gpu
    monkeypatch.delenv("SHL_MI355X_CONCAT_FORM", raising=False)
    case = next(c for c in CASES if c["name"] == name)
    odd = concat_cases.concat_run(fe, pkg.API_MI355X, case, device=dev, on_device=lambda i: i >= 0 and i % 2 == 1)
    check(odd, case, "odd inputs in HBM, the rest and the output on the host")
    even = concat_cases.concat_run(fe, pkg.API_MI355X, case, device=dev, on_device=lambda i: i < 0 or i % 2 == 0)
    check(even, case, "even inputs and the output in HBM, the rest on the host")


def test_every_form_is_exercised(built, monkeypatch):
    """(needs no device: the rules are host code)"""
    hip = pkg.load_hip()
    monkeypatch.delenv("SHL_MI355X_CONCAT_FORM", raising=False)
    seen = set()
    for case in CASES:
        ptrs = [(i + 1) << 24 for i in range(len(case["xs"]))]
        launches = (sum(1 for x in case["xs"] if x.size) + 7) // 8
        seen.add((concat_cases.CabiArgs(case, ptrs).name(hip, 1 << 40), case["dtype"], min(launches, 3)))
    for form in (VEC, GEN):
        for dtype in ("int8", "f16"):
            for launches in (1, 2, 3):
                assert (form, dtype, launches) in seen, (form, dtype, launches)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["form_i8_nhwc_16_32_48", "form_f16_nhwc_8_24", "records_one_differs"])
def test_a_pointer_off_the_16_byte_grid_takes_the_literal_form(gpu, name, monkeypatch):
    """through the C ABI only: an input, and separately the output, one element into a larger device buffer"""
    _, hip, _, dev = gpu
    monkeypatch.delenv("SHL_MI355X_CONCAT_FORM", raising=False)
    case = next(c for c in CASES if c["name"] == name)
    n = len(case["xs"])
    check(cabi_run(hip, dev, case, want_form=VEC), case, "aligned")
    for i in range(n):
        skew = [1 if j == i else 0 for j in range(n)]
        check(cabi_run(hip, dev, case, in_skew=skew, want_form=GEN), case, "input %d one element in" % i)
    check(cabi_run(hip, dev, case, out_skew=1, want_form=GEN), case, "the output one element in")
    per16 = 16 // case["xs"][0].itemsize
    check(cabi_run(hip, dev, case, in_skew=[per16] * n, out_skew=per16, want_form=VEC), case, "everything 16 bytes in")


@pytest.mark.gpu
def test_refusals_write_nothing(gpu):
    fe, hip, _, dev = gpu
    case = next(c for c in CASES if c["name"] == "records_one_differs")
    wrong = tuple(case["out_shape"][:3]) + (case["out_shape"][3] + 16,)
    for device in (None, dev):
        for kw in (dict(out_shape=wrong), dict(axis=4), dict(axis=2), dict(count=0)):
            rc, out = concat_cases.concat_run(fe, pkg.API_MI355X, case, device=device, poison=POISON, **kw)
            assert rc != pkg.CSINN_TRUE, kw
            assert np.all(out.view(np.uint8) == POISON), "a refused call wrote to its output: %r" % (kw,)
    # the output aliasing an input, on the device
    x = case["xs"][0]
    p = dev.alloc(8 * x.nbytes)
    dev.upload(p, np.full(8 * x.nbytes, POISON, np.uint8))
    args = concat_cases.CabiArgs(case, [p, p + x.nbytes, p])
    assert args.run(hip, p + x.nbytes) == -2 and b"overlaps an input" in hip.shl_mi355x_last_error()
    assert np.all(dev.download(p, (8 * x.nbytes,), np.uint8) == POISON)
    dev.free(p)


@pytest.mark.gpu
def test_fp16_with_a_scale_other_than_one_is_refused(gpu):
    fe, _, _, dev = gpu
    case = dict(next(c for c in CASES if c["name"] == "form_f16_nhwc_8_24"))
    for bad in (dict(out_q=(0.5, 0)), dict(in_qs=[(1.0, 0), (2.0, 0)])):
        rc, out = concat_cases.concat_run(fe, pkg.API_MI355X, dict(case, **bad), device=dev, poison=POISON)
        assert rc != pkg.CSINN_TRUE and np.all(out.view(np.uint8) == POISON)

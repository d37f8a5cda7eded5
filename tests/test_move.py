"""Transpose, pad, reshape and flatten on the GPU (-m gpu): every case of move_cases through the C ABI on device buffers -- in
the form the rules choose and under every value of the form switch, the output between poisoned guard bands --, through
csinn_<op> on host tensors (the staging path) and on DMABUF tensors, bit for bit against the genuine library's golden outputs
(binary16 compared on bits); pointers off the 16-byte grid; what `perf` reports; refusals that must write nothing."""
import ctypes as C

import numpy as np
import pytest

import cases
import move_cases as mc
from cases import pkg

CASES = mc.all_cases()
IDS = [mc.case_id(c) for c in CASES]
GOLD = mc.golden()
POISON = 0x5A
GUARD = 64  # bytes of poison on each side of the output


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt, cases.HipDevice(hip)


def check(got, case, route):
    mc.assert_same(got, GOLD[mc.golden_key(case)], "%s, %s vs reference golden" % (mc.case_id(case), route))


def cabi_run(hip, dev, case, in_skew=0, out_skew=0, want_form=None, expect_rc=0, args=None):
    """device buffers through the C ABI.  in_skew / out_skew: that buffer starts so many BYTES further into its allocation.
    The output sits between GUARD bytes of poison on each side, which must stay; with expect_rc != 0 the output itself is
    poisoned too and must stay."""
    x = case["x"]
    shape = case["out_shape"]
    nbytes = int(np.prod(shape)) * x.itemsize
    raw = np.full(x.nbytes + 64, POISON, np.uint8)
    raw[in_skew:in_skew + x.nbytes] = x.view(np.uint8).ravel()
    d_in = dev.alloc(raw.nbytes)
    dev.upload(d_in, raw)
    frame = np.full(GUARD + out_skew + nbytes + GUARD, POISON, np.uint8)
    d_out = dev.alloc(frame.nbytes)
    dev.upload(d_out, frame)
    args = args or mc.cabi_args(case)
    if want_form is not None:
        assert args.name(hip, d_in + in_skew, d_out + GUARD + out_skew) == want_form
    rc = args.run(hip, d_in + in_skew, d_out + GUARD + out_skew)
    got = dev.download(d_out, frame.shape, np.uint8)
    dev.free(d_out)
    dev.free(d_in)
    lo = GUARD + out_skew
    assert np.all(got[:lo] == POISON) and np.all(got[lo + nbytes:] == POISON), "wrote outside the output"
    if expect_rc != 0:
        assert np.all(got == POISON), "a refused call wrote to the output"
    assert rc == expect_rc, (rc, hip.shl_mi355x_last_error())
    return got[lo:lo + nbytes].view(x.dtype).reshape(shape)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matches_the_reference_through_every_route(gpu, case, monkeypatch):
    fe, hip, _, dev = gpu
    env = mc.FORM_ENV[case["op"]]
    monkeypatch.delenv(env, raising=False)
    natural = mc.expected_form(case)
    check(cabi_run(hip, dev, case, want_form=natural), case, "C ABI, " + natural)
    names = []

    def perf(cb, t_in, t_out, params):
        tp = C.POINTER(pkg.Tensor)
        name = C.c_char_p()
        fn = C.CFUNCTYPE(C.c_int, tp, tp, C.c_void_p, C.POINTER(C.c_char_p))(cb.contents.perf)
        assert fn(t_in, t_out, params, C.byref(name)) == pkg.CSINN_TRUE
        names.append(name.value.decode())
    check(mc.layer_run(fe, pkg.API_MI355X, case, perf=perf), case, "operator API on host tensors")
    check(mc.layer_run(fe, pkg.API_MI355X, case, device=dev, perf=perf), case, "operator API on DMABUF tensors")
    assert names == [natural, natural], "perf reports the launched form"
    # every value of the switch: the forced form where the arguments admit it, the literal form where they do not
    for force in mc.FORCES[case["op"]]:
        monkeypatch.setenv(env, force)
        form = mc.expected_form(case, force=force)
        check(cabi_run(hip, dev, case, want_form=form), case, "C ABI, forced to " + force)


SKEWED = ["transpose.65x67_i8_both", "transpose.64x64_f16", "transpose.128x4_i8_zp", "transpose.2x16x7x7_to_nhwc_i8_div", "transpose.1x64x8x8_to_nhwc_i8_eq", "transpose.heads_2x5x4x16_f16", "transpose.heads_2x5x4x16_i8_eq",
          "transpose.identity_2x3x4x5_i8_eq", "transpose.yolo_1x3x8x4x4_f16", "pad.vec_2x4x4x16_hw_11_nhwc_i8_eq",
          "pad.vec_2x4x4x16_hw_11_nchw_f16", "reshape.4099_i8_eq", "flatten.16_f16"]


@pytest.mark.gpu
@pytest.mark.parametrize("key", SKEWED)
def test_pointers_off_the_grid_take_a_narrower_form(gpu, key, monkeypatch):
    """a case with one pointer 4 bytes, then one element, into its allocation -- the input, and separately the output --
    runs the form the rules give that alignment and still matches; everything 16 bytes in keeps the form"""
    _, hip, _, dev = gpu
    case = next(c for c in CASES if mc.golden_key(c) == key)
    monkeypatch.delenv(mc.FORM_ENV[case["op"]], raising=False)
    es = case["x"].itemsize
    for skew, align in ((4, 4), (es, es), (16, 16)):
        check(cabi_run(hip, dev, case, in_skew=skew, want_form=mc.expected_form(case, align_in=align)), case, "input %d bytes in" % skew)
        check(cabi_run(hip, dev, case, out_skew=skew, want_form=mc.expected_form(case, align_out=align)), case, "output %d bytes in" % skew)
    natural = mc.expected_form(case)
    check(cabi_run(hip, dev, case, in_skew=16, out_skew=16, want_form=natural), case, "everything 16 bytes in")


@pytest.mark.gpu
def test_refused_arguments_fail_and_write_nothing(gpu):
    fe, hip, _, dev = gpu
    by_key = {mc.golden_key(c): c for c in CASES}
    tr, pad = by_key["transpose.2x3x5x7_to_nhwc_i8_both"], by_key["pad.hw_11_nhwc_i8_both"]
    flat = by_key["reshape.2x1x1x24_i8_eq"]
    # through the C ABI: what only it can be handed
    for field, k, value in (("perm", 1, 0), ("perm", 2, 4), ("perm", 0, -1), ("dim", 1, -3)):
        args = mc.cabi_args(tr)
        getattr(args.desc, field)[k] = value
        cabi_run(hip, dev, tr, expect_rc=-2, args=args)
    for rank in (0, 9):
        args = mc.cabi_args(tr)
        args.desc.rank = rank
        cabi_run(hip, dev, tr, expect_rc=-2, args=args)
    for field, k, value in (("before", 1, -1), ("after", 2, -1), ("dim", 3, -1)):
        args = mc.cabi_args(pad)
        getattr(args.desc, field)[k] = value
        cabi_run(hip, dev, pad, expect_rc=-2, args=args)
    args = mc.cabi_args(flat)
    args.elems = -1
    cabi_run(hip, dev, flat, expect_rc=-2, args=args)
    # through the operator API, on host and on DMABUF tensors
    for device in (None, dev):
        for case, kw in ((tr, dict(permute_num=3)), (tr, dict(perm=(0, 2, 2, 1))), (tr, dict(perm=(0, 2, 4, 1))),
                         (tr, dict(perm=(0, 2, -1, 1))), (tr, dict(out_shape=(2, 5, 3, 7))), (tr, dict(out_shape=(2, 5, 7, 2))),
                         (tr, dict(in_scales=(0.5, 0.25))), (tr, dict(out_dt=pkg.DTYPE_FLOAT32)),
                         (pad, dict(mode=pkg.PAD_EDGE)), (pad, dict(mode=pkg.PAD_REFLECT)), (pad, dict(pad_num=3)),
                         (pad, dict(before=[0, -1, 1, 0], out_shape=(1, 5, 7, 3))), (pad, dict(out_shape=(1, 7, 6, 3))),
                         (pad, dict(out_shape=(1, 7, 7, 4))), (pad, dict(layout=pkg.LAYOUT_NC)),
                         (flat, dict(out_shape=(2, 23))), (flat, dict(out_shape=(2, 25))),
                         (dict(flat, op="flatten"), dict(out_shape=(47,)))):
            rc, out = mc.layer_run(fe, pkg.API_MI355X, case, device=device, poison=POISON, **kw)
            assert rc != pkg.CSINN_TRUE, kw
            assert np.all(out.view(np.uint8) == POISON), "a refused call wrote to the output: %r" % (kw,)
    # an output overlapping the input, on the device
    x = tr["x"]
    p = dev.alloc(4 * x.nbytes)
    dev.upload(p, np.full(4 * x.nbytes, POISON, np.uint8))
    for case in (tr, pad, flat):
        assert mc.cabi_args(case).run(hip, p, p + case["x"].nbytes - 1) == -2 and b"overlaps the input" in hip.shl_mi355x_last_error()
    assert np.all(dev.download(p, (4 * x.nbytes,), np.uint8) == POISON)
    dev.free(p)


@pytest.mark.gpu
def test_fp16_with_a_scale_other_than_one_is_refused(gpu):
    fe, _, _, dev = gpu
    by_key = {mc.golden_key(c): c for c in CASES}
    for key in ("transpose.3x5_f16", "pad.hw_11_nhwc_f16", "reshape.15_f16", "flatten.15_f16"):
        for case in (dict(by_key[key], out_q=(0.5, 0)), dict(by_key[key], in_q=(2.0, 0))):
            rc, out = mc.layer_run(fe, pkg.API_MI355X, case, device=dev, poison=POISON)
            assert rc != pkg.CSINN_TRUE and np.all(out.view(np.uint8) == POISON)

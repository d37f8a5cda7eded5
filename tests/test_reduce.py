"""The reductions on the GPU (-m gpu): every case of reduce_cases through the C ABI on device buffers -- in the form the rule
chooses and again forced to the literal form, the output between poisoned guard bands --, through csinn_<op> on host tensors
(the staging path) and on DMABUF tensors, bit for bit against the genuine library's golden outputs (binary16 compared on
bits); pointers 1, 2 and 4 elements off the 16-byte grid; what `perf` reports; refusals that must write nothing."""
import ctypes as C

import numpy as np
import pytest

import cases
import reduce_cases as rc
from cases import pkg

CASES = rc.all_cases()
IDS = [rc.case_id(c) for c in CASES]
GOLD = rc.golden()
POISON = 0x5A
GUARD = 64  # bytes of poison on each side of the output
FORM_ENV = "SHL_MI355X_REDUCE_FORM"


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt, cases.HipDevice(hip)


def check(got, case, route):
    rc.assert_same(got, GOLD[rc.golden_key(case)].reshape(got.shape), "%s, %s vs reference golden" % (rc.case_id(case), route))


def cabi_run(hip, dev, case, in_skew=0, out_skew=0, want_form=None, expect_rc=0, desc=None):
    """device buffers through the C ABI.  in_skew / out_skew: that buffer starts so many BYTES further into its allocation.
    The output sits between GUARD bytes of poison on each side, which must stay; with expect_rc != 0 the output itself is
    poisoned too and must stay."""
    x = case["x"]
    shape = rc.out_shape_of(case)
    nbytes = int(np.prod(shape)) * x.itemsize
    raw = np.full(x.nbytes + 64, POISON, np.uint8)
    raw[in_skew:in_skew + x.nbytes] = x.view(np.uint8).ravel()
    d_in = dev.alloc(raw.nbytes)
    dev.upload(d_in, raw)
    frame = np.full(GUARD + out_skew + nbytes + GUARD, POISON, np.uint8)
    d_out = dev.alloc(frame.nbytes)
    dev.upload(d_out, frame)
    desc = desc or rc.cabi_desc(case)
    if want_form is not None:
        assert hip.shl_mi355x_reduce_kernel_name(d_in + in_skew, d_out + GUARD + out_skew, C.byref(desc)).decode() == want_form
    status = hip.shl_mi355x_reduce(d_in + in_skew, d_out + GUARD + out_skew, C.byref(desc), None)
    got = dev.download(d_out, frame.shape, np.uint8)
    dev.free(d_out)
    dev.free(d_in)
    lo = GUARD + out_skew
    assert np.all(got[:lo] == POISON) and np.all(got[lo + nbytes:] == POISON), "wrote outside the output"
    if expect_rc != 0:
        assert np.all(got == POISON), "a refused call wrote to the output"
    assert status == expect_rc, (status, hip.shl_mi355x_last_error())
    return got[lo:lo + nbytes].view(x.dtype).reshape(shape)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matches_the_reference_through_every_route(gpu, case, monkeypatch):
    fe, hip, _, dev = gpu
    monkeypatch.delenv(FORM_ENV, raising=False)
    natural = rc.expected_form(case)
    check(cabi_run(hip, dev, case, want_form=natural), case, "C ABI, " + natural)
    names = []

    def perf(cb, t_in, t_out, params):
        tp = C.POINTER(pkg.Tensor)
        name = C.c_char_p()
        fn = C.CFUNCTYPE(C.c_int, tp, tp, C.c_void_p, C.POINTER(C.c_char_p))(cb.contents.perf)
        assert fn(t_in, t_out, params, C.byref(name)) == pkg.CSINN_TRUE
        names.append(name.value.decode())
    check(rc.layer_run(fe, pkg.API_MI355X, case, perf=perf), case, "operator API on host tensors")
    check(rc.layer_run(fe, pkg.API_MI355X, case, device=dev, perf=perf), case, "operator API on DMABUF tensors")
    assert names == [natural, natural], "perf reports the launched form"
    monkeypatch.setenv(FORM_ENV, "generic")
    check(cabi_run(hip, dev, case, want_form="reduce_generic"), case, "C ABI, forced to generic")


SKEWED = ["mean.row_3x257_i8", "sum.row_3x259_f16", "max.row_3x515_i8", "min.row_3x63_f16", "sum.row_3x1_i8", "mean.row_3x2_f16",
          "mean.nchw_over_hw_i8", "max.nchw_over_hw_f16", "sum.rows_of_two_runs_i8", "min.rows_of_two_runs_f16",
          "sum.rows_257x5_i8", "mean.rows_65x5_f16", "mean.nhwc_over_hw_i8", "max.cols_5x257_f16", "sum.col_257x3_i8",
          "reduce_sum.whole_tensor_f16", "reduce_max.rank4_axis3_i8", "reduce_mean.last_axis_257_f16",
          "global_maxpool2d.7x7_nchw_i8", "global_maxpool2d.5x9_nhwc_f16", "sum.order_rows_i8", "mean.order_rows_f16",
          "max.special_rows_f16", "sum.strided_generic_i8"]


@pytest.mark.gpu
@pytest.mark.parametrize("key", SKEWED)
def test_pointers_off_the_16_byte_grid(gpu, key, monkeypatch):
    """the input, and separately the output, 1, 2 and 4 elements into its allocation: the form stays (heads and tails off the
    grid take element loads inside the same launch) and the outputs still match"""
    _, hip, _, dev = gpu
    case = next(c for c in CASES if rc.golden_key(c) == key)
    monkeypatch.delenv(FORM_ENV, raising=False)
    es = case["x"].itemsize
    natural = rc.expected_form(case)
    for elems in (1, 2, 4):
        check(cabi_run(hip, dev, case, in_skew=elems * es, want_form=natural), case, "input %d elements in" % elems)
        check(cabi_run(hip, dev, case, out_skew=elems * es, want_form=natural), case, "output %d elements in" % elems)
    check(cabi_run(hip, dev, case, in_skew=3 * es, out_skew=5 * es, want_form=natural), case, "both off the grid")


@pytest.mark.gpu
def test_refused_arguments_fail_and_write_nothing(gpu):
    fe, hip, _, dev = gpu
    by_key = {rc.golden_key(c): c for c in CASES}
    mean, axis, gmp = by_key["mean.nchw_over_hw_i8"], by_key["reduce_max.rank4_axis3_i8"], by_key["global_maxpool2d.7x7_nchw_i8"]
    # through the C ABI: what only it can be handed
    for field, k, value in (("out_extent", 0, -1), ("out_stride", 1, -49), ("inner_extent", 0, 0), ("inner_stride", 1, -1),
                            ("inner_extent", 0, 8), ("out_stride", 0, 246)):  # (the last two reach past the input)
        desc = rc.cabi_desc(mean)
        getattr(desc, field)[k] = value
        cabi_run(hip, dev, mean, expect_rc=-2, desc=desc)
    for field, value in (("kind", 4), ("kind", -1), ("init", 2), ("dtype", 7), ("n_out", 9), ("n_inner", -1), ("in_elems", 0),
                         ("in_elems", 1 << 31), ("in_elems", mean["x"].size - 1)):
        desc = rc.cabi_desc(mean)
        setattr(desc, field, value)
        cabi_run(hip, dev, mean, expect_rc=-2, desc=desc)
    # through the operator API, on host and on DMABUF tensors
    g = rc.descriptor(mean)["groups"]
    for device in (None, dev):
        for case, kw in ((mean, dict(out_shape=(2, 4))), (mean, dict(groups=(g[0], g[1], [8, 7], g[3]))),
                         (mean, dict(groups=(g[0], [-245, 49], g[2], g[3]))), (axis, dict(axis_count=2, axis=[3, 2])),
                         (axis, dict(axis_count=0)), (axis, dict(axis=[4])), (axis, dict(axis=[-2])), (axis, dict(out_shape=(2, 3, 5))),
                         (gmp, dict(out_shape=(2, 4, 1, 1)))):
            status, out = rc.layer_run(fe, pkg.API_MI355X, case, device=device, poison=POISON, **kw)
            assert status != pkg.CSINN_TRUE, kw
            assert np.all(out.view(np.uint8) == POISON), "a refused call wrote to the output: %r" % (kw,)
    # an output overlapping the input, on the device
    x = mean["x"]
    p = dev.alloc(4 * x.nbytes)
    dev.upload(p, np.full(4 * x.nbytes, POISON, np.uint8))
    desc = rc.cabi_desc(mean)
    assert hip.shl_mi355x_reduce(p, p + x.nbytes - 1, C.byref(desc), None) == -2 and b"overlaps the input" in hip.shl_mi355x_last_error()
    assert np.all(dev.download(p, (4 * x.nbytes,), np.uint8) == POISON)
    dev.free(p)


@pytest.mark.gpu
def test_no_outputs_is_ok_and_enqueues_nothing(gpu):
    _, hip, _, dev = gpu
    case = next(c for c in CASES if rc.golden_key(c) == "sum.row_3x64_i8")
    desc = rc.cabi_desc(case)
    desc.out_extent[0] = 0
    p = dev.alloc(256)
    dev.upload(p, np.full(256, POISON, np.uint8))
    assert hip.shl_mi355x_reduce(p, p + 192, C.byref(desc), None) == 0
    assert np.all(dev.download(p, (256,), np.uint8) == POISON)
    dev.free(p)

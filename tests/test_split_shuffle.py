"""Split and shuffle_channel on the GPU (-m gpu): every case of split_shuffle_cases through the C ABI on device buffers -- in
the form the rules choose and forced to every other form that accepts it, every output between poisoned guard bands --,
through csinn_split / csinn_shuffle_channel on host tensors (the packed staging path) and on DMABUF tensors, bit for bit
against the genuine library's golden outputs (binary16 compared on bits); a pointer off the 16-byte grid; what `perf`
reports; refusals that must write nothing."""
import ctypes as C

import numpy as np
import pytest

import cases
import split_shuffle_cases as ssc
from cases import pkg

CASES = ssc.all_cases()
IDS = ["%s-%s" % (c["op"], c["name"]) for c in CASES]
GOLD = ssc.golden()
POISON = 0x5A
GUARD = 64  # bytes of poison on each side of every output


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt, cases.HipDevice(hip)


def check(got, case, route):
    for key, g in zip(ssc.golden_keys(case), got):
        ssc.assert_same(g, GOLD[key], "%s, %s vs reference golden" % (key, route))


def out_shapes(case):
    return case["out_shapes"] if case["op"] == "split" else [case["x"].shape]


def cabi_run(hip, dev, case, in_skew=0, out_skew=None, want_form=None, expect_rc=0):
    """device buffers through the C ABI.  in_skew / out_skew[i]: that buffer starts so many BYTES further into its
    allocation.  Every output sits between GUARD bytes of poison on each side, which must stay; with expect_rc != 0 the
    outputs themselves are poisoned too and must stay."""
    x = case["x"]
    shapes = out_shapes(case)
    out_skew = out_skew or [0] * len(shapes)
    raw = np.full(x.nbytes + 64, POISON, np.uint8)
    raw[in_skew:in_skew + x.nbytes] = x.view(np.uint8).ravel()
    d_in = dev.alloc(raw.nbytes)
    dev.upload(d_in, raw)
    frames, ptrs = [], []
    for shape, skew in zip(shapes, out_skew):
        nbytes = int(np.prod(shape)) * x.itemsize
        frames.append(np.full(GUARD + skew + nbytes + GUARD, POISON, np.uint8))
        ptrs.append(dev.alloc(frames[-1].nbytes))
        dev.upload(ptrs[-1], frames[-1])
    args = ssc.cabi_args(case, [p + GUARD + s for p, s in zip(ptrs, out_skew)])
    if want_form is not None:
        assert args.name(hip, d_in + in_skew) == want_form
    rc = args.run(hip, d_in + in_skew)
    outs = []
    for p, frame, shape, skew in zip(ptrs, frames, shapes, out_skew):
        got = dev.download(p, frame.shape, np.uint8)
        lo, nbytes = GUARD + skew, int(np.prod(shape)) * x.itemsize
        assert np.all(got[:lo] == POISON) and np.all(got[lo + nbytes:] == POISON), "wrote outside an output"
        if expect_rc != 0:
            assert np.all(got == POISON), "a refused call wrote to an output"
        outs.append(got[lo:lo + nbytes].view(x.dtype).reshape(shape))
    for p in ptrs + [d_in]:
        dev.free(p)
    assert rc == expect_rc, (rc, hip.shl_mi355x_last_error())
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matches_the_reference_through_every_route(gpu, case, monkeypatch):
    fe, hip, _, dev = gpu
    env = ssc.FORM_ENV[case["op"]]
    monkeypatch.delenv(env, raising=False)
    natural = ssc.expected_form(case)
    check(cabi_run(hip, dev, case, want_form=natural), case, "C ABI, " + natural)
    names = []

    def perf(cb, t_in, outs, params):
        tp = C.POINTER(pkg.Tensor)
        sig = [tp, C.POINTER(tp) if case["op"] == "split" else tp, C.c_void_p, C.POINTER(C.c_char_p)]
        name = C.c_char_p()
        assert C.CFUNCTYPE(C.c_int, *sig)(cb.contents.perf)(t_in, outs, params, C.byref(name)) == pkg.CSINN_TRUE
        names.append(name.value.decode())
    check(ssc.layer_run(fe, pkg.API_MI355X, case, perf=perf), case, "operator API on host tensors")
    check(ssc.layer_run(fe, pkg.API_MI355X, case, device=dev, perf=perf), case, "operator API on DMABUF tensors")
    assert names == [natural, natural], "perf reports the launched form"
    # every other form that accepts the case, and the switch set to a form that does not (the literal form then)
    for force in ssc.other_forms(case):
        monkeypatch.setenv(env, force)
        form = ssc.forced_form(case, force)
        if form != natural:
            check(cabi_run(hip, dev, case, want_form=form), case, "C ABI, forced to " + force)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["form_i8_nhwc_16_32_48", "form_f16_nhwc_8_24", "records_one_differs", "nhwc_i8_c32_g4",
                                  "nchw_f16_2x4", "nhwc_i8_c116_g2"])
def test_a_pointer_off_the_grid_takes_the_literal_form(gpu, name, monkeypatch):
    """a vector-eligible case with one pointer offset by 4 bytes -- the input, and separately each output -- falls to
    generic (shuffle: to the 4-byte variant of its form) and still matches; everything 16 bytes in keeps the form"""
    _, hip, _, dev = gpu
    case = next(c for c in CASES if c["name"] == name)
    monkeypatch.delenv(ssc.FORM_ENV[case["op"]], raising=False)
    natural = ssc.expected_form(case)
    n = len(out_shapes(case))
    by4 = "split_generic" if case["op"] == "split" else natural.replace("_16", "_4")
    es = case["x"].itemsize
    by_one = natural.split("_")[0] + "_generic"
    check(cabi_run(hip, dev, case, in_skew=4, want_form=by4), case, "input 4 bytes in")
    check(cabi_run(hip, dev, case, in_skew=es, want_form=by_one), case, "input one element in")
    for i in range(n):
        check(cabi_run(hip, dev, case, out_skew=[4 if j == i else 0 for j in range(n)], want_form=by4), case,
              "output %d 4 bytes in" % i)
    check(cabi_run(hip, dev, case, out_skew=[es] + [0] * (n - 1), want_form=by_one), case, "output 0 one element in")
    check(cabi_run(hip, dev, case, in_skew=16, out_skew=[16] * n, want_form=natural), case, "everything 16 bytes in")


@pytest.mark.gpu
def test_refused_arguments_fail_and_write_nothing(gpu):
    fe, hip, _, dev = gpu
    split = next(c for c in CASES if c["name"] == "records_one_differs")
    shuf = next(c for c in CASES if c["name"] == "nhwc_i8_c32_g4")
    # through the C ABI: what only it can be handed
    cabi_run(hip, dev, dict(split, lens=[16, 0, 48]), expect_rc=-2)
    cabi_run(hip, dev, dict(split, lens=[16, -16, 64]), expect_rc=-2)
    cabi_run(hip, dev, dict(shuf, group=5), expect_rc=-2)
    cabi_run(hip, dev, dict(shuf, group=0), expect_rc=-2)
    # through the operator API, on host and on DMABUF tensors
    wrong = [(1, 3, 3, 16), (1, 3, 3, 32), (1, 3, 3, 16)]
    for device in (None, dev):
        for case, kw in ((split, dict(out_shapes=wrong)), (split, dict(axis=4)), (split, dict(axis=2)), (split, dict(count=0)),
                         (split, dict(index=[16, 16])), (split, dict(index=[32, 16])), (split, dict(index=[16, 80])),
                         (split, dict(in_scales=(0.5, 0.25))), (split, dict(out_dt=pkg.DTYPE_FLOAT32)),
                         (shuf, dict(group=5)), (shuf, dict(group=0)), (shuf, dict(out_shapes=[(1, 5, 3, 32)])),
                         (shuf, dict(in_scales=(0.5,) * 32))):
            rc, outs = ssc.layer_run(fe, pkg.API_MI355X, case, device=device, poison=POISON, **kw)
            assert rc != pkg.CSINN_TRUE, kw
            for o in outs:
                assert np.all(o.view(np.uint8) == POISON), "a refused call wrote to an output: %r" % (kw,)
    # an output overlapping the input, on the device
    x = split["x"]
    p = dev.alloc(4 * x.nbytes)
    dev.upload(p, np.full(4 * x.nbytes, POISON, np.uint8))
    args = ssc.SplitArgs(split, [p + 2 * x.nbytes, p + x.nbytes - 1, p + 3 * x.nbytes])
    assert args.run(hip, p) == -2 and b"overlaps the input" in hip.shl_mi355x_last_error()
    sargs = ssc.ShuffleArgs(shuf, [p + shuf["x"].nbytes - 1])
    assert sargs.run(hip, p) == -2 and b"overlaps the input" in hip.shl_mi355x_last_error()
    assert np.all(dev.download(p, (4 * x.nbytes,), np.uint8) == POISON)
    dev.free(p)


@pytest.mark.gpu
def test_fp16_with_a_scale_other_than_one_is_refused(gpu):
    fe, _, _, dev = gpu
    split = next(c for c in CASES if c["name"] == "form_f16_nhwc_8_24")
    shuf = next(c for c in CASES if c["name"] == "nhwc_f16_c8_g2")
    for case in (dict(split, out_qs=[(1.0, 0), (0.5, 0)]), dict(split, in_q=(2.0, 0)), dict(shuf, out_q=(0.5, 0))):
        rc, outs = ssc.layer_run(fe, pkg.API_MI355X, case, device=dev, poison=POISON)
        assert rc != pkg.CSINN_TRUE and all(np.all(o.view(np.uint8) == POISON) for o in outs)

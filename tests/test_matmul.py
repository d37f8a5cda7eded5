"""matmul on the GPU (-m gpu): every case of matmul_cases through the C ABI on device buffers, the output between poisoned
guard bands, and through csinn_matmul on host tensors (the staging path) and on DMABUF tensors.
  SHL_MI355X_MATMUL_FORM=chain   zero differing bytes against the genuine library's golden outputs (binary16 compared on bits)
  SHL_MI355X_MATMUL_FORM=mfma    int8: zero differing bytes against exact_ref always; against the golden zero where the
                                 plan-time proof holds, else within DESIGN's gate (1 LSB, max(2, 2e-4 n) outputs).  binary16:
                                 zero on the exact-sum stratum, within 1e-3 on the non-negative one
  the default rule               the kernel name says which form runs, the result obeys that form's contract
and the refusals, which must write nothing.  No test hands a kernel an out-of-bounds shape: refusals are checks of the
validation path."""
import ctypes as C

import numpy as np
import pytest

import cases
import matmul_cases as mc
from cases import pkg

CASES = mc.all_cases()
IDS = [mc.case_id(c) for c in CASES]
GOLD = mc.golden()
POISON = 0x5A
GUARD = 64  # bytes of poison on each side of the output
FORM_ENV = "SHL_MI355X_MATMUL_FORM"
_EXACT = {}


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt, cases.HipDevice(hip)


def golden_of(case):
    g = GOLD[mc.golden_key(case)].reshape(case["out_shape"])
    return g.view(np.float16) if case["dtype"] == "f16" else g


def exact_of(case):
    if case["name"] not in _EXACT:
        _EXACT[case["name"]] = mc.exact_ref(case)
    return _EXACT[case["name"]]


def check(got, case, form, route):
    """the contract of `form`"""
    what = "%s, %s, %s" % (mc.case_id(case), form, route)
    want = golden_of(case)
    if form == pkg.MATMUL_CHAIN:
        mc.assert_same(got, want, what + " vs reference golden")
    elif case["dtype"] == "int8":
        mc.assert_same(got, exact_of(case), what + " vs exact_ref")
        if mc.is_exact(case):
            mc.assert_same(got, want, what + " vs reference golden (the proof holds)")
        else:
            mc.assert_within_gate(got, want, what + " vs reference golden")
    elif case["regime"] == "exact":
        mc.assert_same(got, want, what + " vs reference golden (exact sums)")
    else:
        mc.assert_f16_gate(got, want, what + " vs reference golden")


def cabi_run(hip, dev, case, want_form=None, expect_rc=0, desc=None, out_skew=0):
    """device buffers through the C ABI.  The output sits between GUARD bytes of poison on each side, which must stay; with
    expect_rc != 0 the output itself is poisoned too and must stay"""
    a, b = case["a"], case["b"]
    nbytes = int(np.prod(case["out_shape"])) * a.itemsize
    d_a, d_b = dev.alloc(a.nbytes), dev.alloc(b.nbytes)
    dev.upload(d_a, a)
    dev.upload(d_b, b)
    frame = np.full(GUARD + out_skew + nbytes + GUARD, POISON, np.uint8)
    d_out = dev.alloc(frame.nbytes)
    dev.upload(d_out, frame)
    desc = desc or mc.cabi_desc(case)
    out = d_out + GUARD + out_skew
    if want_form is not None:
        assert hip.shl_mi355x_matmul_kernel_name(d_a, d_b, out, C.byref(desc)).decode() == want_form
    status = hip.shl_mi355x_matmul(d_a, d_b, out, C.byref(desc), None)
    got = dev.download(d_out, frame.shape, np.uint8)
    for p in (d_out, d_b, d_a):
        dev.free(p)
    lo = GUARD + out_skew
    assert np.all(got[:lo] == POISON) and np.all(got[lo + nbytes:] == POISON), "wrote outside the output"
    if expect_rc != 0:
        assert np.all(got == POISON), "a refused call wrote to the output"
    assert status == expect_rc, (status, hip.shl_mi355x_last_error())
    return got[lo:lo + nbytes].view(a.dtype).reshape(case["out_shape"])


def perf_name(names):
    def perf(cb, t_a, t_b, t_o, params):
        tp = C.POINTER(pkg.Tensor)
        name = C.c_char_p()
        fn = C.CFUNCTYPE(C.c_int, tp, tp, tp, C.c_void_p, C.POINTER(C.c_char_p))(cb.contents.perf)
        assert fn(t_a, t_b, t_o, params, C.byref(name)) == pkg.CSINN_TRUE
        names.append(name.value.decode())
    return perf


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_form_keeps_its_contract_through_every_route(gpu, case, monkeypatch):
    fe, hip, _, dev = gpu
    desc = mc.cabi_desc(case)
    assert bool(hip.shl_mi355x_matmul_is_exact(C.byref(desc))) == mc.is_exact(case), "the C proof and its restatement disagree"
    forces = ["chain", None] if case["regime"] == "special" else ["chain", "mfma", None]
    for force in forces:
        if force is None:
            monkeypatch.delenv(FORM_ENV, raising=False)
        else:
            monkeypatch.setenv(FORM_ENV, force)
        form = mc.expected_form(case, force)
        if case["regime"] == "special":
            assert form == pkg.MATMUL_CHAIN, "the special rows are small enough for the default rule to take the chain"
        names = []
        check(cabi_run(hip, dev, case, want_form=form), case, form, "C ABI")
        check(mc.layer_run(fe, pkg.API_MI355X, case, perf=perf_name(names)), case, form, "csinn_matmul on host tensors")
        check(mc.layer_run(fe, pkg.API_MI355X, case, device=dev, perf=perf_name(names)), case, form, "csinn_matmul on DMABUF tensors")
        assert names == [form, form], "perf reports the launched form"


ODD = [c for c in CASES if c["name"].startswith(("odd_", "m33_", "n65_", "k130_", "dense_2x"))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ODD, ids=[mc.case_id(c) for c in ODD])
def test_output_off_the_16_byte_grid(gpu, case, monkeypatch):
    """the output 1, 2 and 3 elements into its allocation: both forms store by element, the guard bands stay"""
    _, hip, _, dev = gpu
    for force in ("chain", "mfma"):
        monkeypatch.setenv(FORM_ENV, force)
        form = mc.expected_form(case, force)
        for elems in (1, 2, 3):
            check(cabi_run(hip, dev, case, want_form=form, out_skew=elems * case["a"].itemsize), case, form, "output %d elements in" % elems)


@pytest.mark.gpu
def test_a_constant_second_operand(gpu, monkeypatch):
    """mat1 as a constant tensor in layer mode: uploaded by the staging path like an activation"""
    fe, _, _, dev = gpu
    monkeypatch.delenv(FORM_ENV, raising=False)
    for key in ("dense_2x33x65x31_i8", "dense_2x33x65x31_f16", "k64_t00_i8"):
        case = next(c for c in CASES if c["name"] == key)
        check(mc.layer_run(fe, pkg.API_MI355X, case, b_const=True), case, mc.expected_form(case), "constant mat1")


@pytest.mark.gpu
def test_refused_arguments_fail_and_write_nothing(gpu, monkeypatch):
    fe, hip, _, dev = gpu
    monkeypatch.delenv(FORM_ENV, raising=False)
    by = {c["name"]: c for c in CASES}
    case = by["dense_2x33x65x31_i8"]
    # through the C ABI: what only it can be handed
    for field, value in (("m", 0), ("n", -1), ("k", 0), ("batches", 0), ("dtype", 7), ("a_row_stride", -65), ("b_k_stride", -1),
                         ("a_elems", 1 << 31), ("b_elems", 1 << 31), ("out_elems", 1 << 31), ("out_elems", case["a"].size),
                         ("a_elems", case["a"].size - 1), ("b_elems", case["b"].size - 1), ("b_batch_stride", 1),
                         ("a_k_stride", 2), ("a_elems", 0)):
        desc = mc.cabi_desc(case)
        setattr(desc, field, value)
        cabi_run(hip, dev, case, expect_rc=-2, desc=desc)
        assert hip.shl_mi355x_last_error().startswith(b"matmul: ")
    # through the operator API, on host and on DMABUF tensors: the broadcasts the reference refuses, operands that disagree on
    # K, an output tensor of another size
    rng = np.random.default_rng(5)
    wide_b = dict(case, name="b_has_more_batches", a=case["a"][0], b=rng.integers(-128, 128, (2, 65, 31), dtype=np.int8), out_shape=(2, 33, 31))
    other_k = dict(case, name="k_differs", b=rng.integers(-128, 128, (64, 31), dtype=np.int8))
    square = by["dense_3x64x64x64_i8"]
    for device in (None, dev):
        for c, kw in ((wide_b, {}), (other_k, {}), (square, dict(trans_b=True)), (square, dict(trans_a=True)),
                      (case, dict(out_shape=(2, 33, 30))), (case, dict(out_shape=(33, 31)))):
            status, out = mc.layer_run(fe, pkg.API_MI355X, c, device=device, poison=POISON, **kw)
            assert status != pkg.CSINN_TRUE, (c["name"], kw)
            assert np.all(out.view(np.uint8) == POISON), "a refused call wrote to the output: %s %r" % (c["name"], kw)
    # an output overlapping an operand, on the device
    a = case["a"]
    p = dev.alloc(4 * a.nbytes)
    dev.upload(p, np.full(4 * a.nbytes, POISON, np.uint8))
    desc = mc.cabi_desc(case)
    assert hip.shl_mi355x_matmul(p, p + 2 * a.nbytes, p + a.nbytes - 1, C.byref(desc), None) == -2
    assert b"overlaps an operand" in hip.shl_mi355x_last_error()
    assert hip.shl_mi355x_matmul(p + 2 * a.nbytes, p, p + case["b"].nbytes - 1, C.byref(desc), None) == -2
    assert np.all(dev.download(p, (4 * a.nbytes,), np.uint8) == POISON)
    dev.free(p)

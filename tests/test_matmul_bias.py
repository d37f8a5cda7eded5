"""matmul + add of a constant bias as one launch (shl_mi355x_matmul_bias) on the GPU (-m gpu): against the device's own
shl_mi355x_matmul followed by shl_mi355x_add_bcast, bit for bit, in int8 and binary16, each form forced, at the tile and slab
edges, with both transposes and the dense broadcast, under converter records, power-of-two records and an intermediate record
that saturates, on binary16 operands that make NaN and inf intermediates; and, where the plan-time proof holds (binary16:
where every sum is exact), against the oracle chain -- matmul_cases.chain_ref, then the numpy add."""
import ctypes as C
import math

import numpy as np
import pytest

import add_bcast_cases
import cases
import matmul_cases as mc
from cases import pkg
from pool_cases import _q

# (batches, M, N, K) at the edges of the 64 x 64 tile and the 64-byte slab of K; trans_a, trans_b, dense: one B for every batch
SHAPES = [
    ("1x1x1x1", 1, 1, 1, 1, 0, 0, False),
    ("1x17x64x64", 1, 17, 64, 64, 0, 0, False),
    ("3x65x33x70", 3, 65, 33, 70, 0, 0, False),
    ("2x64x130x16", 2, 64, 130, 16, 0, 0, False),
    ("1x63x65x129", 1, 63, 65, 129, 0, 0, False),
    ("3x65x33x70_t11", 3, 65, 33, 70, 1, 1, False),
    ("3x65x33x70_dense", 3, 65, 33, 70, 0, 0, True),
    ("2x64x130x16_t01", 2, 64, 130, 16, 0, 1, False),
    ("2x64x130x16_t10", 2, 64, 130, 16, 1, 0, False),
    ("2x64x130x16_dense", 2, 64, 130, 16, 0, 0, True),
]
FORMS = ("chain", "mfma")
POISON = 0x5A


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return hip, cases.HipDevice(hip)


def records(regime, k):
    """(a, b, intermediate, bias, output) records.  The intermediate's scale follows the spread of the sums of random data
    (matmul_cases.out_record); `sat` divides it by 24, so that most intermediates clamp at -128 / 127 and the clamped value is
    what the bias is added to"""
    if regime == "conv":
        a_q, b_q = _q(0.0473, -9), _q(0.0219, 4)
    else:
        a_q, b_q = _q(2.0 ** -4, -5), _q(2.0 ** -6, 3)
    spread = 74.0 * 74.0 * math.sqrt(k) * a_q[0] * b_q[0] / 40.0
    if regime == "conv":
        mid, bias, out = _q(spread, 3), _q(0.7 * spread, 11), _q(1.7 * spread, -20)
    else:
        s = 2.0 ** round(math.log2(spread))
        if regime == "sat":
            mid, bias, out = _q(s / 32, 100), _q(s / 16, -7), _q(s / 8, 9)
        else:
            mid, bias, out = _q(s, 5), _q(s / 2, -7), _q(2 * s, 9)
    return a_q, b_q, mid, bias, out


def make_case(name, dtype, batches, m, n, k, ta, tb, dense, regime):
    rng = mc._rng("matmul_bias %s %s %s" % (name, dtype, regime))
    sa = (batches,) + ((k, m) if ta else (m, k))
    sb = (() if dense else (batches,)) + ((n, k) if tb else (k, n))
    c = dict(name=name, dtype=dtype, trans_a=bool(ta), trans_b=bool(tb), m=m, n=n, k=k, batches=batches, out_shape=(batches, m, n))
    if dtype == "f16":
        c["a"], c["b"] = mc._f16_data(rng, sa, "exact"), mc._f16_data(rng, sb, "exact")  # every partial sum is exact in either order
        c["bias"] = mc._f16_data(rng, (n,), "exact")
        c["a_q"] = c["b_q"] = c["mid_q"] = c["bias_q"] = c["out_q"] = _q(1.0, 0)
    else:
        c["a"], c["b"] = rng.integers(-128, 128, sa, dtype=np.int8), rng.integers(-128, 128, sb, dtype=np.int8)
        c["bias"] = rng.integers(-128, 128, (n,), dtype=np.int8)
        c["a_q"], c["b_q"], c["mid_q"], c["bias_q"], c["out_q"] = records(regime, k)
    return c


def desc_of(case, out_q):
    return pkg.matmul_desc(pkg.SHL_I8 if case["dtype"] == "int8" else pkg.SHL_F16, case["a"].shape, case["b"].shape, case["trans_a"],
                           case["trans_b"], case["a_q"], case["b_q"], out_q)


def run_both(hip, dev, case, bias_first, want_form):
    """(the fused launch's output, matmul then add_bcast's, the intermediate), all from the device; bytes around the fused output
    are poisoned and must stay"""
    out_elems = int(np.prod(case["out_shape"]))
    es = case["a"].itemsize
    bufs = {}
    for key in ("a", "b", "bias"):
        bufs[key] = dev.alloc(case[key].nbytes)
        dev.upload(bufs[key], case[key])
    frame = np.full(out_elems * es + 128, POISON, np.uint8)
    for key in ("mid", "pair", "fused"):
        bufs[key] = dev.alloc(frame.nbytes)
        dev.upload(bufs[key], frame)
    p_fused = bufs["fused"] + 64
    d_mid, d_out = desc_of(case, case["mid_q"]), desc_of(case, case["out_q"])
    assert hip.shl_mi355x_matmul_kernel_name(bufs["a"], bufs["b"], bufs["mid"], C.byref(d_mid)).decode() == "matmul_" + want_form
    pkg.check(hip.shl_mi355x_matmul(bufs["a"], bufs["b"], bufs["mid"], C.byref(d_mid), None), hip, "shl_mi355x_matmul")
    add = add_bcast_cases.add_desc(dict(dtype=case["dtype"], in_q=case["mid_q"], in1_q=case["bias_q"], out_q=case["out_q"],
                                        small_first=bias_first), (out_elems // case["n"], case["n"]), (case["n"],))
    pkg.check(hip.shl_mi355x_add_bcast(bufs["mid"], bufs["bias"], bufs["pair"], C.byref(add), None), hip, "shl_mi355x_add_bcast")
    name = hip.shl_mi355x_matmul_bias_kernel_name(bufs["a"], bufs["b"], bufs["bias"], p_fused, C.byref(d_out)).decode()
    assert name == "matmul_%s_bias" % want_form
    pkg.check(hip.shl_mi355x_matmul_bias(bufs["a"], bufs["b"], bufs["bias"], p_fused, C.byref(d_out), case["bias_q"][0], case["bias_q"][1],
                                         case["mid_q"][0], case["mid_q"][1], 1 if bias_first else 0, None), hip, "shl_mi355x_matmul_bias")
    got = dev.download(bufs["fused"], frame.shape, np.uint8)
    assert np.all(got[:64] == POISON) and np.all(got[64 + out_elems * es:] == POISON), "wrote outside the output"
    view = lambda raw: raw.view(case["a"].dtype)[:out_elems].reshape(case["out_shape"])
    fused = view(got[64:64 + out_elems * es].copy())
    pair = view(dev.download(bufs["pair"], frame.shape, np.uint8)[:out_elems * es].copy())
    mid = view(dev.download(bufs["mid"], frame.shape, np.uint8)[:out_elems * es].copy())
    for p in bufs.values():
        dev.free(p)
    return fused, pair, mid


def oracle_chain(case, bias_first):
    mid = mc.chain_ref(dict(case, out_q=case["mid_q"]))
    return add_bcast_cases.add_numpy(dict(dtype=case["dtype"], x=mid, y=case["bias"], in_q=case["mid_q"], in1_q=case["bias_q"],
                                          out_q=case["out_q"], small_first=bias_first))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_int8_fused_equals_matmul_then_add(gpu, shape, form, monkeypatch):
    hip, dev = gpu
    monkeypatch.setenv("SHL_MI355X_MATMUL_FORM", form)
    monkeypatch.delenv("SHL_MI355X_ADD_FORM", raising=False)
    for regime in ("conv", "pow2", "sat"):
        case = make_case(shape[0], "int8", *shape[1:], regime)
        exact = hip.shl_mi355x_matmul_is_exact(C.byref(desc_of(case, case["mid_q"])))
        assert exact == (0 if regime == "conv" else 1) and bool(exact) == mc.is_exact(case), regime
        for bias_first in (False, True):
            what = "%s %s %s bias_first=%d" % (shape[0], form, regime, bias_first)
            fused, pair, mid = run_both(hip, dev, case, bias_first, form)
            mc.assert_same(fused, pair, what + ": fused vs matmul then add_bcast")
            if exact:  # inside the proof either form is the reference's chain, and so is the fused launch
                mc.assert_same(fused, oracle_chain(case, bias_first), what + ": fused vs the oracle chain")
        if regime == "sat" and mid.size >= 64:
            clamped = np.count_nonzero((mid == 127) | (mid == -128))
            assert clamped > mid.size // 2, "the saturating record must clamp most intermediates (%d of %d)" % (clamped, mid.size)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_f16_fused_equals_matmul_then_add(gpu, shape, form, monkeypatch):
    hip, dev = gpu
    monkeypatch.setenv("SHL_MI355X_MATMUL_FORM", form)
    monkeypatch.delenv("SHL_MI355X_ADD_FORM", raising=False)
    case = make_case(shape[0], "f16", *shape[1:], "f16")
    for bias_first in (False, True):
        what = "%s %s f16 bias_first=%d" % (shape[0], form, bias_first)
        fused, pair, _ = run_both(hip, dev, case, bias_first, form)
        mc.assert_same(fused, pair, what + ": fused vs matmul then add_bcast")
        mc.assert_same(fused, oracle_chain(case, bias_first), what + ": fused vs the oracle chain (every sum is exact)")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_f16_nan_and_inf_intermediates_go_through_the_adds_rules(gpu, form, monkeypatch):
    """rows of A that make NaN (either sign), inf, inf + -inf and saturating intermediates, a bias with NaNs of both signs and
    both infinities: the fused launch hands on what matmul followed by add hands on, the bias on either side of the add"""
    hip, dev = gpu
    monkeypatch.setenv("SHL_MI355X_MATMUL_FORM", form)
    monkeypatch.delenv("SHL_MI355X_ADD_FORM", raising=False)
    m, n, k = 8, 16, 70
    rng = mc._rng("matmul_bias specials")
    a = rng.uniform(0.5, 2.0, (1, m, k)).astype(np.float16)
    b = rng.uniform(0.5, 2.0, (1, k, n)).astype(np.float16)
    au = a.view(np.uint16)
    au[0, 0, 4] = mc.NAN_P
    au[0, 1, 2] = mc.INF_P
    au[0, 2, 1], au[0, 2, 66] = mc.INF_P, mc.INF_N
    au[0, 3, 8] = mc.NAN_N
    au[0, 4, 3] = mc.INF_N
    a[0, 5, :] = 60000.0
    a[0, 6, :] = -60000.0
    bias = rng.uniform(-2.0, 2.0, (n,)).astype(np.float16)
    bias.view(np.uint16)[:6] = (mc.NAN_P, mc.NAN_N, mc.INF_P, mc.INF_N, 0x7BFF, 0xFBFF)
    one = _q(1.0, 0)
    case = dict(name="specials", dtype="f16", trans_a=False, trans_b=False, m=m, n=n, k=k, batches=1, out_shape=(1, m, n), a=a, b=b,
                bias=bias, a_q=one, b_q=one, mid_q=one, bias_q=one, out_q=one)
    seen = set()
    for bias_first in (False, True):
        fused, pair, mid = run_both(hip, dev, case, bias_first, form)
        mc.assert_same(fused, pair, "specials %s bias_first=%d: fused vs matmul then add_bcast" % (form, bias_first))
        seen |= set(mid.view(np.uint16).ravel().tolist())
        out = fused.view(np.uint16)
        assert {0x7FFF, 0xFFFF} <= set(out.ravel().tolist())
        # an infinite intermediate is stored as +-65504 (the reference's conversion), so only the bias's infinities meet it
        assert out[0, 7, 2] == 0x7BFF and out[0, 7, 3] == 0xFBFF
    assert {0x7BFF, 0xFBFF} <= seen and seen & {0x7FFF, 0xFFFF}, "the intermediates must hold NaNs and both saturations"
    if form == "chain":  # (the chain restates which NaN x86 hands on; the matrix cores' NaNs carry this device's sign)
        assert {0x7FFF, 0xFFFF} <= seen


@pytest.mark.gpu
def test_default_rule_names_the_bias_forms_and_refusals_write_nothing(gpu, monkeypatch):
    hip, dev = gpu
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM", raising=False)
    for shape in SHAPES[:5]:
        case = make_case(shape[0], "int8", *shape[1:], "pow2")
        fused, pair, _ = run_both(hip, dev, case, False, mc.expected_form(case).replace("matmul_", ""))
        mc.assert_same(fused, pair, shape[0] + ", the default rule")
    case = make_case("refusals", "int8", 1, 17, 64, 64, 0, 0, False, "pow2")
    d = desc_of(case, case["out_q"])
    p = dev.alloc(8192)
    dev.upload(p, np.full(8192, POISON, np.uint8))
    a, b, out = p, p + 2048, p + 6144   # a: 1088 bytes, b: 4096, out: 1088
    rec = (case["bias_q"][0], case["bias_q"][1], case["mid_q"][0], case["mid_q"][1], 0, None)
    for bias, text in ((None, b"NULL"), (out + 1087, b"overlaps the bias"), (out - 63, b"overlaps the bias")):
        assert hip.shl_mi355x_matmul_bias(a, b, bias, out, C.byref(d), *rec) == -2 and text in hip.shl_mi355x_last_error()
        assert hip.shl_mi355x_matmul_bias_kernel_name(a, b, bias, out, C.byref(d)) == b""
    assert hip.shl_mi355x_matmul_bias(a, b, p + 7300, a + 100, C.byref(d), *rec) == -2 and b"overlaps an operand" in hip.shl_mi355x_last_error()
    assert hip.shl_mi355x_matmul_bias_kernel_name(a, b, out - 64, out, C.byref(d)) == b"matmul_mfma_bias"
    assert np.all(dev.download(p, (8192,), np.uint8) == POISON)
    dev.free(p)

"""The fused attention core with a bias or mask on the scores (shl_mi355x_attention_bias) on the GPU (-m gpu): against the
device's own shl_mi355x_matmul (mfma form) -> [shl_mi355x_mul] -> shl_mi355x_add_bcast -> shl_mi355x_softmax -> shl_mi355x_matmul
(mfma form) on the same device buffers, bit for bit, in int8 and binary16, over attention_bias_cases.all_cases(), guard bands
around the output.  The unfused calls' own intermediates are read back, as the sweeps do, to show that a case exercises what its
name says: the sum equals the add's numpy restatement, the masks saturate, the far record takes the hardware's division, the
special values arrive in the softmax's input.  And the refusals, each with its code, its message and the kernel name ""."""
import ctypes as C

import numpy as np
import pytest

import add_bcast_cases
import attention_bias_cases as abc
import attention_cases as ac
import cases
import matmul_cases as mc
from cases import pkg

CASES = abc.all_cases()
IDS = [abc.case_id(c) for c in CASES]
POISON = abc.POISON
EINVAL, ENOTSUP = -2, -3
NEG_MAX = 0xFBFF  # -65504


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return hip, cases.HipDevice(hip)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_equals_the_unfused_calls(gpu, case, monkeypatch):
    hip, dev = gpu
    for var in ("SHL_MI355X_MATMUL_FORM", "SHL_MI355X_MUL_FORM", "SHL_MI355X_ADD_FORM", "SHL_MI355X_SOFTMAX_SEQ"):
        monkeypatch.delenv(var, raising=False)
    name = abc.case_id(case)
    fused, chain, total, x_in, p = abc.run_both(hip, dev, case)
    mc.assert_same(fused, chain, name + ": fused vs matmul, [mul], add, softmax, matmul")
    # the unfused sum is the add the case describes (so the fused launch, which equals the chain, has added that bias)
    bias4 = case["bias"].reshape((1,) * (4 - case["bias"].ndim) + case["bias"].shape)
    want = add_bcast_cases.add_numpy(dict(dtype=case["dtype"], x=x_in.reshape(abc.B0, abc.B1, case["s"], case["t"]), y=bias4,
                                          in_q=abc.x_record(case), in1_q=case["b_q"], out_q=case["sb_q"], small_first=case["bias_first"]))
    mc.assert_same(total.reshape(want.shape), want, name + ": the unfused sum vs the add's restatement")
    assert not np.array_equal(mc.bits(total), mc.bits(x_in)), "the bias must change the softmax's input"
    index = abc.index_map(case)
    flat = case["bias"].reshape(-1)
    if case["dtype"] == "int8":
        assert abc.fma_div(case) == (case["kind"] != "far")
        if case["kind"] == "mask":
            masked = flat[index] == -128
            assert masked.any() and np.all(total[masked] == -128), "a masked key must saturate the sum"
            assert np.unique(total[~masked]).size > 8
        if case["kind"] == "far":
            kept = flat[index] == case["b_q"][1]
            assert kept.any() and (~kept).any()
            assert np.all((total[~kept] == -128) | (total[~kept] == 127)) and np.unique(total[kept]).size > 8
    elif case["kind"] == "special":
        bits, bb = mc.bits(total), mc.bits(flat)[index]
        # the reference's float32 -> binary16 conversion saturates: a sum of -inf is stored as -65504, a masked key weighs nothing
        finite = (mc.bits(x_in)[:, :, 5] & 0x7C00) != 0x7C00
        assert finite.sum() > finite.size // 2 and np.all(bits[:, :, 5][finite] == NEG_MAX), "a masked column of finite scores is -65504"
        some_left = finite & ~np.all(bits == NEG_MAX, axis=2) & ~_nan(bits).any(axis=2)  # (a NaN in a row takes all of its p)
        assert np.all(mc.bits(p)[:, :, 5][some_left] == 0)
        assert np.all(bits[1, 4, :] == NEG_MAX), "a row with every key masked"
        assert np.unique(mc.bits(p)[1, 4, :]).size == 1, "... weighs its keys alike"
        nan_row = ac.SPECIAL_ROWS[1]
        assert _nan(mc.bits(x_in)[0, nan_row, :]).all()
        # of two NaNs the add layer's second input's goes through, with its own sign
        second = bb[0, nan_row, :3] if not case["bias_first"] else mc.bits(x_in)[0, nan_row, :3]
        assert np.array_equal(bits[0, nan_row, :3], 0x7FFF | (second & 0x8000))
        # (a stored score is never infinite -- the products saturate too --, so inf + -inf cannot meet inside the chain: the
        # infinities of the bias decide the sums of the row whose scores are +-65504)
        inf_row, inf_x = bits[0, ac.SPECIAL_ROWS[0], :9], mc.bits(x_in)[0, ac.SPECIAL_ROWS[0], :9]
        for col, want_bits in ((0, NEG_MAX), (2, NEG_MAX), (1, 0x7BFF), (3, 0x7BFF)):
            assert _nan(inf_x[col:col + 1]).any() or inf_row[col] == want_bits
        assert (bb == abc.NEG_ZERO).any() and (bb == abc.POS_INF).any()
    if case["kind"] != "special":
        assert np.unique(mc.bits(fused)).size > 8, "the output would tell nothing"


def _nan(bits):
    return (bits & 0x7FFF) > 0x7C00


@pytest.mark.gpu
def test_refusals_name_no_kernel_and_write_nothing(gpu, monkeypatch):
    hip, dev = gpu
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM", raising=False)
    base = next(c for c in CASES if c["name"] == "bias_h_s_t_s33_t65_f16")
    room = dev.alloc(1 << 20)
    dev.upload(room, np.full(1 << 20, POISON, np.uint8))
    step = 1 << 17  # (every tensor of the case is smaller)
    q, k, v, bias, out = (room + i * step for i in range(5))

    def refused(d, bd, ptrs, code, text):
        dref, bref = C.byref(d), (C.byref(bd) if bd is not None else None)
        status = hip.shl_mi355x_attention_bias(*ptrs, dref, bref, None)
        assert status == code, (text, status, hip.shl_mi355x_last_error())
        assert text.encode() in hip.shl_mi355x_last_error(), (text, hip.shl_mi355x_last_error())
        assert hip.shl_mi355x_attention_bias_kernel_name(*ptrs, dref, bref) == b""
        assert hip.shl_mi355x_attention_bias_by_default(*ptrs, dref, bref) == 0
    ok, okb = ac.desc(base), abc.bias_desc(hip, base)
    ptrs = (q, k, v, bias, out)
    assert hip.shl_mi355x_attention_bias_kernel_name(*ptrs, C.byref(ok), C.byref(okb)) == pkg.ATTENTION_BIAS_MFMA.encode()
    refused(ok, None, ptrs, EINVAL, "NULL argument")
    refused(ok, okb, (q, k, v, None, out), EINVAL, "NULL argument")
    refused(ok, okb, (q, k, v, bias + 1, out), EINVAL, "not aligned")
    refused(ok, okb, (q + 1, k, v, bias, out), EINVAL, "not aligned")
    refused(ok, okb, (q, k, v, out + 64, out), EINVAL, "overlaps the bias")
    refused(ok, okb, (q, k, v, bias, k), EINVAL, "overlaps an operand")
    for field, value, text in (("b_ext1", 0, "b_ext1"), ("b_ext1", 4, "b_ext1"), ("bias_is_first", 2, "bias_is_first"),
                               ("row_stride", -1, "negative"), ("key_stride", -1, "negative"), ("key_stride", 1 << 31, "2^31"),
                               ("row_stride", 1 << 27, "2^31")):
        bd = abc.bias_desc(hip, base)
        setattr(bd, field, value)
        refused(ok, bd, ptrs, EINVAL, text)
    for i in range(2):
        bd = abc.bias_desc(hip, base)
        bd.b_stride[i] = -5
        refused(ok, bd, ptrs, EINVAL, "negative")
    bd = abc.bias_desc(hip, base)
    bd.reserved[2] = 1
    refused(ok, bd, ptrs, EINVAL, "reserved")
    d = ac.desc(base)
    d.t = ac.CAP + 1
    refused(d, okb, ptrs, EINVAL, "SHL_MI355X_ATTENTION_MAX_KEYS")
    d = ac.desc(base)
    d.batches, d.s, d.t, d.d, d.dv = 2, 17, 17, 32, 32  # the chain form's
    bd = abc.bias_desc(hip, base)
    bd.b_ext1 = 2
    refused(d, bd, ptrs, ENOTSUP, "chain form")
    monkeypatch.setenv("SHL_MI355X_MATMUL_FORM", "chain")
    refused(ok, okb, ptrs, ENOTSUP, "chain form")
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM")
    assert np.all(dev.download(room, (1 << 20,), np.uint8) == POISON)
    dev.free(room)

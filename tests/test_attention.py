"""The fused attention core (shl_mi355x_attention) on the GPU (-m gpu): against the device's own shl_mi355x_matmul (mfma form)
-> shl_mi355x_mul -> shl_mi355x_softmax -> shl_mi355x_matmul (mfma form) on the same device buffers, bit for bit, in int8 and
binary16, over attention_cases.all_cases(); against the oracle chain -- int8 bit for bit where the plan-time proof holds for
both products, inside DESIGN's gate elsewhere (the case at the cap cannot satisfy the proof), binary16 inside the 1e-3 gate --;
and the refusals, each with its code, its message and the kernel name ""."""
import ctypes as C

import numpy as np
import pytest

import attention_cases as ac
import cases
import matmul_cases as mc
from attention_cases import run_both
from cases import pkg

CASES = ac.all_cases()
IDS = [ac.case_id(c) for c in CASES]
POISON = ac.POISON
EINVAL, ENOTSUP = -2, -3


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return hip, cases.HipDevice(hip)


@pytest.fixture(scope="module")
def oracle():
    """the oracle chain of every case, computed once"""
    return {c["name"]: ac.oracle_chain(c) for c in CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_equals_the_unfused_calls_and_the_oracle_chain(gpu, oracle, case, monkeypatch):
    hip, dev = gpu
    for var in ("SHL_MI355X_MATMUL_FORM", "SHL_MI355X_MUL_FORM", "SHL_MI355X_SOFTMAX_SEQ"):
        monkeypatch.delenv(var, raising=False)
    name = ac.case_id(case)
    fused, chain, p = run_both(hip, dev, case)[:3]
    mc.assert_same(fused, chain, name + ": fused vs matmul, mul, softmax, matmul")
    want = oracle[case["name"]]
    if case["dtype"] == "int8":
        if ac.both_exact(case):  # inside the proof the mfma form is the reference's chain, and so is the fused launch
            mc.assert_same(p, want["p"], name + ": the unfused probabilities vs the oracle chain")
            mc.assert_same(fused, want["out"], name + ": fused vs the oracle chain")
        else:
            mc.assert_within_gate(fused, want["out"], name + ": fused vs the oracle chain")
    else:
        keep = np.ones(fused.shape, bool)
        if case["special"]:  # the matrix cores' NaNs carry this device's sign, the oracle's x86's: those rows are compared above only
            keep[0, list(ac.SPECIAL_ROWS), :] = False
            rows = mc.bits(fused)[0, list(ac.SPECIAL_ROWS), :]
            assert np.all((rows[1] & 0x7FFF) == 0x7FFF), "the NaN in q must reach every output of its row"
        mc.assert_f16_gate(fused[keep], want["out"][keep], name + ": fused vs the oracle chain")


@pytest.mark.gpu
def test_refusals_name_no_kernel_and_write_nothing(gpu, monkeypatch):
    hip, dev = gpu
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM", raising=False)
    base = next(c for c in CASES if c["name"] == "base_f16")
    room = dev.alloc(1 << 16)
    dev.upload(room, np.full(1 << 16, POISON, np.uint8))
    q, k, v, out = room, room + 8192, room + 16384, room + 32768  # 8192 bytes each

    def refused(d, ptrs, code, text):
        status = hip.shl_mi355x_attention(*ptrs, C.byref(d), None)
        assert status == code, (text, status, hip.shl_mi355x_last_error())
        assert text.encode() in hip.shl_mi355x_last_error(), (text, hip.shl_mi355x_last_error())
        assert hip.shl_mi355x_attention_kernel_name(*ptrs, C.byref(d)) == b""
    ok = ac.desc(base)
    assert hip.shl_mi355x_attention_kernel_name(q, k, v, out, C.byref(ok)) == pkg.ATTENTION_MFMA.encode()
    far = (1 << 40, 1 << 41, 1 << 42, 1 << 43)  # (nothing is enqueued: the addresses only have to keep apart)
    d = ac.desc(base)
    d.t = ac.CAP + 1
    refused(d, far, EINVAL, "SHL_MI355X_ATTENTION_MAX_KEYS")
    d.t = ac.CAP
    assert hip.shl_mi355x_attention_kernel_name(*far, C.byref(d)) == pkg.ATTENTION_MFMA.encode()
    # the 17-token block of matmul_cases.attention_block: K = 32 with 2 x 17 x 17 outputs is the chain's
    d = ac.desc(base)
    d.batches, d.s, d.t, d.d, d.dv = 2, 17, 17, 32, 32
    refused(d, (q, k, v, out), ENOTSUP, "chain form")
    monkeypatch.setenv("SHL_MI355X_MATMUL_FORM", "chain")
    refused(ok, (q, k, v, out), ENOTSUP, "chain form")
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM")
    for ptrs in ((q, k, v, q), (q, k, v, k + 8190), (q, k, v, v - 8190), (q, out + 100, v, out)):
        refused(ok, ptrs, EINVAL, "overlaps an operand")
    for ptrs in ((q + 1, k, v, out), (q, k + 1, v, out), (q, k, v + 1, out), (q, k, v, out + 1)):
        refused(ok, ptrs, EINVAL, "not aligned")
    for field in ("reserved0", "reserved"):
        d = ac.desc(base)
        if field == "reserved":
            d.reserved[3] = 1
        else:
            d.reserved0 = 7
        refused(d, (q, k, v, out), EINVAL, "reserved")
    for field, value, text in (("s", 0, "below 1"), ("dv", -4, "below 1"), ("dtype", 2, "dtype"), ("has_scale", 2, "neither 0 nor 1"),
                               ("scale_raw", 1 << 16, "no element"), ("batches", 1 << 30, "2^31")):
        d = ac.desc(base)
        setattr(d, field, value)
        refused(d, (q, k, v, out), EINVAL, text)
    assert np.all(dev.download(room, (1 << 16,), np.uint8) == POISON)
    dev.free(room)

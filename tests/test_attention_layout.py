"""The attention core on operands where the projections left them (shl_mi355x_attention_layout) on the GPU (-m gpu): against
launches of kernels the layout form leaves alone -- shl_mi355x_move / shl_mi355x_transpose make the dense operands,
shl_mi355x_attention / shl_mi355x_attention_bias runs on them, shl_mi355x_transpose runs back -- on the same device buffers, bit
for bit, in int8 and binary16, over attention_layout_cases.all_cases().  The whole output frame is compared: 64-byte guard
bands and the gaps of a gapped layout keep their poison.  And the refusals, each with -2, its message, the kernel name "" and
nothing written; -3 where the dense call gives it."""
import ctypes as C

import numpy as np
import pytest

import attention_cases as ac
import attention_layout_cases as alc
import cases
from cases import pkg

CASES = alc.all_cases()
IDS = [alc.case_id(c) for c in CASES]
POISON = alc.POISON
EINVAL, ENOTSUP = -2, -3


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return hip, cases.HipDevice(hip)


@pytest.fixture(scope="module")
def frames(gpu):
    """every case's (got, want) frames, computed once"""
    return {}


def _frames(gpu, frames, case):
    name = alc.case_id(case)
    if name not in frames:
        frames[name] = alc.run_both(*gpu, case)
    return frames[name]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_layout_launch_equals_the_movers_around_the_dense_launch(gpu, frames, case, monkeypatch):
    for var in ("SHL_MI355X_MATMUL_FORM", "SHL_MI355X_TRANSPOSE_FORM"):
        monkeypatch.delenv(var, raising=False)
    got, want = _frames(gpu, frames, case)
    body = want[alc.GUARD:-alc.GUARD]
    assert np.unique(body).size > 8, "the output would tell nothing"
    if case["gap"]:
        assert (body == POISON).sum() >= case["B"] * case["s"] * case["gap"] * case["q"].itemsize - case["gap"] * case["q"].itemsize
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d bytes differ, the first at %d of %d (guards %d)" % (alc.case_id(case), bad.size, bad[0], got.size, alc.GUARD)


@pytest.mark.gpu
def test_the_moved_bits_decide_what_binary16_specials_become(gpu, frames):
    """the same data read as its movers would have left it and read raw: the two references differ, and each launch equals its own"""
    moved = next(c for c in CASES if c["name"] == "layout_specials_moved_f16")
    raw = next(c for c in CASES if c["name"] == "layout_specials_raw_f16")
    for key in ("q", "k", "v"):
        assert np.array_equal(moved[key].view(np.uint16), raw[key].view(np.uint16))
        u = moved[key].view(np.uint16)
        assert all((u == bits).any() for bits in alc.SPECIAL_BITS)
    (got_m, want_m), (got_r, want_r) = _frames(gpu, frames, moved), _frames(gpu, frames, raw)
    assert np.array_equal(got_m, want_m) and np.array_equal(got_r, want_r)
    assert not np.array_equal(want_m, want_r), "the movers' rule for infinities and NaNs must show in the output"


@pytest.mark.gpu
def test_refusals_name_no_kernel_and_write_nothing(gpu, monkeypatch):
    hip, dev = gpu
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM", raising=False)
    base = next(c for c in CASES if c["name"] == "layout_c3_mask_f16")
    room = dev.alloc(1 << 20)
    dev.upload(room, np.full(1 << 20, POISON, np.uint8))
    step = 1 << 17  # (every tensor of the case is smaller)
    q, k, v, bias, out = (room + i * step for i in range(5))
    d, bd, ok = ac.desc(base), alc.bias_desc(base), alc.layout_desc(hip, base)

    def refused(ptrs, dd, bb, ld, code, text):
        refs = (C.byref(dd), C.byref(bb) if bb is not None else None, C.byref(ld) if ld is not None else None)
        status = hip.shl_mi355x_attention_layout(*ptrs, *refs, None)
        assert status == code, (text, status, hip.shl_mi355x_last_error())
        assert text.encode() in hip.shl_mi355x_last_error(), (text, hip.shl_mi355x_last_error())
        assert hip.shl_mi355x_attention_layout_kernel_name(*ptrs, *refs) == b""
        assert hip.shl_mi355x_attention_layout_by_default(*ptrs, *refs) == 0
    ptrs = (q, k, v, bias, out)
    assert hip.shl_mi355x_attention_layout_kernel_name(*ptrs, C.byref(d), C.byref(bd), C.byref(ok)) == pkg.ATTENTION_BIAS_LAYOUT_MFMA.encode()
    assert hip.shl_mi355x_attention_layout_kernel_name(q, k, v, None, out, C.byref(d), None, C.byref(ok)) == pkg.ATTENTION_LAYOUT_MFMA.encode()

    def changed(**fields):
        ld = alc.layout_desc(hip, base)
        for key, value in fields.items():
            if isinstance(value, tuple):
                getattr(ld, key)[value[0]] = value[1]
            else:
                setattr(ld, key, value)
        return ld
    refused(ptrs, d, bd, None, EINVAL, "NULL argument")
    refused((q, k, v, None, out), d, bd, ok, EINVAL, "NULL argument")  # a bias descriptor without a bias
    refused((q, k, v, bias, out), d, None, ok, EINVAL, "NULL argument")
    refused((q, None, v, bias, out), d, bd, ok, EINVAL, "NULL argument")
    refused(ptrs, d, bd, changed(heads=0), EINVAL, "heads")
    refused(ptrs, d, bd, changed(heads=3), EINVAL, "heads")
    for key in ("q_stride", "k_stride", "v_stride", "out_stride"):
        for i in range(3):
            refused(ptrs, d, bd, changed(**{key: (i, -1)}), EINVAL, "negative")
    refused(ptrs, d, bd, changed(q_stride=(2, 1 << 30)), EINVAL, "2^31")
    refused(ptrs, d, bd, changed(v_stride=(1, (1 << 31) - 1)), EINVAL, "2^31")
    refused(ptrs, d, bd, changed(moved=16), EINVAL, "moved")
    refused(ptrs, d, bd, changed(moved=-1), EINVAL, "moved")
    refused(ptrs, d, bd, changed(reserved=(0, 1)), EINVAL, "reserved")
    refused(ptrs, d, bd, changed(reserved=(1, 7)), EINVAL, "reserved")
    refused(ptrs, d, bd, changed(out_stride=(2, 0)), EINVAL, "overlap each other")          # every row on the first
    refused(ptrs, d, bd, changed(out_stride=(1, 32)), EINVAL, "overlap each other")         # heads half a head apart
    refused(ptrs, d, bd, changed(out_stride=(2, 127)), EINVAL, "overlap each other")        # rows one short of two heads
    refused((q, k, v, bias, q), d, bd, ok, EINVAL, "overlaps an operand")
    refused((q, k, out + 2, bias, out), d, bd, ok, EINVAL, "overlaps an operand")
    refused((q, k, v, out + 64, out), d, bd, ok, EINVAL, "overlaps the bias")
    refused((q + 1, k, v, bias, out), d, bd, ok, EINVAL, "not aligned")
    refused((q, k, v, bias, out + 1), d, bd, ok, EINVAL, "not aligned")
    bad = alc.bias_desc(base)
    bad.key_stride = -1
    refused(ptrs, d, bad, ok, EINVAL, "negative")
    dd = ac.desc(base)
    dd.t = ac.CAP + 1
    refused(ptrs, dd, bd, ok, EINVAL, "SHL_MI355X_ATTENTION_MAX_KEYS")
    # inputs may overlap each other and themselves: q, k and v on one buffer, rows on top of each other
    free = changed(q_stride=(2, 0), k_stride=(2, 8))
    assert hip.shl_mi355x_attention_layout_kernel_name(q, q, q, bias, out, C.byref(d), C.byref(bd), C.byref(free)) != b""
    # -3 exactly where the dense call gives it
    small = ac.desc(base)
    small.batches, small.s, small.t, small.d, small.dv = 2, 17, 17, 32, 32  # the chain form's
    ld = pkg.AttentionLayoutDesc()
    ld.heads = 2
    for key, inner in (("q_stride", 32), ("k_stride", 32), ("v_stride", 32), ("out_stride", 32)):
        getattr(ld, key)[:] = [0, inner, 2 * inner]
    assert hip.shl_mi355x_attention_kernel_name(q, k, v, out, C.byref(small)) == b""
    assert hip.shl_mi355x_attention(q, k, v, out, C.byref(small), None) == ENOTSUP
    refused((q, k, v, None, out), small, None, ld, ENOTSUP, "chain form")
    monkeypatch.setenv("SHL_MI355X_MATMUL_FORM", "chain")
    refused(ptrs, d, bd, ok, ENOTSUP, "chain form")
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM")
    assert np.all(dev.download(room, (1 << 20,), np.uint8) == POISON)
    dev.free(room)

"""shl_mi355x_matmul_bias, the part that needs no GPU: the form rule is matmul's and names the bias kernels; what is wrong
with a call is refused before anything is enqueued (pure host code: made-up addresses, nothing is dereferenced)."""
import ctypes as C

import pytest

from cases import pkg

A, B, BIAS, O = 1 << 40, 2 << 40, 3 << 40, 4 << 40
EINVAL = -2
REC = (0.5, 3, 0.25, -7, 0, None)  # bias record, intermediate record, bias_is_first, stream


def _desc(dtype, m, n, k, batches=1):
    return pkg.matmul_desc(dtype, (batches, m, k), (batches, k, n), False, False, (0.0625, -5), (0.015625, 3), (0.5, 9))


@pytest.mark.parametrize("dtype", [pkg.SHL_I8, pkg.SHL_F16], ids=["int8", "f16"])
def test_the_form_rule_is_matmuls_and_names_the_bias_kernels(built, monkeypatch, dtype):
    hip = pkg.load_hip()
    for force in (None, "chain", "mfma"):
        if force:
            monkeypatch.setenv("SHL_MI355X_MATMUL_FORM", force)
        else:
            monkeypatch.delenv("SHL_MI355X_MATMUL_FORM", raising=False)
        for m, n, k in ((1, 1, 1), (17, 64, 64), (65, 33, 70), (64, 130, 16), (197, 768, 768), (300, 300, 16)):
            d = _desc(dtype, m, n, k)
            plain = hip.shl_mi355x_matmul_kernel_name(A, B, O, C.byref(d)).decode()
            assert plain in ("matmul_chain", "matmul_mfma")
            assert hip.shl_mi355x_matmul_bias_kernel_name(A, B, BIAS, O, C.byref(d)).decode() == plain + "_bias", (force, m, n, k)
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM", raising=False)
    assert hip.shl_mi355x_matmul_bias_kernel_name(A, B, BIAS, O, C.byref(_desc(dtype, 17, 64, 16))) == b"matmul_chain_bias"
    assert hip.shl_mi355x_matmul_bias_kernel_name(A, B, BIAS, O, C.byref(_desc(dtype, 17, 64, 64))) == b"matmul_mfma_bias"


def test_invalid_calls_are_refused_before_anything_is_enqueued(built):
    hip = pkg.load_hip()
    d = _desc(pkg.SHL_I8, 17, 64, 64)      # the output and A hold 1088 bytes, B 4096, the bias 64
    h = _desc(pkg.SHL_F16, 17, 64, 64)

    def refused(text, a=A, b=B, bias=BIAS, out=O, desc=d):
        ref = C.byref(desc) if desc is not None else None
        assert hip.shl_mi355x_matmul_bias(a, b, bias, out, ref, *REC) == EINVAL, text
        err = hip.shl_mi355x_last_error()
        assert b"matmul_bias: " in err and text.encode() in err, (text, err)
        assert hip.shl_mi355x_matmul_bias_kernel_name(a, b, bias, out, ref) == b""
    refused("NULL argument", bias=None)
    refused("NULL argument", a=None)
    refused("NULL argument", desc=None)
    refused("the output overlaps the bias", bias=O + 1087)
    refused("the output overlaps the bias", bias=O - 63)
    refused("the output overlaps an operand", out=A + 1087)
    refused("not aligned to its elements", bias=BIAS + 1, desc=h)
    bad = _desc(pkg.SHL_I8, 17, 64, 64)
    bad.out_elems = 17 * 64 + 1
    refused("batches x m x n", desc=bad)
    assert hip.shl_mi355x_matmul_bias_kernel_name(A, B, O - 64, O, C.byref(d)) == b"matmul_mfma_bias"   # the bias ends where the output begins
    assert hip.shl_mi355x_matmul_bias_kernel_name(A, B, BIAS + 1, O, C.byref(d)) == b"matmul_mfma_bias"  # an int8 bias may lie anywhere

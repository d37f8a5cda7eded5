"""The biased attention launch without a GPU: the exported entry points and the new descriptor's layout; the case list's own
conditions; validation and the stride derivation through the library (pure host code); and the same host code --
csrc/attention_canon.h:att_bias_validate and att_bias_geometry -- in a stand-alone program under the address and
undefined-behaviour sanitizers: every refusal, and for every bias geometry the derived strides against numpy's broadcast_to."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import attention_bias_cases as abc
import attention_cases as ac
import cases
import eltwise_cases
from cases import pkg

CASES = abc.all_cases()
IDS = [abc.case_id(c) for c in CASES]
EINVAL, ENOTSUP = -2, -3
FAR = (1 << 40, 1 << 41, 1 << 42, 1 << 44, 1 << 43)  # q, k, v, bias, out
SHAPES = [(s, t) for s in (1, 31, 32, 33, 65) for t in (1, 63, 64, 65, 129, 257, 1024)]


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_new_symbols_are_exported_and_the_descriptor_has_the_headers_layout(built):
    new = {"shl_mi355x_attention_bias", "shl_mi355x_attention_bias_kernel_name", "shl_mi355x_attention_bias_by_default",
           "shl_mi355x_attention_bias_geometry"}
    assert new <= _exports(pkg.lib_path("libshl_mi355x.so")) and new <= set(pkg.load_hip().EXPORTS)
    assert "shl_mi355x_session_fused_attention_biases" in _exports(pkg.lib_path("libshl_mi355x_opt.so"))
    D = pkg.AttentionBiasDesc
    assert C.sizeof(D) == 72 and D.b_stride.offset == 8 and D.row_stride.offset == 24 and D.key_stride.offset == 32
    assert D.b_scale.offset == 40 and D.sb_zp.offset == 52 and D.reserved.offset == 56
    assert C.sizeof(pkg.AttentionDesc) == 120  # the unbiased descriptor is what it was


def test_case_list_covers_what_it_must():
    for dtype in ("int8", "f16"):
        cs = [c for c in CASES if c["dtype"] == dtype]
        assert {1, 31, 32, 33, 65} <= {c["s"] for c in cs} and {1, 63, 64, 65, 129, 257, ac.CAP} <= {c["t"] for c in cs}
        assert set(abc.GEOMETRIES) == {c["geom"] for c in cs}
        assert all(c["batches"] == 6 for c in cs)
        for key in ("has_scale", "bias_first", "bias_off"):
            assert {bool(c[key]) for c in cs} == {False, True}, key
        assert all(ac.expect_fused(c) for c in cs), "both products must be the mfma form's"
    i8 = [c for c in CASES if c["dtype"] == "int8"]
    assert {"mask", "far", "plain"} == {c["kind"] for c in i8}
    assert {abc.fma_div(c) for c in i8} == {False, True}
    for c in i8:
        assert abc.fma_div(c) == (c["kind"] != "far"), c["name"]
    f16 = [c for c in CASES if c["kind"] == "special"]
    assert {c["bias_first"] for c in f16} == {False, True}
    for c in f16:
        u = c["bias"].view(np.uint16)
        assert np.all(u[0, :, :, 5] == abc.NEG_INF) and np.all(u[0, 1, 4, :] == abc.NEG_INF)
        assert (u == abc.POS_INF).any() and (u == abc.NEG_ZERO).any() and ((u & 0x7FFF) > 0x7C00).sum() == 3


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_library_derives_the_strides_numpy_broadcasts_by(built, case):
    hip = pkg.load_hip()
    bd = abc.bias_desc(hip, case)
    got = abc.desc_index_map(bd, case["batches"], case["s"], case["t"])
    assert np.array_equal(got, abc.index_map(case))
    assert case["batches"] % bd.b_ext1 == 0 and min(bd.b_stride[0], bd.b_stride[1], bd.row_stride, bd.key_stride) >= 0
    d = ac.desc(case)
    assert hip.shl_mi355x_attention_bias_kernel_name(*FAR, C.byref(d), C.byref(bd)) == pkg.ATTENTION_BIAS_MFMA.encode()
    # the default is the measured one (profiles/attention_bias_notes.md): none of these small shapes is in it
    assert hip.shl_mi355x_attention_bias_by_default(*FAR, C.byref(d), C.byref(bd)) == 0


def test_by_default_only_the_measured_classes_are_fused(built, monkeypatch):
    """csrc/attention_canon.h:att_bias_default restated (profiles/attention_bias_notes.md): heads of at most 32 -- on at least 768
    keys when the grid is one round of the chip (at most 256 workgroups of 32 query rows), on at most 64 keys when it is at
    least 3072 workgroups"""
    hip = pkg.load_hip()
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM", raising=False)
    base = next(c for c in CASES if c["name"] == "bias_h_s_t_s33_t65_i8")
    for fields, want in ((dict(batches=8, s=850, t=850, d=32, dv=32), 1),     # a DETR encoder layer at batch 1: 216 workgroups
                         (dict(batches=64, s=850, t=850, d=32, dv=32), 0),    # ... at batch 8: 1728
                         (dict(batches=8, s=1024, t=768, d=32, dv=32), 1), (dict(batches=8, s=1025, t=768, d=32, dv=32), 0),
                         (dict(batches=8, s=850, t=767, d=32, dv=32), 0), (dict(batches=8, s=850, t=850, d=33, dv=33), 0),
                         (dict(batches=1536, s=49, t=49, d=32, dv=32), 1),    # Swin-T stage 1 at batch 8: 3072 workgroups
                         (dict(batches=192, s=49, t=49, d=32, dv=32), 0),     # ... at batch 1: 384
                         (dict(batches=1535, s=49, t=49, d=32, dv=32), 0), (dict(batches=3072, s=32, t=64, d=32, dv=32), 1),
                         (dict(batches=3072, s=32, t=65, d=32, dv=32), 0), (dict(batches=1536, s=49, t=49, d=64, dv=64), 0),
                         (dict(batches=96, s=128, t=128, d=64, dv=64), 0), (dict(batches=96, s=197, t=197, d=64, dv=64), 0)):
        d = ac.desc(dict(base, **fields))
        bd = pkg.AttentionBiasDesc()
        bd.b_ext1, bd.key_stride, bd.b_scale, bd.sb_scale = 1, 1, 1.0, 1.0  # a bias [T]
        assert hip.shl_mi355x_attention_bias_kernel_name(*FAR, C.byref(d), C.byref(bd)) != b"", fields
        assert hip.shl_mi355x_attention_bias_by_default(*FAR, C.byref(d), C.byref(bd)) == want, fields
    monkeypatch.setenv("SHL_MI355X_MATMUL_FORM", "chain")
    d = ac.desc(dict(base, batches=8, s=850, t=850, d=32, dv=32))
    assert hip.shl_mi355x_attention_bias_by_default(*FAR, C.byref(d), C.byref(bd)) == 0


def _md(full, small):
    return eltwise_cases.mul_desc(dict(dtype="int8", in_q=(1.0, 0), in1_q=(1.0, 0), out_q=(1.0, 0)), full, small)


def test_geometries_the_descriptor_cannot_express_are_not_derived(built):
    hip = pkg.load_hip()
    bd = pkg.AttentionBiasDesc()
    geo = lambda full, small, b, s, t: hip.shl_mi355x_attention_bias_geometry(C.byref(_md(full, small)), b, s, t, C.byref(bd))
    assert geo((2, 3, 4, 8, 8), (2, 1, 4, 1, 1), 24, 8, 8) == ENOTSUP       # three batch groups
    assert geo((2, 3, 8, 8), (1, 1, 8, 1), 6, 8, 8) == 0                      # a bias per row
    assert (bd.row_stride, bd.key_stride) == (1, 0)
    assert geo((6, 4, 2, 8), (1, 4, 1, 8), 6, 8, 8) == ENOTSUP               # a group border inside the rows
    assert geo((6, 8, 2, 4), (1, 1, 2, 1), 6, 8, 8) == ENOTSUP               # ... inside the keys
    assert geo((2, 3, 8, 8), (1, 3, 8, 8), 6, 8, 9) == EINVAL                # not the scores' element count
    assert geo((2, 3, 8, 8), (1, 3, 8, 8), 0, 8, 8) == EINVAL
    assert hip.shl_mi355x_attention_bias_geometry(None, 6, 8, 8, C.byref(bd)) == EINVAL
    # three batch dims of which two neighbours vary together are two groups again
    assert geo((2, 3, 4, 8, 8), (2, 3, 1, 8, 8), 24, 8, 8) == 0
    assert (bd.b_ext1, bd.b_stride[0], bd.b_stride[1], bd.row_stride, bd.key_stride) == (4, 64, 0, 8, 1)


REFUSALS = [  # (descriptor fields, bias descriptor fields, pointers, what the message says)
    (dict(), dict(), (0, FAR[1], FAR[2], FAR[3], FAR[4]), "NULL argument"),
    (dict(), dict(), (FAR[0], FAR[1], FAR[2], 0, FAR[4]), "NULL argument"),
    (dict(), dict(no_bd=1), FAR, "NULL argument"),
    (dict(t=ac.CAP + 1), dict(), FAR, "SHL_MI355X_ATTENTION_MAX_KEYS"),
    (dict(s=0), dict(), FAR, "below 1"),
    (dict(dtype=2), dict(), FAR, "dtype"),
    (dict(reserved0=1), dict(), FAR, "reserved"),
    (dict(), dict(reserved2=1), FAR, "reserved"),
    (dict(), dict(bias_is_first=2), FAR, "bias_is_first"),
    (dict(), dict(bias_is_first=-1), FAR, "bias_is_first"),
    (dict(), dict(bs0=-1), FAR, "negative"),
    (dict(), dict(bs1=-1), FAR, "negative"),
    (dict(), dict(rs=-64), FAR, "negative"),
    (dict(), dict(ks=-1), FAR, "negative"),
    (dict(), dict(b_ext1=0), FAR, "b_ext1"),
    (dict(), dict(b_ext1=-3), FAR, "b_ext1"),
    (dict(), dict(b_ext1=4), FAR, "b_ext1"),
    (dict(), dict(b_ext1=7), FAR, "b_ext1"),
    (dict(), dict(ks=1 << 31), FAR, "2^31"),
    (dict(), dict(rs=1 << 26), FAR, "2^31"),
    (dict(), dict(bs0=(1 << 62)), FAR, "2^31"),
    (dict(), dict(bs0=1 << 30, bs1=1 << 29, rs=1 << 24, ks=1 << 24), FAR, "2^31"),
    (dict(dtype=1), dict(), (FAR[0], FAR[1], FAR[2], FAR[3] + 1, FAR[4]), "not aligned"),
    (dict(), dict(), (FAR[0], FAR[1], FAR[2], FAR[4], FAR[4]), "overlaps the bias"),
    (dict(), dict(), (FAR[0], FAR[1], FAR[2], FAR[4] + 6 * 64 * 64 - 1, FAR[4]), "overlaps the bias"),
    (dict(), dict(), (FAR[0], FAR[1], FAR[2], FAR[4] - 3 * 64 * 64 + 1, FAR[4]), "overlaps the bias"),
    (dict(), dict(), (FAR[0], FAR[1], FAR[4] + 8, FAR[3], FAR[4]), "overlaps an operand"),
    (dict(), dict(), (FAR[0], FAR[1], FAR[2], (1 << 64) - 64, FAR[4]), "wraps around"),
]
ACCEPTED = [  # (fields, bias fields, pointers): "ok" and the largest index
    (dict(), dict(), FAR, 3 * 64 * 64 - 1),
    (dict(), dict(), (FAR[0], FAR[1], FAR[2], FAR[4] + 6 * 64 * 64, FAR[4]), 3 * 64 * 64 - 1),  # touching is fine
    (dict(), dict(), (FAR[0], FAR[1], FAR[2], FAR[4] - 3 * 64 * 64, FAR[4]), 3 * 64 * 64 - 1),
    (dict(), dict(), (FAR[0], FAR[1], FAR[2], FAR[3] + 1, FAR[4]), 3 * 64 * 64 - 1),            # int8: any address
    (dict(), dict(b_ext1=6, bs0=1 << 62, bs1=0, rs=0, ks=0), FAR, 0),                            # a stride along an extent of 1
    (dict(s=1), dict(rs=1 << 40), FAR, 2 * 64 * 64 + 63),
    (dict(), dict(b_ext1=1, bs0=0, bs1=1 << 62, rs=0, ks=1), FAR, 63),
    (dict(), dict(bs0=0, bs1=0, rs=(1 << 24), ks=(1 << 24) - 1), FAR, 63 * (1 << 24) + 63 * ((1 << 24) - 1)),
    (dict(d=63, dv=64), dict(), FAR, "enotsup"),
]


def _vline(fields, bfields, ptrs):
    """base: int8, 2 x 3 batches of 64 x 64 scores on d = dv = 64, a bias [1, 3, 64, 64]"""
    f = dict(dtype=0, batches=6, s=64, t=64, d=64, dv=64, reserved0=0)
    b = dict(b_ext1=3, bias_is_first=0, bs0=0, bs1=64 * 64, rs=64, ks=1, reserved2=0, no_bd=0)
    f.update(fields)
    b.update(bfields)
    return "v " + " ".join(str(int(f[k])) for k in ("dtype", "batches", "s", "t", "d", "dv", "reserved0")) + " " + \
        " ".join(str(int(b[k])) for k in ("b_ext1", "bias_is_first", "bs0", "bs1", "rs", "ks", "reserved2", "no_bd")) + " " + \
        " ".join(str(int(p)) for p in ptrs)


def _glines():
    """(line, batches, s, t, the index map numpy expects or None when the geometry has no descriptor)"""
    out = []
    for s, t in SHAPES:
        for geom, shape_of in abc.GEOMETRIES.items():
            shape = shape_of(s, t)
            md = _md((abc.B0, abc.B1, s, t), shape)
            line = "g %d %d %d %d " % (md.ngroups, 6, s, t) + " ".join("%d %d" % (md.dim[g], md.b_stride[g]) for g in range(md.ngroups))
            out.append((line, 6, s, t, abc.index_map(dict(bias_shape=shape, s=s, t=t))))
    for full, small, b, s, t in (((2, 3, 4, 8, 8), (2, 1, 4, 1, 1), 24, 8, 8), ((6, 4, 2, 8), (1, 4, 1, 8), 6, 8, 8), ((6, 8, 2, 4), (1, 1, 2, 1), 6, 8, 8)):
        md = _md(full, small)
        line = "g %d %d %d %d " % (md.ngroups, b, s, t) + " ".join("%d %d" % (md.dim[g], md.b_stride[g]) for g in range(md.ngroups))
        out.append((line, b, s, t, None))
    return out


DRIVER = r"""
// Stand-alone driver of the biased launch's host code in csrc/attention_canon.h.  A line "v ..." is a call for
// att_bias_validate (+ att_unsupported): prints "einval <message>", "enotsup" or "ok <largest bias index>".  A line "g ..." is
// a set of collapsed groups for att_bias_geometry: prints its status and b_ext1 and the four strides.  Nothing is launched.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "attention_canon.h"

int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char mode[4];
    while (fscanf(f, "%3s", mode) == 1) {
        if (mode[0] == 'v') {
            long long v[15];
            unsigned long long p[5];
            for (int i = 0; i < 15; i++)
                if (fscanf(f, "%lld", &v[i]) != 1) return 3;
            for (int i = 0; i < 5; i++)
                if (fscanf(f, "%llu", &p[i]) != 1) return 3;
            shl_mi355x_attention_desc *d = new shl_mi355x_attention_desc;  // on the heap: reads past them are caught
            shl_mi355x_attention_bias_desc *b = new shl_mi355x_attention_bias_desc;
            memset(d, 0, sizeof(*d));
            memset(b, 0, sizeof(*b));
            d->dtype = (int32_t)v[0], d->batches = (int32_t)v[1], d->s = (int32_t)v[2], d->t = (int32_t)v[3], d->d = (int32_t)v[4];
            d->dv = (int32_t)v[5], d->reserved0 = (int32_t)v[6], d->p_zp = -128;
            d->q_scale = d->k_scale = d->v_scale = d->s_scale = d->c_scale = d->sc_scale = d->out_scale = 0.0625f, d->p_scale = 1.0f / 256;
            b->b_ext1 = (int32_t)v[7], b->bias_is_first = (int32_t)v[8], b->b_stride[0] = v[9], b->b_stride[1] = v[10];
            b->row_stride = v[11], b->key_stride = v[12], b->reserved[2] = (int32_t)v[13];
            b->b_scale = b->sb_scale = 0.0625f;
            const void *a[5];
            for (int i = 0; i < 5; i++) a[i] = (const void *)(uintptr_t)p[i];
            const char *why = shl::att_bias_validate(a[0], a[1], a[2], a[3], a[4], d, v[14] ? NULL : b);
            if (why) printf("einval %s\n", why);
            else if (shl::att_unsupported(d)) printf("enotsup\n");
            else printf("ok %lld\n", (long long)shl::att_bias_last(d, b));
            delete d;
            delete b;
        } else {
            int ng, batches, s, t;
            if (fscanf(f, "%d %d %d %d", &ng, &batches, &s, &t) != 4) return 3;
            shl_mi355x_mul_desc *m = new shl_mi355x_mul_desc;
            shl_mi355x_attention_bias_desc *b = new shl_mi355x_attention_bias_desc;
            memset(m, 0, sizeof(*m));
            memset(b, 0, sizeof(*b));
            m->ngroups = ng;
            for (int g = 0; g < ng && g < 4; g++) {
                long long dim, stride;
                if (fscanf(f, "%lld %lld", &dim, &stride) != 2) return 3;
                m->dim[g] = dim, m->b_stride[g] = stride;
            }
            const int rc = shl::att_bias_geometry(m, batches, s, t, b);
            printf("%d %d %lld %lld %lld %lld\n", rc, b->b_ext1, (long long)b->b_stride[0], (long long)b->b_stride[1], (long long)b->row_stride,
                   (long long)b->key_stride);
            delete m;
            delete b;
        }
    }
    fclose(f);
    return 0;
}
"""


def test_validation_through_the_library_refuses_what_the_header_lists(built, monkeypatch):
    hip = pkg.load_hip()
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM", raising=False)
    base = next(c for c in CASES if c["name"] == "bias_h_s_t_s33_t65_i8")
    d, ok = ac.desc(base), abc.bias_desc(hip, base)
    assert hip.shl_mi355x_attention_bias_kernel_name(*FAR, C.byref(d), C.byref(ok)) == pkg.ATTENTION_BIAS_MFMA.encode()

    def refused(bd, ptrs, text, code=EINVAL):
        ref = C.byref(bd) if bd is not None else None
        assert hip.shl_mi355x_attention_bias(*ptrs, C.byref(d), ref, None) == code, (text, hip.shl_mi355x_last_error())
        assert text.encode() in hip.shl_mi355x_last_error(), (text, hip.shl_mi355x_last_error())
        assert hip.shl_mi355x_attention_bias_kernel_name(*ptrs, C.byref(d), ref) == b""
    refused(None, FAR, "NULL argument")
    refused(ok, FAR[:3] + (None, FAR[4]), "NULL argument")
    refused(ok, FAR[:3] + (FAR[4] + 5, FAR[4]), "overlaps the bias")
    for field, value, text in (("b_ext1", 0, "b_ext1"), ("b_ext1", 5, "b_ext1"), ("bias_is_first", 3, "bias_is_first"),
                               ("row_stride", -1, "negative"), ("key_stride", -2, "negative"), ("key_stride", 1 << 31, "2^31")):
        bd = abc.bias_desc(hip, base)
        setattr(bd, field, value)
        refused(bd, FAR, text)
    bd = abc.bias_desc(hip, base)
    bd.reserved[0] = 9
    refused(bd, FAR, "reserved")
    monkeypatch.setenv("SHL_MI355X_MATMUL_FORM", "chain")
    refused(ok, FAR, "chain form", ENOTSUP)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc to compile with")
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on machines without a GPU")
def test_host_code_runs_clean_under_address_and_undefined_sanitizers(built, tmp_path):
    """att_bias_validate and att_bias_geometry compiled (-Xarch_host -fsanitize=address,undefined) into a program of its own: every
    refusal with its message, the calls that must pass with the largest index they form, and the strides of every bias geometry
    on every class of s and t, which must index the bias as numpy's broadcast_to does"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    inc = os.path.join(cases.ROOT, "include")
    csrc = os.path.join(cases.ROOT, "csi-nn2_amd", "csrc")
    san = "-fsanitize=address,undefined"
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "attention_bias_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-gpu-rdc", "-ffp-contract=off", "-Xarch_host", san,
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + inc, "-I" + csrc, "-x", "hip", "-c",
                    str(tmp_path / "driver.cpp"), "-o", str(tmp_path / "driver.o")], check=True)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fno-gpu-rdc", san, str(tmp_path / "driver.o"), "-o", exe], check=True)
    glines = _glines()
    lines = [_vline(f, b, p) for f, b, p, _ in REFUSALS] + [_vline(f, b, p) for f, b, p, _ in ACCEPTED] + [g[0] for g in glines]
    (tmp_path / "problems.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("SHL_MI355X_MATMUL_FORM", None)
    res = subprocess.run([exe, str(tmp_path / "problems.txt")], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
    rows = res.stdout.splitlines()
    assert len(rows) == len(lines)
    for (f, b, p, text), row in zip(REFUSALS, rows):
        assert row.startswith("einval ") and text in row, (f, b, p, row)
    for (f, b, p, want), row in zip(ACCEPTED, rows[len(REFUSALS):]):
        assert row == ("enotsup" if want == "enotsup" else "ok %d" % want), (f, b, p, row)
    for (line, batches, s, t, want), row in zip(glines, rows[len(REFUSALS) + len(ACCEPTED):]):
        rc, ext1, bs0, bs1, rs, ks = (int(x) for x in row.split())
        if want is None:
            assert rc == 2, (line, row)
            continue
        assert rc == 0, (line, row)
        bd = pkg.AttentionBiasDesc()
        bd.b_ext1, bd.b_stride[0], bd.b_stride[1], bd.row_stride, bd.key_stride = ext1, bs0, bs1, rs, ks
        assert np.array_equal(abc.desc_index_map(bd, batches, s, t), want), (line, row)

"""The attention layout launch without a GPU: the exported entry points and the new descriptor's layout; the case list's own
conditions; the stride derivation through the library against numpy's reshape(...).transpose(...) for every pattern and for
200 seeded random chains; and the same host code -- csrc/attention_canon.h:att_layout_validate, att_layout_strides and
att_layout_default -- in a stand-alone program under the address and undefined-behaviour sanitizers: every refusal, the calls
that must pass, the patterns and the random chains again."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import attention_cases as ac
import attention_layout_cases as alc
import cases
from cases import pkg

CASES = alc.all_cases()
IDS = [alc.case_id(c) for c in CASES]
EINVAL, ENOTSUP = -2, -3
FAR = (1 << 40, 1 << 41, 1 << 42, 1 << 44, 1 << 43)  # q, k, v, bias, out


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_new_symbols_are_exported_and_the_descriptor_has_the_headers_layout(built):
    new = {"shl_mi355x_attention_layout", "shl_mi355x_attention_layout_kernel_name", "shl_mi355x_attention_layout_by_default",
           "shl_mi355x_attention_layout_strides"}
    assert new <= _exports(pkg.lib_path("libshl_mi355x.so")) and new <= set(pkg.load_hip().EXPORTS)
    D = pkg.AttentionLayoutDesc
    assert C.sizeof(D) == 64 and D.heads.offset == 0 and D.moved.offset == 4 and D.q_stride.offset == 8 and D.k_stride.offset == 20
    assert D.v_stride.offset == 32 and D.out_stride.offset == 44 and D.reserved.offset == 56
    assert C.sizeof(pkg.AttentionDesc) == 120 and C.sizeof(pkg.AttentionBiasDesc) == 72  # the older descriptors are what they were


def test_case_list_covers_what_it_must():
    for dtype in ("int8", "f16"):
        cs = [c for c in CASES if c["dtype"] == dtype]
        assert {"reshape", "bshd", "packed", "k0231", "rank3"} == {c["pattern"] for c in cs}
        assert {None, "h_s_t", "b_t"} == {c["bias_geom"] for c in cs} and {0, 1, 2, 4} == {c["offset"] for c in cs}
        assert any(c["gap"] for c in cs) and any(c["d"] == 68 for c in cs) and {False, True} == {bool(c["has_scale"]) for c in cs}
        assert any((c["B"], c["H"], c["s"], c["t"], c["d"], c["dv"]) == (2, 3, 33, 70, 64, 72) for c in cs)
        assert any((c["B"], c["H"], c["s"], c["t"], c["d"], c["dv"]) == (16, 4, 49, 49, 32, 32) and c["bias_geom"] == "h_s_t" for c in cs)
        assert all(ac.expect_fused(c) for c in cs), "both products must be the mfma form's"
    assert {0, 15} == {c["moved"] for c in CASES if c["special_bits"]}


def _default(batches, s, t, d, dv=None):
    """csrc/attention_canon.h:att_layout_default restated (profiles/attention_layout_notes.md), dv = d: heads of 32 to 64 on 49
    to 197 keys from 21 workgroups of 32 query rows on -- the extremes of the measured rows --; heads of at most 32 on at least
    768 keys while the grid is at most 256 workgroups"""
    groups = batches * ((s + 31) // 32)
    if dv is not None and dv != d:
        return False
    return (49 <= t <= 197 and 32 <= d <= 64 and groups >= 21) or (d <= 32 and t >= 768 and groups <= 256)


def test_by_default_only_the_measured_classes_are_folded(built, monkeypatch):
    """one shape inside each admitted class and its nearest measured (or first unmeasured) neighbours outside, with and
    without a bias"""
    hip = pkg.load_hip()
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM", raising=False)
    base = next(c for c in CASES if c["name"] == "layout_c1_i8")
    for B, H, s, t, d, want in ((1, 12, 197, 197, 64, 1),    # ViT-B/16 at batch 1 ... and 8
                                (8, 12, 197, 197, 64, 1),
                                (1, 12, 198, 198, 64, 0),    # not measured
                                (1, 8, 384, 384, 64, 0),     # an encoder of 384 tokens: 0.98 in binary16
                                (1, 8, 512, 512, 64, 0),     # ... of 512: 1.03
                                (1, 12, 128, 128, 64, 1),    # BERT-base on 128 tokens
                                (64, 3, 49, 49, 32, 1),      # Swin-T windows
                                (4, 4, 64, 64, 64, 1),       # MobileViT
                                (1, 12, 197, 197, 65, 0),
                                (1, 12, 197, 197, 31, 0), (4, 12, 48, 48, 64, 0), (4, 12, 49, 49, 64, 1),  # below the measured extremes
                                (1, 3, 197, 197, 64, 1),     # DeiT-tiny at batch 1: 21 workgroups, the smallest grid measured
                                (1, 2, 197, 197, 64, 0),     # 14
                                (1, 8, 850, 850, 32, 1),     # a DETR encoder layer at batch 1: 216 workgroups
                                (8, 8, 850, 850, 32, 0),     # ... at batch 8: 1728, not measured
                                (1, 8, 1024, 768, 32, 1), (1, 8, 1025, 768, 32, 0), (1, 8, 850, 767, 32, 0), (1, 8, 850, 850, 33, 0)):
        assert int(_default(B * H, s, t, d)) == want
        d_ = ac.desc(dict(base, batches=B * H, s=s, t=t, d=d, dv=d))
        ld = pkg.AttentionLayoutDesc()
        ld.heads, ld.moved = H, 15
        ld.q_stride[:] = ld.out_stride[:] = [s * H * d, d, H * d]
        ld.k_stride[:] = ld.v_stride[:] = [t * H * d, d, H * d]
        bd = pkg.AttentionBiasDesc()
        bd.b_ext1, bd.key_stride, bd.b_scale, bd.sb_scale = 1, 1, 1.0, 1.0  # a bias [T]
        for bias, bref in ((None, None), (FAR[3], C.byref(bd))):
            args = FAR[:3] + (bias, FAR[4], C.byref(d_), bref, C.byref(ld))
            assert hip.shl_mi355x_attention_layout_kernel_name(*args) != b"", (B, H, s, t, d, hip.shl_mi355x_last_error())
            assert hip.shl_mi355x_attention_layout_by_default(*args) == want, (B, H, s, t, d)
    monkeypatch.setenv("SHL_MI355X_MATMUL_FORM", "chain")
    assert hip.shl_mi355x_attention_layout_by_default(*args[:5], C.byref(ac.desc(base)), bref, C.byref(alc.layout_desc(hip, base))) == 0


def _patterns():
    """(source dims, steps, swap_last2) of every pattern the planner must take, on small extents"""
    B, S, H, D = 2, 5, 3, 4
    return [((B, S, H * D), [("reshape", (B, S, H, D)), ("transpose", (0, 2, 1, 3))], 0),
            ((B, S, H, D), [("transpose", (0, 2, 1, 3))], 0),
            ((S, H, D), [("transpose", (1, 0, 2))], 0),
            ((B, S, H, D), [("transpose", (0, 2, 3, 1))], 1),
            ((B, S, H * D), [("reshape", (B, S, H, D)), ("transpose", (0, 2, 3, 1))], 1),
            ((B, S, H * D), [("reshape", (B, S, H, D)), ("transpose", (0, 2, 1, 3)), ("reshape", (B * H, S, D))], 0),
            ((1, S, H * D), [("reshape", (1, S, H, D)), ("transpose", (0, 2, 1, 3))], 0),
            ((B, 1, H * D), [("reshape", (B, 1, H, D)), ("transpose", (0, 2, 1, 3))], 0),
            ((B, S, D), [], 0),
            ((B, S, 3 * H * D), [("reshape", (B, S, 3 * H, D)), ("transpose", (0, 2, 1, 3))], 0)]


def _random_chains():
    rng = np.random.default_rng(20240607)
    out = []
    while len(out) < 200:
        rank = int(rng.integers(2, 6))
        dims = tuple(int(x) for x in rng.integers(1, 6, rank))
        steps = []
        if rng.random() < 0.5 and rank >= 2:  # a reshape in front: split the last dim or merge the first two
            last = dims[-1]
            f = [x for x in (2, 3, 4, 5) if last % x == 0]
            new = dims[:-1] + (f[0], last // f[0]) if f and rank < 6 else (dims[0] * dims[1],) + dims[2:]
            if len(new) >= 2:
                steps.append(("reshape", new))
                dims_now = new
            else:
                dims_now = dims
        else:
            dims_now = dims
        steps.append(("transpose", tuple(int(x) for x in rng.permutation(len(dims_now)))))
        if rng.random() < 0.3:
            shape = tuple(dims_now[p] for p in steps[-1][1])
            if len(shape) >= 3:
                steps.append(("reshape", (shape[0] * shape[1],) + shape[2:]))
        out.append((dims, steps, int(rng.random() < 0.2)))
    return out


def _agrees(row, src, steps, swap):
    rc, batches, rows, cols, heads, s0, s1, s2 = row
    want = alc.numpy_view(src, steps, swap)
    assert (batches, rows, cols) == want.shape and batches % heads == 0, (src, steps, swap, row)
    assert np.array_equal(alc.strides_index(batches, rows, cols, heads, [s0, s1, s2]), want), (src, steps, swap, row)


def test_the_library_derives_the_strides_numpy_views_by(built):
    hip = pkg.load_hip()
    for src, steps, swap in _patterns():
        rc, *rest = alc.derive(hip, src, steps, swap)
        assert rc == 0, (src, steps, swap, hip.shl_mi355x_last_error())
        _agrees((rc, *rest[:4], *rest[4]), src, steps, swap)
    agreed = refused = 0
    for src, steps, swap in _random_chains():
        rc, *rest = alc.derive(hip, src, steps, swap)
        assert rc in (0, ENOTSUP), (src, steps, swap, rc, hip.shl_mi355x_last_error())
        if rc == 0:
            _agrees((rc, *rest[:4], *rest[4]), src, steps, swap)
            agreed += 1
        else:
            refused += 1
    assert agreed >= 20 and refused >= 20, (agreed, refused)
    # what it must refuse, and what describes no view
    assert alc.derive(hip, (2, 5, 3, 4), [("transpose", (0, 1, 3, 2))], 0)[0] == ENOTSUP          # the inner stride is not 1
    assert alc.derive(hip, (2, 3, 4, 5, 6), [("transpose", (2, 1, 0, 3, 4))], 0)[0] == ENOTSUP    # three batch pieces
    assert alc.derive(hip, (2, 5, 3, 4), [("transpose", (0, 2, 1, 3)), ("reshape", (2, 3, 20))], 0)[0] == ENOTSUP
    assert alc.derive(hip, (2, 5, 12), [("reshape", (2, 5, 3, 5))], 0)[0] == EINVAL
    assert alc.derive(hip, (2, 5, 3, 4), [("transpose", (0, 2, 2, 3))], 0)[0] == EINVAL
    assert alc.derive(hip, (2, 5, 3, 4), [("transpose", (0, 2, 1, 3)), ("transpose", (0, 2, 1, 3))], 0)[0] == EINVAL
    assert alc.derive(hip, (7,), [], 0)[0] == EINVAL


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_case_names_the_layout_kernel_and_none_is_a_default(built, case, monkeypatch):
    hip = pkg.load_hip()
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM", raising=False)
    d, ld = ac.desc(case), alc.layout_desc(hip, case)
    bd = alc.bias_desc(case) if case["bias_geom"] else None
    args = FAR[:3] + (FAR[3] if bd else None, FAR[4], C.byref(d), C.byref(bd) if bd else None, C.byref(ld))
    want = pkg.ATTENTION_BIAS_LAYOUT_MFMA if bd else pkg.ATTENTION_LAYOUT_MFMA
    assert hip.shl_mi355x_attention_layout_kernel_name(*args) == want.encode(), hip.shl_mi355x_last_error()
    assert hip.shl_mi355x_attention_layout_by_default(*args) == int(_default(case["batches"], case["s"], case["t"], case["d"], case["dv"]))
    for key, (rows, inner) in alc.operands(case).items():
        if case["pattern"] == "packed" and key != "out":
            continue
        src, steps, swap = alc.chain_of(case, rows, inner, key)
        st = list(getattr(ld, key + "_stride"))
        if key == "out" and case["gap"]:
            continue
        assert np.array_equal(alc.strides_index(case["batches"], rows, inner, ld.heads, st), alc.numpy_view(src, steps, swap))


# base: int8, B = 2, H = 3, S = T = 64, d = dv = 64 out of [B, S, H D]: heads 3, strides {64 * 192, 64, 192} for all four
BASE = dict(dtype=0, batches=6, s=64, t=64, d=64, dv=64, has_bias=0, heads=3, moved=15, q=(12288, 64, 192), k=(12288, 64, 192),
            v=(12288, 64, 192), o=(12288, 64, 192), r0=0, r1=0, no_ld=0)
SPAN = 2 * 12288  # the elements an operand of the base spans
REFUSALS = [  # (fields, pointers, what the message says)
    (dict(), (0,) + FAR[1:], "NULL argument"),
    (dict(), FAR[:4] + (0,), "NULL argument"),
    (dict(no_ld=1), FAR, "NULL argument"),
    (dict(has_bias=1), FAR[:3] + (0, FAR[4]), "NULL argument"),
    (dict(t=ac.CAP + 1), FAR, "SHL_MI355X_ATTENTION_MAX_KEYS"),
    (dict(s=0), FAR, "below 1"),
    (dict(dtype=2), FAR, "dtype"),
    (dict(heads=0), FAR, "heads"),
    (dict(heads=-3), FAR, "heads"),
    (dict(heads=4), FAR, "heads"),
    (dict(moved=16), FAR, "moved"),
    (dict(moved=-1), FAR, "moved"),
    (dict(r0=1), FAR, "reserved"),
    (dict(r1=-1), FAR, "reserved"),
    (dict(q=(-1, 64, 192)), FAR, "negative"),
    (dict(k=(12288, -64, 192)), FAR, "negative"),
    (dict(v=(12288, 64, -192)), FAR, "negative"),
    (dict(o=(12288, 64, -1)), FAR, "negative"),
    (dict(q=(12288, 64, 1 << 30)), FAR, "2^31"),
    (dict(k=((1 << 31) - 1, 64, 192)), FAR, "2^31"),
    (dict(v=(12288, (1 << 31) - 1, 192)), FAR, "2^31"),
    (dict(o=(1 << 30, 1 << 29, 1 << 24)), FAR, "2^31"),
    (dict(dtype=1), (FAR[0] + 1,) + FAR[1:], "not aligned"),
    (dict(dtype=1), FAR[:4] + (FAR[4] + 1,), "not aligned"),
    (dict(o=(12288, 64, 0)), FAR, "overlap each other"),
    (dict(o=(12288, 63, 192)), FAR, "overlap each other"),
    (dict(o=(12288, 64, 191)), FAR, "overlap each other"),
    (dict(o=(12287, 64, 192)), FAR, "overlap each other"),
    (dict(o=(0, 64, 192)), FAR, "overlap each other"),
    (dict(), FAR[:4] + (FAR[0],), "overlaps an operand"),
    (dict(), FAR[:4] + (FAR[1] + SPAN - 1,), "overlaps an operand"),
    (dict(), FAR[:4] + (FAR[2] - SPAN + 1,), "overlaps an operand"),
    (dict(has_bias=1), FAR[:3] + (FAR[4] + 5, FAR[4]), "overlaps the bias"),
    (dict(), FAR[:4] + ((1 << 64) - 64,), "wraps around"),
]
ACCEPTED = [  # (fields, pointers, "ok" / "enotsup")
    (dict(), FAR, "ok"),
    (dict(has_bias=1), FAR, "ok"),
    (dict(), FAR[:4] + (FAR[1] + SPAN,), "ok"),                                  # touching is fine
    (dict(), FAR[:4] + (FAR[2] - SPAN,), "ok"),
    (dict(), (FAR[0], FAR[0] + 64, FAR[0] + 128, FAR[3], FAR[4]), "ok"),         # q, k and v inside one buffer
    (dict(q=(0, 0, 0), k=(0, 64, 0), v=(12288, 0, 8)), FAR, "ok"),               # inputs: broadcasts, rows that overlap
    (dict(o=(12288 + 64, 64, 192 + 1)), FAR, "ok"),                               # gaps
    (dict(o=(64 * 64, 2 * 64 * 64, 64)), FAR, "ok"),                              # the batch parts in the other order
    (dict(heads=6, o=(1 << 30, 64 * 64, 64)), FAR, "ok"),                         # a stride along an extent of 1
    (dict(heads=1, o=(64 * 64, 1 << 30, 64)), FAR, "ok"),
    (dict(s=1, o=(192, 64, 1 << 30)), FAR, "ok"),
    (dict(moved=0), FAR, "ok"),
    (dict(d=63), FAR, "enotsup"),
]


def _vline(fields, ptrs):
    f = dict(BASE)
    f.update(fields)
    nums = [f[k] for k in ("dtype", "batches", "s", "t", "d", "dv", "has_bias", "heads", "moved")]
    for k in ("q", "k", "v", "o"):
        nums += list(f[k])
    nums += [f["r0"], f["r1"], f["no_ld"]]
    return "v " + " ".join(str(int(x)) for x in nums) + " " + " ".join(str(int(p)) for p in ptrs)


def _gline(src, steps, swap):
    parts = ["g", str(len(src))] + [str(x) for x in src] + [str(len(steps))]
    for kind, v in steps:
        parts += [str(int(kind == "transpose")), str(len(v))] + [str(x) for x in v]
    return " ".join(parts + [str(swap)])


DRIVER = r"""
// Stand-alone driver of the layout launch's host code in csrc/attention_canon.h.  A line "v ..." is a call for
// att_layout_validate (+ att_unsupported, att_layout_default): prints "einval <message>", "enotsup" or "ok <by default>".  A
// line "g ..." is a chain of movers for att_layout_strides: prints its status, batches, rows, cols, heads and the three strides.
// Nothing is launched.
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
            long long v[24];
            unsigned long long p[5];
            for (int i = 0; i < 24; i++)
                if (fscanf(f, "%lld", &v[i]) != 1) return 3;
            for (int i = 0; i < 5; i++)
                if (fscanf(f, "%llu", &p[i]) != 1) return 3;
            shl_mi355x_attention_desc *d = new shl_mi355x_attention_desc;  // on the heap: reads past them are caught
            shl_mi355x_attention_bias_desc *b = new shl_mi355x_attention_bias_desc;
            shl_mi355x_attention_layout_desc *l = new shl_mi355x_attention_layout_desc;
            memset(d, 0, sizeof(*d));
            memset(b, 0, sizeof(*b));
            memset(l, 0, sizeof(*l));
            d->dtype = (int32_t)v[0], d->batches = (int32_t)v[1], d->s = (int32_t)v[2], d->t = (int32_t)v[3], d->d = (int32_t)v[4];
            d->dv = (int32_t)v[5], d->p_zp = -128;
            d->q_scale = d->k_scale = d->v_scale = d->s_scale = d->c_scale = d->sc_scale = d->out_scale = 0.0625f, d->p_scale = 1.0f / 256;
            b->b_ext1 = 1, b->key_stride = 1, b->b_scale = b->sb_scale = 0.0625f;  // a bias [t]
            l->heads = (int32_t)v[7], l->moved = (int32_t)v[8];
            for (int i = 0; i < 3; i++) {
                l->q_stride[i] = (int32_t)v[9 + i], l->k_stride[i] = (int32_t)v[12 + i];
                l->v_stride[i] = (int32_t)v[15 + i], l->out_stride[i] = (int32_t)v[18 + i];
            }
            l->reserved[0] = (int32_t)v[21], l->reserved[1] = (int32_t)v[22];
            const void *a[5];
            for (int i = 0; i < 5; i++) a[i] = (const void *)(uintptr_t)p[i];
            // (without a bias both the pointer and the descriptor are NULL)
            const char *why = shl::att_layout_validate(a[0], a[1], a[2], v[6] ? a[3] : NULL, a[4], d, v[6] ? b : NULL, v[23] ? NULL : l);
            if (why) printf("einval %s\n", why);
            else if (shl::att_unsupported(d)) printf("enotsup\n");
            else printf("ok %d\n", (int)shl::att_layout_default(d, l));
            delete d;
            delete b;
            delete l;
        } else {
            int rank, nsteps, swap;
            int32_t *src = new int32_t[8];
            if (fscanf(f, "%d", &rank) != 1 || rank > 8) return 3;
            for (int i = 0; i < rank; i++)
                if (fscanf(f, "%d", &src[i]) != 1) return 3;
            if (fscanf(f, "%d", &nsteps) != 1 || nsteps > 8) return 3;
            shl::AttViewStep *step = new shl::AttViewStep[nsteps > 0 ? nsteps : 1];
            for (int n = 0; n < nsteps; n++) {
                memset(&step[n], 0, sizeof(step[n]));
                if (fscanf(f, "%d %d", &step[n].is_transpose, &step[n].rank) != 2 || step[n].rank > 8) return 3;
                for (int i = 0; i < step[n].rank; i++)
                    if (fscanf(f, "%d", &step[n].v[i]) != 1) return 3;
            }
            if (fscanf(f, "%d", &swap) != 1) return 3;
            int32_t batches = 0, rows = 0, cols = 0, heads = 0;
            int32_t *stride = new int32_t[3]();
            const int rc = shl::att_layout_strides(src, rank, step, nsteps, swap, &batches, &rows, &cols, &heads, stride);
            printf("%d %d %d %d %d %d %d %d\n", rc, batches, rows, cols, heads, stride[0], stride[1], stride[2]);
            delete[] src;
            delete[] step;
            delete[] stride;
        }
    }
    fclose(f);
    return 0;
}
"""


def test_validation_through_the_library_refuses_what_the_header_lists(built, monkeypatch):
    hip = pkg.load_hip()
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM", raising=False)
    base = next(c for c in CASES if c["name"] == "layout_c1_i8")
    d = ac.desc(base)

    def status(ptrs, ld):
        return hip.shl_mi355x_attention_layout(*ptrs[:3], None, ptrs[4], C.byref(d), None, C.byref(ld) if ld is not None else None, None)

    def refused(ptrs, ld, text, code=EINVAL):
        assert status(ptrs, ld) == code, (text, hip.shl_mi355x_last_error())
        assert text.encode() in hip.shl_mi355x_last_error(), (text, hip.shl_mi355x_last_error())
        assert hip.shl_mi355x_attention_layout_kernel_name(*ptrs[:3], None, ptrs[4], C.byref(d), None,
                                                           C.byref(ld) if ld is not None else None) == b""
    refused(FAR, None, "NULL argument")
    for field, value, text in (("heads", 0, "heads"), ("heads", 4, "heads"), ("moved", 16, "moved")):
        ld = alc.layout_desc(hip, base)
        setattr(ld, field, value)
        refused(FAR, ld, text)
    for key, i, value, text in (("q_stride", 0, -1, "negative"), ("out_stride", 2, -5, "negative"), ("k_stride", 2, 1 << 30, "2^31"),
                                ("out_stride", 2, 0, "overlap each other"), ("out_stride", 1, 71, "overlap each other")):
        ld = alc.layout_desc(hip, base)
        getattr(ld, key)[i] = value
        refused(FAR, ld, text)
    ld = alc.layout_desc(hip, base)
    ld.reserved[1] = 3
    refused(FAR, ld, "reserved")
    ok = alc.layout_desc(hip, base)
    refused(FAR[:4] + (FAR[0] + 8,), ok, "overlaps an operand")
    monkeypatch.setenv("SHL_MI355X_MATMUL_FORM", "chain")
    refused(FAR, ok, "chain form", ENOTSUP)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc to compile with")
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on machines without a GPU")
def test_host_code_runs_clean_under_address_and_undefined_sanitizers(built, tmp_path):
    """att_layout_validate, att_layout_strides and att_layout_default compiled (-Xarch_host -fsanitize=address,undefined) into a
    program of its own: every refusal with its message, the calls that must pass, and the strides of every pattern and of the
    200 random chains, which must index the source as numpy's reshape and transpose do -- or be refused"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    inc = os.path.join(cases.ROOT, "include")
    csrc = os.path.join(cases.ROOT, "csi-nn2_amd", "csrc")
    san = "-fsanitize=address,undefined"
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "attention_layout_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-gpu-rdc", "-ffp-contract=off", "-Xarch_host", san,
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + inc, "-I" + csrc, "-x", "hip", "-c",
                    str(tmp_path / "driver.cpp"), "-o", str(tmp_path / "driver.o")], check=True)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fno-gpu-rdc", san, str(tmp_path / "driver.o"), "-o", exe], check=True)
    chains = _patterns() + _random_chains()
    odd = [((2, 5, 3, 4), [("transpose", (0, 1, 3, 2))], 0, 2), ((2, 3, 4, 5, 6), [("transpose", (2, 1, 0, 3, 4))], 0, 2),
           ((2, 5, 12), [("reshape", (2, 5, 3, 5))], 0, 1), ((2, 5, 3, 4), [("transpose", (0, 2, 2, 3))], 0, 1),
           ((2, 5, 3, 4), [("transpose", (0, 9, 1, 3))], 0, 1), ((7,), [], 0, 1), ((2, 0, 4), [], 0, 1),
           ((1 << 15, 1 << 15, 4), [], 0, 2)]
    lines = [_vline(f, p) for f, p, _ in REFUSALS] + [_vline(f, p) for f, p, _ in ACCEPTED] + [_gline(*c) for c in chains] + \
        [_gline(s, st, sw) for s, st, sw, _ in odd]
    (tmp_path / "problems.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("SHL_MI355X_MATMUL_FORM", None)
    res = subprocess.run([exe, str(tmp_path / "problems.txt")], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
    rows = res.stdout.splitlines()
    assert len(rows) == len(lines)
    for (f, p, text), row in zip(REFUSALS, rows):
        assert row.startswith("einval ") and text in row, (f, p, row)
    at = len(REFUSALS)
    for (f, p, want), row in zip(ACCEPTED, rows[at:]):
        fields = dict(BASE, **f)
        by_default = int(_default(fields["batches"], fields["s"], fields["t"], fields["d"], fields["dv"]))
        assert row == ("enotsup" if want == "enotsup" else "ok %d" % by_default), (f, p, row)
    at += len(ACCEPTED)
    n_patterns = len(_patterns())
    for i, ((src, steps, swap), row) in enumerate(zip(chains, rows[at:])):
        vals = tuple(int(x) for x in row.split())
        assert vals[0] in ((0,) if i < n_patterns else (0, 2)), (src, steps, swap, row)
        if vals[0] == 0:
            _agrees(vals, src, steps, swap)
    at += len(chains)
    for (src, steps, swap, want), row in zip(odd, rows[at:]):
        assert int(row.split()[0]) == want, (src, steps, swap, row)

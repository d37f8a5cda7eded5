"""The fused attention core without a GPU: the case list's own conditions (the plan-time proof for both products where the
comparison with the oracle is bit for bit, rows of p and outputs that can tell results apart), the exported entry points and the
descriptor's layout, validation, the cap and the form rule through the library (pure host code) against a Python restatement,
and the same host code -- csrc/attention_canon.h -- in a stand-alone program under the address and undefined-behaviour
sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import attention_cases as ac
import cases
import matmul_cases as mc
from cases import pkg

CASES = ac.all_cases()
IDS = [ac.case_id(c) for c in CASES]
EINVAL, ENOTSUP = -2, -3
FORM_ENV = "SHL_MI355X_MATMUL_FORM"
FAR = (1 << 40, 1 << 41, 1 << 42, 1 << 43)


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_new_symbols_are_exported_and_the_descriptor_has_the_headers_layout(built):
    assert {"shl_mi355x_attention", "shl_mi355x_attention_kernel_name"} <= _exports(pkg.lib_path("libshl_mi355x.so"))
    assert "shl_mi355x_session_fused_attentions" in _exports(pkg.lib_path("libshl_mi355x_opt.so"))
    assert C.sizeof(pkg.AttentionDesc) == 120 and pkg.AttentionDesc.q_scale.offset == 40 and pkg.AttentionDesc.q_zp.offset == 72
    assert pkg.AttentionDesc.reserved.offset == 104
    header = open(os.path.join(cases.ROOT, "include", "shl_mi355x.h")).read()
    assert "#define SHL_MI355X_ATTENTION_MAX_KEYS %d\n" % ac.CAP in header


def test_case_list_covers_what_it_must():
    for dtype in ("int8", "f16"):
        cs = [c for c in CASES if c["dtype"] == dtype]
        assert any((c["s"], c["t"], c["d"], c["dv"], c["batches"]) == (64, 64, 64, 64, 1) for c in cs)
        assert {65, 97, 256, 257, 320, ac.CAP} <= {c["t"] for c in cs} and {1, 33} <= {c["s"] for c in cs}
        assert {72, 128} <= {c["d"] for c in cs} and 40 in {c["dv"] for c in cs} and 3 in {c["batches"] for c in cs}
        assert any(c["t"] == ac.CAP and c["s"] == 32 for c in cs)
        assert {(c["has_scale"], c["has_scale"] and c["scale_first"]) for c in cs} == {(True, False), (True, True), (False, False)}
    i8 = [c for c in CASES if c["dtype"] == "int8"]
    assert {c["regime"] for c in i8} == {"pow2", "conv"}
    for key in ("q_q", "k_q", "v_q"):
        assert {-128, 0, 127} <= {c[key][1] for c in i8}, key
    assert all(c["p_q"] == ac.P_Q for c in i8)
    assert any(c["special"] for c in CASES)


@pytest.fixture(scope="module")
def chains():
    return {c["name"]: ac.oracle_chain(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_pass_on_this_case_means_something(case, chains):
    """rows of p that are peaked but not one-hot, an output that spreads; int8: the proof decides whether the mfma form's
    formula is the oracle chain bit for bit, and it is; where the proof fails the formula stays inside the gate"""
    chain = chains[case["name"]]
    rows, outs = ac.spread_report(case, chain)
    assert rows > 8, "a row of p holds %d distinct values" % rows
    assert outs > 8, "the output holds %d distinct values" % outs
    assert ac.expect_fused(case)
    if case["dtype"] != "int8":
        return
    # (no row of scores is flat because the record clamped it)
    assert np.mean((chain["s"] == 127) | (chain["s"] == -128)) < 0.02
    formula = ac.device_formula(case)
    if ac.both_exact(case):
        assert case["regime"] == "pow2"
        for key in ("s", "p", "out"):
            mc.assert_same(formula[key], chain[key], "%s: %s by the mfma form's formula vs the oracle chain" % (case["name"], key))
    else:
        assert case["regime"] == "conv" or case["t"] == ac.CAP  # (255 x 128 x 1024 > 2^24: the cap cannot satisfy the proof)
        mc.assert_within_gate(formula["out"], chain["out"], case["name"] + ": the mfma form's formula vs the oracle chain")


def lds_bytes(dtype, t, waves=4):
    """csrc/attention_canon.h:att_lds restated: an e row per wave, two tables per wave (int8), the 32 x t tile, operand slabs,
    row sums"""
    es, i8 = (1, True) if dtype == "int8" else (2, False)
    pitch = (t * es + 63) // 64 * 64 + 16
    return waves * (t + 256) * 8 + (waves * (256 * 8 + 256) if i8 else 0) + 32 * pitch + (32 + 128) * 80 + 512, pitch


def waves_of(dtype, batches, s, t):
    """csrc/attention_canon.h:att_waves restated: 16, 8 or 4 waves -- the most that keep the grid at or under 256 CUs x 16 waves
    and fit 160 KiB of LDS"""
    groups = batches * ((s + 31) // 32)
    for waves in (16, 8):
        if groups * waves <= 256 * 16 and lds_bytes(dtype, t, waves)[0] <= 160 * 1024:
            return waves
    return 4


def test_the_cap_fits_the_lds_as_the_header_states():
    assert lds_bytes("f16", ac.CAP)[0] == 120320 and lds_bytes("int8", ac.CAP)[0] == 96768
    assert lds_bytes("f16", ac.CAP, 8)[0] == 161280 and lds_bytes("int8", ac.CAP, 8)[0] == 146944
    assert waves_of("f16", 1, 32, ac.CAP) == 8 and waves_of("int8", 12, 197, 197) == 16 and waves_of("f16", 96, 197, 197) == 4
    for dt in ("int8", "f16"):
        for t in range(1, ac.CAP + 1):
            for batches in (1, 40, 300):
                assert lds_bytes(dt, t, waves_of(dt, batches, 64, t))[0] <= 160 * 1024
    header = open(os.path.join(cases.ROOT, "include", "shl_mi355x.h")).read()
    assert "120320" in header and "161280 of 163840" in header and "96768" in header and "146944" in header


def _refusal(hip, d, ptrs=FAR):
    """(status, kernel name) of a call that must not reach the device"""
    name = hip.shl_mi355x_attention_kernel_name(*ptrs, C.byref(d))
    return (0 if name else hip.shl_mi355x_attention(*ptrs, C.byref(d), None)), name


@pytest.mark.parametrize("force", [None, "chain", "mfma"])
def test_kernel_name_follows_the_form_rule_of_both_products(built, force, monkeypatch):
    hip = pkg.load_hip()
    if force is None:
        monkeypatch.delenv(FORM_ENV, raising=False)
    else:
        monkeypatch.setenv(FORM_ENV, force)
    for case in CASES:
        status, name = _refusal(hip, ac.desc(case))
        if ac.expect_fused(case, force):
            assert name == pkg.ATTENTION_MFMA.encode(), ac.case_id(case)
        else:
            assert (status, name) == (ENOTSUP, b"") and b"chain form" in hip.shl_mi355x_last_error(), ac.case_id(case)
    # around the rule's thresholds: K = 63 / 64 with few outputs, K = 32 with 65536 / 65537 scores, few keys in P V
    base = next(c for c in CASES if c["name"] == "base_i8")
    for fields in (dict(d=63), dict(d=64), dict(d=32, s=256, t=256), dict(d=32, s=257, t=256), dict(t=63), dict(t=63, dv=1024, s=65),
                   dict(t=17, s=17, d=32, dv=32, batches=2), dict(d=32768), dict(d=32769), dict(q_zp=128), dict(v_zp=-129)):
        case = dict(base, **{k: v for k, v in fields.items() if not k.endswith("_zp")})
        d = ac.desc(case)
        for k, v in fields.items():
            if k.endswith("_zp"):
                setattr(d, k, v)
        want = ac.expect_fused(case, force) and not any(k.endswith("_zp") for k in fields)
        status, name = _refusal(hip, d)
        assert (name == pkg.ATTENTION_MFMA.encode()) == want, (fields, force, name)
        assert want or status == ENOTSUP, (fields, status)


def test_by_default_only_the_measured_class_is_fused(built, monkeypatch):
    """csrc/attention_canon.h:att_default restated: heads of at most 32 on at least 768 keys, where the call names a kernel"""
    hip = pkg.load_hip()
    monkeypatch.delenv(FORM_ENV, raising=False)
    for case in CASES:
        assert hip.shl_mi355x_attention_by_default(*FAR, C.byref(ac.desc(case))) == 0, ac.case_id(case)
    base = next(c for c in CASES if c["name"] == "base_i8")
    for fields, want in ((dict(batches=8, s=850, t=850, d=32, dv=32), 1), (dict(s=768, t=768, d=32), 1), (dict(s=768, t=767, d=32), 0),
                         (dict(s=768, t=768, d=33), 0), (dict(s=768, t=768, d=16, dv=16), 1), (dict(s=64, t=768, d=32), 0),
                         (dict(s=768, t=ac.CAP + 1, d=32), 0)):
        d = ac.desc(dict(base, **fields))
        assert hip.shl_mi355x_attention_by_default(*FAR, C.byref(d)) == want, fields
    monkeypatch.setenv(FORM_ENV, "chain")
    assert hip.shl_mi355x_attention_by_default(*FAR, C.byref(ac.desc(dict(base, s=768, t=768, d=32)))) == 0


def test_invalid_descriptors_are_refused_before_touching_the_device(built, monkeypatch):
    hip = pkg.load_hip()
    monkeypatch.delenv(FORM_ENV, raising=False)
    base = next(c for c in CASES if c["name"] == "base_f16")
    q, k, v, out = FAR

    def refused(d, ptrs, text, code=EINVAL):
        ref = C.byref(d) if d is not None else None
        status = hip.shl_mi355x_attention(*ptrs, ref, None)
        assert status == code, (text, status, hip.shl_mi355x_last_error())
        assert text.encode() in hip.shl_mi355x_last_error(), (text, hip.shl_mi355x_last_error())
        assert hip.shl_mi355x_attention_kernel_name(*ptrs, ref) == b""
    ok = ac.desc(base)
    assert hip.shl_mi355x_attention_kernel_name(q, k, v, out, C.byref(ok)) == pkg.ATTENTION_MFMA.encode()
    refused(None, FAR, "NULL argument")
    for i in range(4):
        refused(ok, tuple(None if j == i else p for j, p in enumerate(FAR)), "NULL argument")
    for field, value, text in (("dtype", 2, "dtype"), ("batches", 0, "below 1"), ("s", 0, "below 1"), ("t", -1, "below 1"), ("d", 0, "below 1"),
                               ("dv", 0, "below 1"), ("t", ac.CAP + 1, "SHL_MI355X_ATTENTION_MAX_KEYS"), ("reserved0", 1, "reserved"),
                               ("has_scale", 2, "neither 0 nor 1"), ("scale_is_first", -1, "neither 0 nor 1"),
                               ("scale_raw", -1, "no element"), ("scale_raw", 1 << 16, "no element"),
                               ("batches", 1 << 19, "2^31"), ("s", 0x7FFFFFFF, "2^31"), ("d", 0x7FFFFFFF, "2^31"), ("dv", 1 << 25, "2^31")):
        bad = ac.desc(base)
        setattr(bad, field, value)
        refused(bad, FAR, text)
    for i in range(4):
        bad = ac.desc(base)
        bad.reserved[i] = -1
        refused(bad, FAR, "reserved")
    i8 = ac.desc(next(c for c in CASES if c["name"] == "base_i8"))
    for raw in (-129, 128):
        i8.scale_raw = raw
        refused(i8, FAR, "no element")
    nbytes = 64 * 64 * 2
    for ptrs in ((q, k, v, q), (q, k, v, q + nbytes - 2), (q, k, v, k - nbytes + 2), (q, k, out + 2, out), (out, k, v, out)):
        refused(ok, ptrs, "overlaps an operand")
    assert hip.shl_mi355x_attention_kernel_name(q, k, v, q + nbytes, C.byref(ok)) != b""  # touching is fine
    for i in range(4):
        refused(ok, tuple(p + 1 if j == i else p for j, p in enumerate(FAR)), "not aligned")
    refused(ok, ((1 << 64) - 64, k, v, out), "wraps around")
    chain = ac.desc(base)
    chain.batches, chain.s, chain.t, chain.d, chain.dv = 2, 17, 17, 32, 32
    refused(chain, FAR, "chain form", ENOTSUP)


# ------------------------------------------------------------------------------------ the host code under sanitizers
DRIVER = r"""
// Stand-alone driver of csrc/attention_canon.h, the host code of csrc/attention.hip: reads one descriptor per line, prints
// "einval", "enotsup", or the workgroup's waves, its LDS bytes, its tile pitch and the three operands' load widths.  Nothing is launched.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "attention_canon.h"

int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    long long v[15];
    unsigned long long p[4];
    // <dtype> <batches> <s> <t> <d> <dv> <has_scale> <scale_is_first> <scale_raw> <reserved0> <q k v p zero points> <reserved[3]> <4 addresses>
    for (;;) {
        int got = 0;
        for (int i = 0; i < 15; i++) got += fscanf(f, "%lld", &v[i]) == 1;
        if (got != 15) break;
        if (fscanf(f, "%llu %llu %llu %llu", &p[0], &p[1], &p[2], &p[3]) != 4) return 3;
        struct shl_mi355x_attention_desc *d = new shl_mi355x_attention_desc;  // on the heap: reads past it are caught
        memset(d, 0, sizeof(*d));
        d->dtype = (int32_t)v[0], d->batches = (int32_t)v[1], d->s = (int32_t)v[2], d->t = (int32_t)v[3], d->d = (int32_t)v[4];
        d->dv = (int32_t)v[5], d->has_scale = (int32_t)v[6], d->scale_is_first = (int32_t)v[7], d->scale_raw = (int32_t)v[8];
        d->reserved0 = (int32_t)v[9], d->q_zp = (int32_t)v[10], d->k_zp = (int32_t)v[11], d->v_zp = (int32_t)v[12];
        d->p_zp = (int32_t)v[13], d->reserved[3] = (int32_t)v[14];
        d->q_scale = d->k_scale = d->v_scale = d->s_scale = d->c_scale = d->sc_scale = d->out_scale = 0.0625f, d->p_scale = 1.0f / 256;
        const void *q = (const void *)(uintptr_t)p[0], *k = (const void *)(uintptr_t)p[1], *vv = (const void *)(uintptr_t)p[2];
        const void *o = (const void *)(uintptr_t)p[3];
        if (shl::att_validate(q, k, vv, o, d)) {
            printf("einval\n");
        } else if (shl::att_unsupported(d)) {
            printf("enotsup\n");
        } else {
            const int waves = shl::att_waves(d);
            const shl::AttLds l = shl::att_lds(d, waves);
            const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
            printf("%d %d %d %d %d %d\n", waves, l.bytes, l.tile_pitch, shl::att_vec(q, d->d, es), shl::att_vec(k, d->d, es), shl::att_vec(vv, d->dv, es));
        }
        delete d;
    }
    fclose(f);
    return 0;
}
"""


def _line(fields, ptrs=FAR):
    f = dict(dtype=0, batches=1, s=64, t=64, d=64, dv=64, has_scale=1, scale_is_first=0, scale_raw=0, reserved0=0, q_zp=0, k_zp=0,
             v_zp=0, p_zp=-128, reserved3=0)
    f.update(fields)
    return " ".join(str(int(f[k])) for k in ("dtype", "batches", "s", "t", "d", "dv", "has_scale", "scale_is_first", "scale_raw", "reserved0",
                                             "q_zp", "k_zp", "v_zp", "p_zp", "reserved3")) + " " + " ".join(str(int(p)) for p in ptrs)


def _problems():
    """(line, fields, pointers, the class the restatement expects: "einval", "rule" -- the form rule decides -- )"""
    big = 0x7FFFFFFF
    out = []
    for c in CASES:
        fields = dict(dtype=pkg.SHL_I8 if c["dtype"] == "int8" else pkg.SHL_F16, batches=c["batches"], s=c["s"], t=c["t"], d=c["d"], dv=c["dv"],
                      has_scale=int(c["has_scale"]), q_zp=c["q_q"][1], k_zp=c["k_q"][1], v_zp=c["v_q"][1])
        for skew in (0, 2, 8, 16):
            out.append((fields, tuple(p + skew for p in FAR), "rule"))
    for fields in (dict(t=ac.CAP), dict(t=ac.CAP, dtype=1), dict(d=63), dict(d=32, s=257, t=256), dict(t=63, dv=1040, s=65), dict(d=32768),
                   dict(d=32769), dict(q_zp=128), dict(k_zp=-129), dict(p_zp=-129), dict(batches=big // 64 // 64, d=1, dv=1)):
        out.append((fields, FAR, "rule"))
    for fields in (dict(t=ac.CAP + 1), dict(s=0), dict(t=-1), dict(d=0), dict(dv=-7), dict(batches=0), dict(batches=big, s=big, t=1024, d=big, dv=big),
                   dict(batches=big), dict(s=big), dict(d=big), dict(dv=big), dict(batches=1 << 19), dict(dtype=-3), dict(dtype=2),
                   dict(reserved0=5), dict(reserved3=-1), dict(has_scale=3), dict(scale_is_first=2), dict(scale_raw=128), dict(scale_raw=-129),
                   dict(dtype=1, scale_raw=65536)):
        out.append((fields, FAR, "einval"))
    for ptrs in ((0, FAR[1], FAR[2], FAR[3]), (FAR[0], FAR[1], FAR[2], FAR[0] + 17), (FAR[0], FAR[1], FAR[2], FAR[2] - 5),
                 ((1 << 64) - 64, FAR[1], FAR[2], FAR[3]), (FAR[0], FAR[1], FAR[2], (1 << 64) - 64)):
        out.append((dict(), ptrs, "einval"))
    out.append((dict(dtype=1), (FAR[0] + 1, FAR[1], FAR[2], FAR[3]), "einval"))
    return out


def _expect(fields, ptrs, kind, force):
    """the restatement: what the program must print"""
    if kind == "einval":
        return ["einval"]
    f = dict(dtype=0, batches=1, s=64, t=64, d=64, dv=64, q_zp=0, k_zp=0, v_zp=0, p_zp=-128)
    f.update(fields)
    dtype = "int8" if f["dtype"] == pkg.SHL_I8 else "f16"
    zps_fit = all(-128 <= f[k] <= 127 for k in ("q_zp", "k_zp", "v_zp", "p_zp"))
    case = dict(dtype=dtype, batches=f["batches"], s=f["s"], t=f["t"], d=f["d"], dv=f["dv"], q_q=(1.0, 0), k_q=(1.0, 0), s_q=(1.0, 0),
                p_q=(1.0, 0), v_q=(1.0, 0), out_q=(1.0, 0), q=None, k=None, v=None)
    if not ac.expect_fused(case, force) or (dtype == "int8" and not zps_fit):
        return ["enotsup"]
    es = 1 if dtype == "int8" else 2
    waves = waves_of(dtype, f["batches"], f["s"], f["t"])
    total, pitch = lds_bytes(dtype, f["t"], waves)
    vec = lambda p, inner: int(p % 16 == 0 and inner * es % 16 == 0)
    return [str(waves), str(total), str(pitch), str(vec(ptrs[0], f["d"])), str(vec(ptrs[1], f["d"])), str(vec(ptrs[2], f["dv"]))]


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc to compile with")
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on machines without a GPU")
def test_host_code_runs_clean_under_address_and_undefined_sanitizers(built, tmp_path):
    """csrc/attention_canon.h -- validation, the cap, the form rule, the LDS layout: all the host code of csrc/attention.hip --
    compiled (-Xarch_host -fsanitize=address,undefined) into a program of its own, which takes every case's descriptor and a
    list of hostile ones apart and must agree with the Python restatement line by line"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    inc = os.path.join(cases.ROOT, "include")
    csrc = os.path.join(cases.ROOT, "csi-nn2_amd", "csrc")
    san = "-fsanitize=address,undefined"
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "attention_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-gpu-rdc", "-ffp-contract=off", "-Xarch_host", san,
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + inc, "-I" + csrc, "-x", "hip", "-c",
                    str(tmp_path / "driver.cpp"), "-o", str(tmp_path / "driver.o")], check=True)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fno-gpu-rdc", san, str(tmp_path / "driver.o"), "-o", exe], check=True)
    problems = _problems()
    (tmp_path / "problems.txt").write_text("\n".join(_line(f, p) for f, p, _ in problems) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    seen = set()
    for force in (None, "chain", "mfma"):
        e = dict(env)
        e.pop(FORM_ENV, None)
        if force:
            e[FORM_ENV] = force
        res = subprocess.run([exe, str(tmp_path / "problems.txt")], capture_output=True, text=True, env=e, timeout=120)
        assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
        rows = [ln.split() for ln in res.stdout.splitlines()]
        assert len(rows) == len(problems)
        for (fields, ptrs, kind), row in zip(problems, rows):
            assert row == _expect(fields, ptrs, kind, force), (fields, ptrs, force, row)
            seen.add(row[0] if len(row) == 1 else "fused")
    assert seen == {"einval", "enotsup", "fused"}

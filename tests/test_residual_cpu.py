"""The fused residual tail without a GPU: the exported entry points and the descriptor's layout, what the library answers with
no plan, the case list's own conditions, and the call's validation -- csrc/residual_validate.h, pure host code -- in a
stand-alone program under the address and undefined-behaviour sanitizers against a Python restatement."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import cases
import residual_cases as rc
from cases import pkg

EINVAL, ENOTSUP = -2, -3
ALGO_IGEMM, ALGO_DW, ALGO_DECONV_GATHER, ALGO_DECONV_PHASE = pkg.ALGO_IGEMM, pkg.ALGO_DW, pkg.ALGO_DECONV_GATHER, pkg.ALGO_DECONV_PHASE


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_new_symbols_are_exported_and_the_descriptor_has_the_headers_layout(built):
    new = {"shl_mi355x_conv_add_fusable", "shl_mi355x_conv_add_forward", "shl_mi355x_conv_add_kernel_name", "shl_mi355x_conv_add_by_default"}
    assert new <= _exports(pkg.lib_path("libshl_mi355x.so"))
    assert new <= set(pkg.load_hip().EXPORTS)
    assert "shl_mi355x_session_fused_residuals" in _exports(pkg.lib_path("libshl_mi355x_opt.so"))
    assert C.sizeof(pkg.ResidualDesc) == 32 and pkg.ResidualDesc.act.offset == 20 and pkg.ResidualDesc.out_zp.offset == 28


def test_without_a_plan_nothing_is_named_and_nothing_runs(built):
    hip = pkg.load_hip()
    d = pkg.ResidualDesc(1, 0.5, 0, 0.5, 0, 0, 0.5, 0)
    assert hip.shl_mi355x_conv_add_kernel_name(None, 1) == b""
    assert hip.shl_mi355x_conv_add_fusable(None, 1) == 0 and hip.shl_mi355x_conv_add_by_default(None, 1) == 0
    assert hip.shl_mi355x_conv_add_forward(None, 1 << 40, 1 << 41, 1 << 42, 1, C.byref(d), None) == EINVAL
    assert b"NULL argument" in hip.shl_mi355x_last_error()


def test_case_list_covers_what_it_must():
    cs = rc.all_cases() + rc.child_cases()
    assert {c["conv_first"] for c in cs} == {0, 1} and {c["act"] for c in cs} == {0, 1, 2}
    assert any(c["conv"]["act"] == 2 for c in cs), "a convolution with its own folded relu6"
    assert any(not c["conv"]["exact"] for c in cs), "converter scales"
    assert {rc.fma_div_of(c) for c in cs} == {0, 1}
    for key in ("skip_q", "sum_q", "out_q"):
        assert {-128, 0, 127} <= {c[key][1] for c in cs}, key
    assert any((c["skip"] == -128).all() for c in cs) and any((c["skip"] == 127).all() for c in cs)
    for form in ("wave", "tile"):
        assert any((c["skip"] == -128).all() and c["form"] == form for c in cs)
    shapes = {(c["form"], c["conv"]["n"] * c["conv"]["ho"] * c["conv"]["wo"], c["conv"]["co"], c["conv"]["c"], c["conv"]["kh"]) for c in cs}
    assert {("wave", 33, 36, 16, 1), ("wave", 33, 30, 16, 1), ("wave", 64, 32, 256, 1), ("wave", 35, 32, 16, 3), ("tile", 129, 130, 16, 1),
            ("tile", 257, 64, 64, 1)} <= shapes
    assert any(c["form"] == "wave" and c["conv"]["stride"] == (2, 2) and c["conv"]["h"] == 9 for c in cs)


@pytest.mark.parametrize("case", rc.all_cases() + rc.child_cases(), ids=lambda c: c["name"])
def test_the_oracle_chain_can_tell_results_apart(case):
    """an expected output that spreads (except under the sum scale of 2^41, which maps every sum to the zero point, and under an
    activation's output zero point of 127, which saturates every positive value), and a
    post-op that changes the convolution's bytes"""
    chain = rc.oracle_chain(case)
    import numpy as np
    if not rc.flat_by_record(case):
        assert len(np.unique(chain["out"])) > 8, case["name"]
    assert (chain["out"] != chain["conv"]).mean() > 0.5


# ------------------------------------------------------------------------------------ the host code under sanitizers
DRIVER = r"""
// Stand-alone driver of csrc/residual_validate.h, the host code of shl_mi355x_conv_add_forward: reads one call per line, prints
// its status and message.  Nothing is launched.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "residual_validate.h"

int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    long long v[12];
    double sc[3];
    unsigned long long p[3];
    // <present dtype layout algo in_pixels in_c out_pixels out_c plan_batch batch act conv_first> <3 scales> <3 addresses, 0 = NULL>
    for (;;) {
        int got = 0;
        for (int i = 0; i < 12; i++) got += fscanf(f, "%lld", &v[i]) == 1;
        if (got != 12) break;
        if (fscanf(f, "%lf %lf %lf %llu %llu %llu", &sc[0], &sc[1], &sc[2], &p[0], &p[1], &p[2]) != 6) return 3;
        shl::ResidualPlanFacts *facts = new shl::ResidualPlanFacts;  // on the heap: reads past them are caught
        shl_mi355x_residual_desc *d = new shl_mi355x_residual_desc;
        memset(facts, 0, sizeof(*facts));
        memset(d, 0, sizeof(*d));
        facts->present = (int32_t)v[0], facts->dtype = (int32_t)v[1], facts->layout = (int32_t)v[2], facts->algo = (int32_t)v[3];
        facts->in_pixels = v[4], facts->in_c = v[5], facts->out_pixels = v[6], facts->out_c = v[7], facts->plan_batch = (int32_t)v[8];
        d->act = (int32_t)v[10], d->conv_first = (int32_t)v[11];
        d->skip_scale = (float)sc[0], d->sum_scale = (float)sc[1], d->out_scale = (float)sc[2];
        const char *msg = NULL;
        const int st = shl::residual_validate(facts, (const void *)(uintptr_t)p[0], (const void *)(uintptr_t)p[1],
                                              (const void *)(uintptr_t)p[2], (int32_t)v[9], d, &msg);
        printf("%d|%s\n", st, msg ? msg : "");
        delete d;
        delete facts;
    }
    fclose(f);
    const char *forms[4] = {"wave", "tile", "regs", NULL};
    for (int i = 0; i < 4; i++) {
        const char *r = shl::residual_forced_form(forms[i]);
        printf("form|%s\n", r ? r : "-");
    }
    return 0;
}
"""

FAR = (1 << 40, 1 << 41, 1 << 42)
BASE = dict(present=1, dtype=pkg.SHL_I8, layout=pkg.SHL_NHWC, algo=ALGO_IGEMM, in_pixels=64, in_c=16, out_pixels=64, out_c=32, plan_batch=2,
            batch=0, act=1, conv_first=1, skip_scale=0.25, sum_scale=0.5, out_scale=0.125)
KEYS = ("present", "dtype", "layout", "algo", "in_pixels", "in_c", "out_pixels", "out_c", "plan_batch", "batch", "act", "conv_first")


def _problems():
    """(fields, (input, skip, output) addresses, expected status, a piece of the expected message)"""
    inp, skip, out = FAR
    nout, nin = 2 * 64 * 32, 2 * 64 * 16
    ps = [(dict(), FAR, 0, ""), (dict(batch=5, act=0, out_scale=float("nan")), FAR, 0, ""), (dict(act=2, conv_first=0), FAR, 0, ""),
          (dict(), (inp, inp, out), 0, ""),  # the skip tensor may be the input
          (dict(), (inp, skip, inp + nin), 0, ""), (dict(), (inp, out - nout, out), 0, "")]  # touching is fine
    ps += [(dict(present=0), FAR, EINVAL, "NULL argument")]
    ps += [(dict(), tuple(0 if j == i else p for j, p in enumerate(FAR)), EINVAL, "NULL argument") for i in range(3)]
    ps += [(dict(dtype=pkg.SHL_F16), FAR, ENOTSUP, "not int8"), (dict(layout=pkg.SHL_NCHW), FAR, ENOTSUP, "not int8"),
           (dict(algo=ALGO_DW), FAR, ENOTSUP, "not int8"), (dict(algo=ALGO_DECONV_GATHER), FAR, ENOTSUP, "transposed"),
           (dict(algo=ALGO_DECONV_PHASE), FAR, ENOTSUP, "transposed")]
    ps += [(dict(act=-1), FAR, EINVAL, "act"), (dict(act=3), FAR, EINVAL, "act")]
    for key in ("skip_scale", "sum_scale", "out_scale"):
        for bad in (0.0, -0.5, float("inf"), float("nan")):
            ps.append(({key: bad}, FAR, EINVAL, "scale"))
    ps += [(dict(), (out, skip, out), EINVAL, "overlaps the input"), (dict(), (out + nout - 1, skip, out), EINVAL, "overlaps the input"),
           (dict(), (out - nin + 1, skip, out), EINVAL, "overlaps the input"), (dict(), (inp, out, out), EINVAL, "overlaps the skip"),
           (dict(), (inp, out + 1, out), EINVAL, "overlaps the skip"), (dict(), (inp, out - nout + 1, out), EINVAL, "overlaps the skip"),
           (dict(batch=1 << 26), FAR, EINVAL, "2^31"), (dict(plan_batch=1 << 30, batch=0), FAR, EINVAL, "2^31"),
           (dict(), (inp, skip, (1 << 64) - 64), EINVAL, "wraps around")]
    return ps


def _line(fields, ptrs):
    f = dict(BASE, **fields)
    return " ".join(str(int(f[k])) for k in KEYS) + " " + " ".join(repr(float(f[k])) for k in ("skip_scale", "sum_scale", "out_scale")) + \
        " " + " ".join(str(int(p)) for p in ptrs)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc to compile with")
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on machines without a GPU")
def test_validation_runs_clean_under_address_and_undefined_sanitizers(built, tmp_path):
    """csrc/residual_validate.h compiled (-fsanitize=address,undefined) into a program of its own: every refusal gives its
    status and its message, every legal call passes"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    inc = os.path.join(cases.ROOT, "include")
    csrc = os.path.join(cases.ROOT, "csi-nn2_amd", "csrc")
    san = "-fsanitize=address,undefined"
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "residual_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-gpu-rdc", "-ffp-contract=off", "-Xarch_host", san,
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + inc, "-I" + csrc, "-x", "hip", "-c",
                    str(tmp_path / "driver.cpp"), "-o", str(tmp_path / "driver.o")], check=True)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fno-gpu-rdc", san, str(tmp_path / "driver.o"), "-o", exe], check=True)
    problems = _problems()
    (tmp_path / "problems.txt").write_text("\n".join(_line(f, p) for f, p, _, _ in problems) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe, str(tmp_path / "problems.txt")], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
    rows = [ln.split("|") for ln in res.stdout.splitlines()]
    assert [r[1] for r in rows if r[0] == "form"] == ["wave", "tile", "-", "-"]
    rows = [r for r in rows if r[0] != "form"]
    assert len(rows) == len(problems)
    for (fields, ptrs, status, text), row in zip(problems, rows):
        assert int(row[0]) == status and text in row[1] and (status != 0 or row[1] == ""), (fields, ptrs, row)
    assert {int(r[0]) for r in rows} == {0, EINVAL, ENOTSUP}

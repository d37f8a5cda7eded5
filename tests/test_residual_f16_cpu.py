"""The binary16 fused residual tail without a GPU: the exported entry points, what the library answers with no plan, the case
list's own conditions, and the call's validation and the default rule -- csrc/residual_validate.h, pure host code -- in a
stand-alone program under the address and undefined-behaviour sanitizers against a Python restatement."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases
import residual_f16_cases as rc
from cases import pkg

EINVAL, ENOTSUP = -2, -3
ALGO_IGEMM, ALGO_DW, ALGO_DECONV_GATHER, ALGO_DECONV_PHASE = pkg.ALGO_IGEMM, pkg.ALGO_DW, pkg.ALGO_DECONV_GATHER, pkg.ALGO_DECONV_PHASE
NEW = {"shl_mi355x_conv_add_f16_fusable", "shl_mi355x_conv_add_f16_forward", "shl_mi355x_conv_add_f16_kernel_name",
       "shl_mi355x_conv_add_f16_by_default"}


def _header_constants():
    text = open(os.path.join(cases.ROOT, "csi-nn2_amd", "csrc", "residual_validate.h")).read()
    return {m.group(1): int(eval(m.group(2), {"__builtins__": {}})) for m in
            re.finditer(r"constexpr int64_t (RESIDUAL_F16_\w+) = ([0-9 <]+);", text)}


def default_rule(M, Co, kbytes, taps, tile):
    """csrc/residual_validate.h:residual_f16_default restated, over the header's constants"""
    k = _header_constants()
    if tile:
        return taps == 1 and M >= k["RESIDUAL_F16_TILE_MIN_M"] and Co >= k["RESIDUAL_F16_TILE_MIN_CO"]
    return kbytes >= k["RESIDUAL_F16_WAVE_MIN_KBYTES"]


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_new_symbols_are_exported_and_declared(built):
    assert NEW <= _exports(pkg.lib_path("libshl_mi355x.so"))
    assert NEW <= set(pkg.load_hip().EXPORTS)
    header = open(os.path.join(cases.ROOT, "include", "shl_mi355x.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(const shl_mi355x_conv_plan \*plan" % name, header), name


def test_without_a_plan_nothing_is_named_and_nothing_runs(built):
    hip = pkg.load_hip()
    d = pkg.ResidualDesc(1, 0.0, 0, 0.0, 0, 0, 0.0, 0)
    assert hip.shl_mi355x_conv_add_f16_kernel_name(None, 1) == b""
    assert hip.shl_mi355x_conv_add_f16_fusable(None, 1) == 0 and hip.shl_mi355x_conv_add_f16_by_default(None, 1) == 0
    assert hip.shl_mi355x_conv_add_f16_forward(None, 1 << 40, 1 << 41, 1 << 42, 1, C.byref(d), None) == EINVAL
    assert b"NULL argument" in hip.shl_mi355x_last_error()


def test_case_list_covers_what_its_docstring_claims():
    cs = rc.all_cases() + rc.child_cases()
    assert all(c["conv"]["dtype"] == "f16" and c["conv"]["layout"] == cases.NHWC and c["skip"].dtype == np.float16 for c in cs)
    assert {c["conv_first"] for c in cs} == {0, 1} and {c["act"] for c in cs} == {0, 1, 2}
    assert any(c["conv"]["act"] == 2 for c in cs), "a convolution with its own folded relu6"
    shapes = {(c["form"], c["conv"]["n"] * c["conv"]["ho"] * c["conv"]["wo"], c["conv"]["co"], c["conv"]["c"], c["conv"]["kh"]) for c in cs}
    assert {("wave", 33, 36, 16, 1), ("wave", 33, 30, 16, 1), ("wave", 64, 32, 128, 1), ("wave", 35, 32, 16, 3), ("tile", 129, 144, 32, 1),
            ("tile", 129, 130, 16, 1), ("tile", 257, 64, 32, 1), ("tile", 130, 32, 8, 3)} <= shapes
    assert any(c["form"] == "wave" and c["conv"]["stride"] == (2, 2) and c["conv"]["h"] == 9 for c in cs)
    # store paths: wave 8-byte / element / split-K; tile staged (Co % 8 == 0) / 8-byte (Co % 4 == 0 only) / element
    wave = [c for c in cs if c["form"] == "wave"]
    tile = [c for c in cs if c["form"] == "tile"]
    assert any(c["conv"]["co"] % 4 == 0 for c in wave) and any(c["conv"]["co"] % 4 for c in wave)
    assert any(rc.splits_k(c) and rc.k_row_bytes(c) == 256 for c in wave) and any(not rc.splits_k(c) for c in wave)
    assert any(c["conv"]["co"] % 8 == 0 for c in tile) and any(c["conv"]["co"] % 8 == 4 for c in tile) and any(c["conv"]["co"] % 4 for c in tile)
    assert not any(rc.splits_k(c) for c in tile), "the stand-alone convolution of a tile case must add K up in the tile kernels' order"
    assert all(c["conv"]["c"] % 32 == 0 for c in rc.child_cases())
    # specials: both families, both operand orders, every pattern present, a NaN in the convolution's input
    sp = [c for c in cs if c["specials"]]
    assert {(c["form"], c["conv_first"]) for c in sp} == {("wave", 0), ("wave", 1), ("tile", 0), ("tile", 1)}
    for c in sp:
        assert set(rc.SPECIALS.tolist()) <= set(c["skip"].view(np.uint16).reshape(-1).tolist())
        assert np.isnan(c["conv"]["input"]).sum() == 1
    assert not any(np.isnan(c["conv"]["input"]).any() or not np.isfinite(c["skip"]).all() for c in cs if not c["specials"])


@pytest.mark.parametrize("case", [c for c in rc.all_cases() + rc.child_cases() if not c["specials"]], ids=lambda c: c["name"])
def test_the_oracle_chain_can_tell_results_apart(case):
    chain = rc.oracle_chain(case)
    assert len(np.unique(chain["out"])) > 8, case["name"]
    assert (chain["out"] != chain["conv"]).mean() > 0.5


# ------------------------------------------------------------------------------------ the host code under sanitizers
DRIVER = r"""
// Stand-alone driver of csrc/residual_validate.h, the host code of shl_mi355x_conv_add_f16_forward: reads one call per line,
// prints its status and message; then the default rule on a grid of shapes.  Nothing is launched.
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
        const int st = shl::residual_f16_validate(facts, (const void *)(uintptr_t)p[0], (const void *)(uintptr_t)p[1],
                                                  (const void *)(uintptr_t)p[2], (int32_t)v[9], d, &msg);
        printf("%d|%s\n", st, msg ? msg : "");
        delete d;
        delete facts;
    }
    fclose(f);
    printf("const|%lld|%lld|%lld\n", (long long)shl::RESIDUAL_F16_WAVE_MIN_KBYTES, (long long)shl::RESIDUAL_F16_TILE_MIN_M,
           (long long)shl::RESIDUAL_F16_TILE_MIN_CO);
    const long long Ms[] = {1, 49, 196, 784, 3136, 6272, 25088, 100351, 100352, 401408};
    const long long Cos[] = {24, 32, 64, 96, 160, 255, 256, 2048};
    const long long Ks[] = {64, 127, 128, 256, 320, 512, 1152, 9216};
    for (long long M : Ms)
        for (long long Co : Cos)
            for (long long K : Ks)
                for (int taps = 1; taps <= 9; taps += 8)
                    for (int tile = 0; tile < 2; tile++)
                        printf("rule|%lld|%lld|%lld|%d|%d|%d\n", M, Co, K, taps, tile, (int)shl::residual_f16_default(M, Co, K, taps, tile != 0));
    return 0;
}
"""

FAR = (1 << 40, 1 << 41, 1 << 42)
BASE = dict(present=1, dtype=pkg.SHL_F16, layout=pkg.SHL_NHWC, algo=ALGO_IGEMM, in_pixels=64, in_c=16, out_pixels=64, out_c=32, plan_batch=2,
            batch=0, act=1, conv_first=1, skip_scale=0.25, sum_scale=0.5, out_scale=0.125)
KEYS = ("present", "dtype", "layout", "algo", "in_pixels", "in_c", "out_pixels", "out_c", "plan_batch", "batch", "act", "conv_first")


def _problems():
    """(fields, (input, skip, output) addresses, expected status, a piece of the expected message)"""
    inp, skip, out = FAR
    nout, nin = 2 * 2 * 64 * 32, 2 * 2 * 64 * 16  # bytes: 2-byte elements
    ps = [(dict(), FAR, 0, ""), (dict(batch=5, act=0), FAR, 0, ""), (dict(act=2, conv_first=0), FAR, 0, ""),
          (dict(), (inp, inp, out), 0, ""),  # the skip tensor may be the input
          (dict(), (inp, skip, inp + nin), 0, ""), (dict(), (inp, out - nout, out), 0, "")]  # touching is fine
    # the scale fields are not read: what the int8 launch refuses passes
    for key in ("skip_scale", "sum_scale", "out_scale"):
        for odd in (0.0, -0.5, float("inf"), float("nan")):
            ps.append(({key: odd}, FAR, 0, ""))
    ps += [(dict(present=0), FAR, EINVAL, "NULL argument")]
    ps += [(dict(), tuple(0 if j == i else p for j, p in enumerate(FAR)), EINVAL, "NULL argument") for i in range(3)]
    ps += [(dict(dtype=pkg.SHL_I8), FAR, ENOTSUP, "not binary16"), (dict(layout=pkg.SHL_NCHW), FAR, ENOTSUP, "not binary16"),
           (dict(algo=ALGO_DW), FAR, ENOTSUP, "not binary16"), (dict(algo=pkg.ALGO_STEM), FAR, ENOTSUP, "not binary16"),
           (dict(algo=pkg.ALGO_DIRECT), FAR, ENOTSUP, "not binary16"), (dict(algo=ALGO_DECONV_GATHER), FAR, ENOTSUP, "transposed"),
           (dict(algo=ALGO_DECONV_PHASE), FAR, ENOTSUP, "transposed")]
    ps += [(dict(act=-1), FAR, EINVAL, "act"), (dict(act=3), FAR, EINVAL, "act")]
    ps += [(dict(), (out, skip, out), EINVAL, "overlaps the input"), (dict(), (out + nout - 1, skip, out), EINVAL, "overlaps the input"),
           (dict(), (out - nin + 1, skip, out), EINVAL, "overlaps the input"), (dict(), (inp, out, out), EINVAL, "overlaps the skip"),
           (dict(), (inp, out + nout - 2, out), EINVAL, "overlaps the skip"), (dict(), (inp, out - nout + 2, out), EINVAL, "overlaps the skip"),
           # (an output of int8 size would not reach: the sizes count 2-byte elements)
           (dict(), (inp, out + nout // 2, out), EINVAL, "overlaps the skip"),
           (dict(), (inp, skip + 1, out), EINVAL, "2-byte aligned"),
           (dict(batch=1 << 26), FAR, EINVAL, "2^31"), (dict(plan_batch=1 << 30, batch=0), FAR, EINVAL, "2^31"),
           (dict(), (inp, skip, (1 << 64) - 64), EINVAL, "wraps around")]
    return ps


def _line(fields, ptrs):
    f = dict(BASE, **fields)
    return " ".join(str(int(f[k])) for k in KEYS) + " " + " ".join(repr(float(f[k])) for k in ("skip_scale", "sum_scale", "out_scale")) + \
        " " + " ".join(str(int(p)) for p in ptrs)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc to compile with")
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on machines without a GPU")
def test_validation_and_default_rule_run_clean_under_address_and_undefined_sanitizers(built, tmp_path):
    """csrc/residual_validate.h compiled (-fsanitize=address,undefined) into a program of its own: every refusal gives its
    status and its message, every legal call passes, and the default rule answers as its Python restatement does"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    inc = os.path.join(cases.ROOT, "include")
    csrc = os.path.join(cases.ROOT, "csi-nn2_amd", "csrc")
    san = "-fsanitize=address,undefined"
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "residual_f16_host")
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
    consts = [r for r in rows if r[0] == "const"]
    k = _header_constants()
    assert [int(x) for x in consts[0][1:]] == [k["RESIDUAL_F16_WAVE_MIN_KBYTES"], k["RESIDUAL_F16_TILE_MIN_M"], k["RESIDUAL_F16_TILE_MIN_CO"]]
    rules = [r for r in rows if r[0] == "rule"]
    assert len(rules) == 10 * 8 * 8 * 2 * 2
    for r in rules:
        M, Co, K, taps, tile, ans = (int(x) for x in r[1:])
        assert bool(ans) == bool(default_rule(M, Co, K, taps, bool(tile))), r
    rows = [r for r in rows if r[0] not in ("const", "rule")]
    assert len(rows) == len(problems)
    for (fields, ptrs, status, text), row in zip(problems, rows):
        assert int(row[0]) == status and text in row[1] and (status != 0 or row[1] == ""), (fields, ptrs, row)
    assert {int(r[0]) for r in rows} == {0, EINVAL, ENOTSUP}

"""Table activations folded into the DEPTHWISE launch, without a GPU: the exported entry points and their bindings, what the
library answers with no plan, the case lists' coverage, and the call's host code -- the depthwise functions of
csrc/lut_validate.h -- in a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

import act_fuse_cases as ac
import cases
import dw_act_cases as dc
from cases import pkg

EINVAL, ENOTSUP = -2, -3
ALGO_IGEMM, ALGO_DW, ALGO_DECONV_GATHER, ALGO_DECONV_PHASE = pkg.ALGO_IGEMM, pkg.ALGO_DW, pkg.ALGO_DECONV_GATHER, pkg.ALGO_DECONV_PHASE
DOT4, MFMA, NHWC = 0, 1, 2  # DW_LUT_* of lut_validate.h
NEW = {"shl_mi355x_dwconv_lut_fusable", "shl_mi355x_dwconv_lut_forward", "shl_mi355x_dwconv_lut_kernel_name", "shl_mi355x_dwconv_lut_by_default"}


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_new_symbols_are_exported_and_bound(built):
    assert NEW <= _exports(pkg.lib_path("libshl_mi355x.so"))
    hip = pkg.load_hip()
    assert NEW <= set(hip.EXPORTS)
    for name in NEW:
        assert getattr(hip, name).argtypes is not None


def test_without_a_plan_nothing_is_named_and_nothing_runs(built):
    import numpy as np
    hip = pkg.load_hip()
    table = np.zeros(256, np.uint8)
    assert hip.shl_mi355x_dwconv_lut_kernel_name(None, 1) == b""
    assert hip.shl_mi355x_dwconv_lut_fusable(None, 1) == 0 and hip.shl_mi355x_dwconv_lut_by_default(None, 1) == 0
    assert hip.shl_mi355x_dwconv_lut_forward(None, 1 << 40, 1 << 41, 1, table.ctypes.data, None) == EINVAL
    assert b"dwconv_lut_forward: NULL argument" in hip.shl_mi355x_last_error()


def test_case_list_covers_what_it_must():
    cs = dc.all_cases() + dc.child_cases()
    convs = {c["shape"]: dc.conv_of(c["shape"]) for c in cs}
    for kernel in ("dot4", "nhwc", "mfma"):
        mine = [c for c in cs if c["kernel"] == kernel]
        assert {c["table"] for c in mine} == set(ac.TABLES), kernel
        by_shape = {}
        for c in mine:
            by_shape.setdefault(c["shape"], set()).add(c["table"])
        assert all("permutation" in t and len(t) >= 2 for t in by_shape.values()), kernel
        assert any(convs[s]["n"] == 2 for s in by_shape), kernel + ": a batch of 2"
    assert all(v["depthwise"] and v["co"] == v["c"] for v in convs.values())
    shapes = {(c["kernel"], convs[c["shape"]]["c"], convs[c["shape"]]["ho"], convs[c["shape"]]["wo"], convs[c["shape"]]["kh"],
               convs[c["shape"]]["kw"], convs[c["shape"]]["stride"][0]) for c in cs}
    assert {("dot4", 4, 3, 5, 3, 3, 1), ("dot4", 32, 2, 33, 3, 3, 1), ("nhwc", 8, 7, 7, 5, 5, 1), ("nhwc", 12, 5, 6, 5, 5, 2), ("nhwc", 8, 6, 7, 3, 5, 1),
            ("mfma", 32, 5, 7, 3, 3, 1), ("mfma", 64, 5, 5, 3, 3, 2), ("mfma", 128, 9, 17, 3, 3, 1)} <= shapes
    assert any(k == "mfma" and c == 96 for k, c, *_ in shapes)
    dot4 = [convs[c["shape"]] for c in cs if c["kernel"] == "dot4"]
    assert any(v["stride"] == (2, 2) and v["pad"][0] != v["pad"][2] for v in dot4), "stride 2 with asymmetric padding"
    assert any(v["dilation"] == (2, 2) for v in dot4) and any(v["act"] == 2 for v in dot4) and any(not v["exact"] for v in dot4)
    assert {v["out_zp"] for v in dot4} >= {-128, 127}
    # 264 positions per row: the second block in y has 8 busy lanes
    v = convs["dot4_c32_2x33"]
    assert v["wo"] * (v["c"] // 4) == 264


# ------------------------------------------------------------------------------------ the host code under sanitizers
DRIVER = r"""
// Stand-alone driver of the depthwise functions of csrc/lut_validate.h, the host code of shl_mi355x_dwconv_lut_forward.  Reads
// one call per line, prints its status and message; then the default rule on the grid of its arguments.  Nothing is launched.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "lut_validate.h"

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    long long v[12];
    unsigned long long p[3];
    // <present dtype layout algo in_pixels in_c out_pixels out_c plan_batch batch out_w kernel> <input, output, table addresses, 0 = NULL>
    for (;;) {
        int got = 0;
        for (int i = 0; i < 12; i++) got += fscanf(f, "%lld", &v[i]) == 1;
        if (got != 12) break;
        if (fscanf(f, "%llu %llu %llu", &p[0], &p[1], &p[2]) != 3) return 3;
        shl::LutPlanFacts *facts = new shl::LutPlanFacts;  // on the heap: reads past them are caught
        memset(facts, 0, sizeof(*facts));
        facts->present = (int32_t)v[0], facts->dtype = (int32_t)v[1], facts->layout = (int32_t)v[2], facts->algo = (int32_t)v[3];
        facts->in_pixels = v[4], facts->in_c = v[5], facts->out_pixels = v[6], facts->out_c = v[7], facts->plan_batch = (int32_t)v[8];
        const char *msg = NULL;
        const int st = shl::dw_lut_validate(v[0] == 2 ? NULL : facts, v[10], (int32_t)v[11], (const void *)(uintptr_t)p[0],
                                            (const void *)(uintptr_t)p[1], (int32_t)v[9], (const uint8_t *)(uintptr_t)p[2], &msg);
        printf("%d|%s\n", st, msg ? msg : "");
        delete facts;
    }
    fclose(f);
    // the default rule: <M C taps strided kernel> per line
    f = fopen(argv[2], "r");
    if (!f) return 2;
    long long r[5];
    while (fscanf(f, "%lld %lld %lld %lld %lld", &r[0], &r[1], &r[2], &r[3], &r[4]) == 5)
        printf("default|%d\n", shl::dw_lut_default(r[0], r[1], r[2], r[3] != 0, (int32_t)r[4]) ? 1 : 0);
    fclose(f);
    return 0;
}
"""

FAR = (1 << 40, 1 << 41, 1 << 42)
BASE = dict(present=1, dtype=pkg.SHL_I8, layout=pkg.SHL_NHWC, algo=ALGO_DW, in_pixels=64, in_c=32, out_pixels=64, out_c=32, plan_batch=2, batch=0,
            out_w=8, kernel=DOT4)
KEYS = ("present", "dtype", "layout", "algo", "in_pixels", "in_c", "out_pixels", "out_c", "plan_batch", "batch", "out_w", "kernel")
ROW_LIMIT = 65535 * 256  # (pixel, channel group) positions of the longest output row the dot4 grid takes


def _problems():
    """(fields, (input, output, table) addresses, expected status, a piece of the expected message)"""
    inp, out, tab = FAR
    nout = nin = 2 * 64 * 32
    ps = [(dict(), FAR, 0, ""), (dict(batch=5), FAR, 0, ""), (dict(), (inp, inp + nin, tab), 0, ""), (dict(), (out + nout, out, tab), 0, ""),
          (dict(batch=(1 << 25) - 1), FAR, 0, ""),  # touching is fine; 2^31 - 64 pixels are
          (dict(kernel=MFMA), FAR, 0, ""), (dict(kernel=NHWC), FAR, 0, "")]
    ps += [(dict(present=0), FAR, EINVAL, "NULL argument"), (dict(present=2), FAR, EINVAL, "NULL argument")]
    ps += [(dict(), tuple(0 if j == i else p for j, p in enumerate(FAR)), EINVAL, "NULL argument") for i in range(3)]
    ps += [(dict(dtype=pkg.SHL_F16), FAR, ENOTSUP, "not int8"), (dict(layout=pkg.SHL_NCHW), FAR, ENOTSUP, "not int8"),
           (dict(algo=ALGO_IGEMM), FAR, ENOTSUP, "not int8"), (dict(algo=pkg.ALGO_DIRECT), FAR, ENOTSUP, "not int8"),
           (dict(out_c=64), FAR, ENOTSUP, "depthwise"),
           (dict(algo=ALGO_DECONV_GATHER), FAR, ENOTSUP, "transposed"), (dict(algo=ALGO_DECONV_PHASE), FAR, ENOTSUP, "transposed")]
    ps += [(dict(), (out, out, tab), EINVAL, "overlaps the input"), (dict(), (out + nout - 1, out, tab), EINVAL, "overlaps the input"),
           (dict(), (out - nin + 1, out, tab), EINVAL, "overlaps the input"),
           (dict(batch=1 << 26), FAR, EINVAL, "2^31"), (dict(plan_batch=1 << 30, batch=0), FAR, EINVAL, "2^31"),
           (dict(batch=1 << 25), FAR, EINVAL, "2^31"), (dict(), (inp, (1 << 64) - 64, tab), EINVAL, "wraps around"),
           (dict(), ((1 << 64) - 64, out, tab), EINVAL, "wraps around")]
    # the dot4 grid: out_w * (C / 4) positions per row in blocks of 256, at most 65535 of them; the other kernels do not care
    wide = dict(in_pixels=1, out_pixels=ROW_LIMIT // 8, plan_batch=1)
    ps += [(dict(wide, out_w=ROW_LIMIT // 8), FAR, 0, ""), (dict(wide, out_w=ROW_LIMIT // 8 + 1, out_pixels=ROW_LIMIT // 8 + 1), FAR, ENOTSUP, "65535 blocks"),
           (dict(wide, out_w=ROW_LIMIT // 8 + 1, out_pixels=ROW_LIMIT // 8 + 1, kernel=NHWC), FAR, 0, ""),
           (dict(wide, out_w=ROW_LIMIT // 8 + 1, out_pixels=ROW_LIMIT // 8 + 1, kernel=MFMA), FAR, 0, "")]
    return ps


def _line(fields, ptrs):
    f = dict(BASE, **fields)
    return " ".join(str(int(f[k])) for k in KEYS) + " " + " ".join(str(int(p)) for p in ptrs)


def default_rule(M, C, taps, strided, kernel):
    """csrc/lut_validate.h:dw_lut_default restated from the measured table (profiles/dw_act_fuse_notes.md)"""
    E = M * C  # the bytes the second launch would read and write again
    if kernel == DOT4:  # 3x3 at batch 1 (196 x 184 the smallest) up to 1568 x 1152 at batch 32; 100352 x 144 was inside its spread
        return int(taps == 9 and 36064 <= E <= 1806336)
    if kernel == MFMA:  # 6272 x 480 up to 401408 x 32 at batch 32
        return int(taps == 9 and 3010560 <= E <= 12845056)
    # 5x5 from 49 x 672 at batch 1 up to 6272 x 672 at batch 32; 25088 x 240 won by no more than its spread
    return int(kernel == NHWC and taps == 25 and 32928 <= E <= 4214784)


# (M, C) on both sides of every bound, per kernel
_EDGES = {DOT4: ((196, 184), (1568, 1152)), MFMA: ((6272, 480), (401408, 32)), NHWC: ((49, 672), (6272, 672))}


def _rule_grid():
    """both sides of every number the rule turns on, for the three kernels, and the measured sizes under every kernel and tap count"""
    sizes = [(1, 4), (1, 32), ((1 << 31) - 1, 4), ((1 << 31) - 1, 1152), (100352, 144), (25088, 240), (25088, 144), (12544, 32), (3136, 144)]
    for (lo_m, lo_c), (hi_m, hi_c) in _EDGES.values():
        sizes += [(lo_m, lo_c), (lo_m, lo_c - 1), (lo_m - 1, lo_c), (lo_m, lo_c + 1), (hi_m, hi_c), (hi_m, hi_c + 1), (hi_m + 1, hi_c), (hi_m, hi_c - 1)]
    return [(M, C, taps, strided, kernel) for M, C in sizes for taps in (1, 9, 15, 25, 49) for strided in (0, 1) for kernel in (DOT4, MFMA, NHWC, 3)]


# the measured shapes (tools/dw_act_bench.py): (M, C, taps, strided, kernel) -> fused by default
MEASURED = (
    ((196, 240, 9, 1, DOT4), 1), ((196, 200, 9, 0, DOT4), 1), ((196, 184, 9, 0, DOT4), 1), ((196, 480, 9, 0, DOT4), 1), ((196, 672, 9, 0, DOT4), 1),
    ((12544, 32, 9, 0, DOT4), 1), ((3136, 144, 9, 0, DOT4), 1), ((49, 1152, 9, 0, DOT4), 1),
    ((49, 672, 25, 1, NHWC), 1), ((49, 960, 25, 0, NHWC), 1), ((784, 144, 25, 1, NHWC), 1), ((784, 240, 25, 0, NHWC), 1), ((196, 480, 25, 0, NHWC), 1),
    ((196, 672, 25, 0, NHWC), 1), ((49, 1152, 25, 0, NHWC), 1),
    ((6272, 240, 9, 1, DOT4), 1), ((6272, 200, 9, 0, DOT4), 1), ((6272, 184, 9, 0, DOT4), 1), ((6272, 480, 9, 0, MFMA), 1), ((6272, 672, 9, 0, MFMA), 1),
    ((401408, 32, 9, 0, MFMA), 1), ((100352, 144, 9, 0, DOT4), 0), ((1568, 1152, 9, 0, DOT4), 1),
    ((1568, 672, 25, 1, NHWC), 1), ((1568, 960, 25, 0, NHWC), 1), ((25088, 144, 25, 1, NHWC), 1), ((25088, 240, 25, 0, NHWC), 0), ((6272, 480, 25, 0, NHWC), 1),
    ((6272, 672, 25, 0, NHWC), 1), ((1568, 1152, 25, 0, NHWC), 1),
)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile with")
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on machines without a GPU")
def test_host_code_runs_clean_under_address_and_undefined_sanitizers(built, tmp_path):
    """the depthwise functions of csrc/lut_validate.h compiled (-fsanitize=address,undefined) into a program of its own: every
    refusal gives its status and its message, every legal call passes, and the default rule answers as its restatement on both
    sides of its boundaries"""
    inc = os.path.join(cases.ROOT, "include")
    csrc = os.path.join(cases.ROOT, "csi-nn2_amd", "csrc")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "dw_act_fuse_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + san + ["-I" + inc, "-I" + csrc, str(tmp_path / "driver.cpp"), "-o", exe],
                   check=True)
    problems, grid = _problems(), _rule_grid()
    (tmp_path / "problems.txt").write_text("\n".join(_line(f, p) for f, p, _, _ in problems) + "\n")
    (tmp_path / "rule.txt").write_text("\n".join(" ".join(str(v) for v in row) for row in grid) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe, str(tmp_path / "problems.txt"), str(tmp_path / "rule.txt")], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
    rows = [ln.split("|") for ln in res.stdout.splitlines()]
    answers = [default_rule(*row) for row in grid]
    assert [int(r[1]) for r in rows if r[0] == "default"] == answers and {0, 1} == set(answers)
    for kernel, ((lo_m, lo_c), (hi_m, hi_c)) in _EDGES.items():  # either side of each bound
        taps = 25 if kernel == NHWC else 9
        assert [default_rule(m, c, taps, 0, kernel) for m, c in ((lo_m, lo_c), (lo_m, lo_c - 1), (hi_m, hi_c), (hi_m, hi_c + 1))] == [1, 0, 1, 0]
    assert len(MEASURED) == 30
    for row, want in MEASURED:
        assert default_rule(*row) == want, row
    rows = [r for r in rows if r[0] != "default"]
    assert len(rows) == len(problems)
    for (fields, ptrs, status, text), row in zip(problems, rows):
        assert int(row[0]) == status and text in row[1] and (status != 0 or row[1] == ""), (fields, ptrs, row)
    assert {int(r[0]) for r in rows} == {0, EINVAL, ENOTSUP}

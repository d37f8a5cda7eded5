"""Table activations folded into the convolution's launch, without a GPU: the exported entry points, what the library answers
with no plan, the gate tables of shl_mi355x_gate_mul_table_i8 against the genuine library's 256 outputs
(tests/golden/act_fuse_cases.npz), and the call's host code -- csrc/lut_validate.h and the table builders of
source/mi355x_opt/eltwise.c -- in a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import act_fuse_cases as ac
import cases
import eltwise_cases as ec
from cases import pkg

EINVAL, ENOTSUP = -2, -3
ALGO_IGEMM, ALGO_DW, ALGO_DECONV_GATHER, ALGO_DECONV_PHASE = pkg.ALGO_IGEMM, pkg.ALGO_DW, pkg.ALGO_DECONV_GATHER, pkg.ALGO_DECONV_PHASE
GATES = ac.gate_cases()


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_new_symbols_are_exported(built):
    new = {"shl_mi355x_conv_lut_fusable", "shl_mi355x_conv_lut_forward", "shl_mi355x_conv_lut_kernel_name", "shl_mi355x_conv_lut_by_default"}
    assert new <= _exports(pkg.lib_path("libshl_mi355x.so"))
    assert new <= set(pkg.load_hip().EXPORTS)
    assert {"shl_mi355x_session_fused_activations", "shl_mi355x_gate_mul_table_i8"} <= _exports(pkg.lib_path("libshl_mi355x_opt.so"))


def test_without_a_plan_nothing_is_named_and_nothing_runs(built):
    hip = pkg.load_hip()
    table = np.zeros(256, np.uint8)
    assert hip.shl_mi355x_conv_lut_kernel_name(None, 1) == b""
    assert hip.shl_mi355x_conv_lut_fusable(None, 1) == 0 and hip.shl_mi355x_conv_lut_by_default(None, 1) == 0
    assert hip.shl_mi355x_conv_lut_forward(None, 1 << 40, 1 << 41, 1, table.ctypes.data, None) == EINVAL
    assert b"NULL argument" in hip.shl_mi355x_last_error()


def test_golden_file_holds_exactly_the_gate_cases():
    golden = ac.golden()
    assert sorted(golden) == sorted(c["name"] for c in GATES) and len(GATES) == 16
    assert {c["x_first"] for c in GATES} == {0, 1} and {c["kind"] for c in GATES} == set(ac.GATE_KINDS)
    for c in GATES:
        assert golden[c["name"]].dtype == np.int8 and golden[c["name"]].shape == (256,)
    zps = ac.GATE_TRIPLES["zps"]
    assert [r[1] for r in zps] == [-128, 0, 127]
    assert [r[1] for r in ac.GATE_TRIPLES["zps_neg"]] == [127, 0, 127]
    for key in ("pow2", "conv", "zps_neg"):  # the products spread
        assert np.unique(golden["gate_sigmoid_%s_x_first" % key]).size > 64, key


@pytest.mark.parametrize("case", GATES, ids=[c["name"] for c in GATES])
def test_gate_table_equals_the_genuine_librarys_outputs(standalone, case):
    """entry[b] is the byte the reference's mul gives for (b, act(b)) in the layer's operand order; the numpy restatement of
    the two layers agrees"""
    fe, hip, opt = standalone
    want = ac.golden()[case["name"]]
    assert np.array_equal(ac.by_q(ac.gate_table(opt, case)), want)
    assert np.array_equal(ac.gate_numpy(case), want)


def test_gate_byte_is_the_activations_own_table_entry(standalone):
    """mul by one with the gate's record as the output record hands the gate back: the gate inside the builder is the
    existing builder's"""
    fe, hip, opt = standalone
    for kind in ac.GATE_KINDS:
        qx, qg = ac.GATE_TRIPLES["conv"][0], ac.GATE_TRIPLES["conv"][1]
        act = np.zeros(256, np.uint8)
        getattr(opt, "shl_mi355x_%s_table_i8" % kind)(qx[0], qx[1], qg[0], qg[1], act.ctypes.data_as(ac.C.POINTER(ac.C.c_uint8)))
        want = ec.eltwise_numpy(dict(op=kind, dtype="int8", x=ac.EVERY, in_q=qx, out_q=qg, n=0.0))
        assert np.array_equal(ac.by_q(act), want)


def test_case_list_covers_what_it_must():
    cs = ac.all_cases() + ac.child_cases()
    assert {c["table"] for c in cs} == set(ac.TABLES)
    for form in ("wave", "tile"):
        assert {c["table"] for c in cs if c["form"] == form} >= {"sigmoid", "hard_sigmoid", "silu", "leaky_relu", "identity", "permutation", "gate"}
    assert {ac.TABLES[c["table"]][1][1] for c in cs if ac.TABLES[c["table"]][1]} >= {-128, 127}
    convs = {c["shape"]: ac.conv_of(c["shape"]) for c in cs}
    assert any(v["act"] == 2 for v in convs.values()), "a convolution with its own folded relu6"
    assert any(not v["exact"] for v in convs.values()), "converter scales"
    shapes = {(c["form"], convs[c["shape"]]["n"] * convs[c["shape"]]["ho"] * convs[c["shape"]]["wo"], convs[c["shape"]]["co"],
               convs[c["shape"]]["c"], convs[c["shape"]]["kh"]) for c in cs}
    assert {("wave", 33, 36, 16, 1), ("wave", 33, 30, 16, 1), ("wave", 64, 32, 256, 1), ("wave", 35, 32, 16, 3), ("tile", 129, 144, 64, 1),
            ("tile", 129, 130, 16, 1), ("tile", 257, 64, 64, 1)} <= shapes
    assert any(c["form"] == "wave" and convs[c["shape"]]["stride"] == (2, 2) and convs[c["shape"]]["h"] == 9 for c in cs)
    perm = ac.oracle_table(dict(shape="wave_1x1_m33_co36", table="permutation"))
    assert sorted(perm.view(np.uint8)) == list(range(256)) and (perm != ac.EVERY).mean() > 0.9


# ------------------------------------------------------------------------------------ the host code under sanitizers
DRIVER = r"""
// Stand-alone driver of csrc/lut_validate.h, the host code of shl_mi355x_conv_lut_forward, and of the gate table builder of
// source/mi355x_opt/eltwise.c.  Reads one call per line, prints its status and message; then the default rule on the grid of
// its arguments; then one gate table per line.  Nothing is launched.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "lut_validate.h"
extern "C" void shl_mi355x_gate_mul_table_i8(int kind, float x_scale, int32_t x_zp, float gate_scale, int32_t gate_zp, int x_is_first,
                                             float out_scale, int32_t out_zp, uint8_t table[256]);

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    long long v[10];
    unsigned long long p[3];
    // <present dtype layout algo in_pixels in_c out_pixels out_c plan_batch batch> <input, output, table addresses, 0 = NULL>
    for (;;) {
        int got = 0;
        for (int i = 0; i < 10; i++) got += fscanf(f, "%lld", &v[i]) == 1;
        if (got != 10) break;
        if (fscanf(f, "%llu %llu %llu", &p[0], &p[1], &p[2]) != 3) return 3;
        shl::LutPlanFacts *facts = new shl::LutPlanFacts;  // on the heap: reads past them are caught
        memset(facts, 0, sizeof(*facts));
        facts->present = (int32_t)v[0], facts->dtype = (int32_t)v[1], facts->layout = (int32_t)v[2], facts->algo = (int32_t)v[3];
        facts->in_pixels = v[4], facts->in_c = v[5], facts->out_pixels = v[6], facts->out_c = v[7], facts->plan_batch = (int32_t)v[8];
        const char *msg = NULL;
        const int st = shl::lut_validate(facts, (const void *)(uintptr_t)p[0], (const void *)(uintptr_t)p[1], (int32_t)v[9],
                                         (const uint8_t *)(uintptr_t)p[2], &msg);
        printf("%d|%s\n", st, msg ? msg : "");
        delete facts;
    }
    fclose(f);
    const char *forms[4] = {"wave", "tile", "regs", NULL};
    for (int i = 0; i < 4; i++) {
        const char *r = shl::lut_forced_form(forms[i]);
        printf("form|%s\n", r ? r : "-");
    }
    // the default rule: <M Co kbytes taps strided tile> per line
    f = fopen(argv[2], "r");
    if (!f) return 2;
    long long r[6];
    while (fscanf(f, "%lld %lld %lld %lld %lld %lld", &r[0], &r[1], &r[2], &r[3], &r[4], &r[5]) == 6)
        printf("default|%d\n", shl::lut_default(r[0], r[1], r[2], r[3], r[4] != 0, r[5] != 0) ? 1 : 0);
    fclose(f);
    // gate tables: <kind x_first x_zp gate_zp out_zp> <3 scales> per line, into 256 bytes on the heap
    if (argc > 3) {
        f = fopen(argv[3], "r");
        if (!f) return 2;
        long long g[5];
        double sc[3];
        while (fscanf(f, "%lld %lld %lld %lld %lld %lf %lf %lf", &g[0], &g[1], &g[2], &g[3], &g[4], &sc[0], &sc[1], &sc[2]) == 8) {
            uint8_t *table = new uint8_t[256];
            shl_mi355x_gate_mul_table_i8((int)g[0], (float)sc[0], (int32_t)g[2], (float)sc[1], (int32_t)g[3], (int)g[1], (float)sc[2],
                                         (int32_t)g[4], table);
            printf("gate|");
            for (int i = 0; i < 256; i++) printf("%02x", table[i]);
            printf("\n");
            delete[] table;
        }
        fclose(f);
    }
    return 0;
}
"""

FAR = (1 << 40, 1 << 41, 1 << 42)
BASE = dict(present=1, dtype=pkg.SHL_I8, layout=pkg.SHL_NHWC, algo=ALGO_IGEMM, in_pixels=64, in_c=16, out_pixels=64, out_c=32, plan_batch=2, batch=0)
KEYS = ("present", "dtype", "layout", "algo", "in_pixels", "in_c", "out_pixels", "out_c", "plan_batch", "batch")


def _problems():
    """(fields, (input, output, table) addresses, expected status, a piece of the expected message)"""
    inp, out, tab = FAR
    nout, nin = 2 * 64 * 32, 2 * 64 * 16
    ps = [(dict(), FAR, 0, ""), (dict(batch=5), FAR, 0, ""), (dict(), (inp, inp + nin, tab), 0, ""), (dict(), (out + nout, out, tab), 0, ""),
          (dict(batch=(1 << 25) - 1), FAR, 0, "")]  # touching is fine; 2^31 - 64 pixels are
    ps += [(dict(present=0), FAR, EINVAL, "NULL argument")]
    ps += [(dict(), tuple(0 if j == i else p for j, p in enumerate(FAR)), EINVAL, "NULL argument") for i in range(3)]
    ps += [(dict(dtype=pkg.SHL_F16), FAR, ENOTSUP, "not int8"), (dict(layout=pkg.SHL_NCHW), FAR, ENOTSUP, "not int8"),
           (dict(algo=ALGO_DW), FAR, ENOTSUP, "not int8"), (dict(algo=ALGO_DECONV_GATHER), FAR, ENOTSUP, "transposed"),
           (dict(algo=ALGO_DECONV_PHASE), FAR, ENOTSUP, "transposed")]
    ps += [(dict(), (out, out, tab), EINVAL, "overlaps the input"), (dict(), (out + nout - 1, out, tab), EINVAL, "overlaps the input"),
           (dict(), (out - nin + 1, out, tab), EINVAL, "overlaps the input"),
           (dict(batch=1 << 26), FAR, EINVAL, "2^31"), (dict(plan_batch=1 << 30, batch=0), FAR, EINVAL, "2^31"),
           (dict(batch=1 << 25), FAR, EINVAL, "2^31"), (dict(), (inp, (1 << 64) - 64, tab), EINVAL, "wraps around")]
    return ps


def _line(fields, ptrs):
    f = dict(BASE, **fields)
    return " ".join(str(int(f[k])) for k in KEYS) + " " + " ".join(str(int(p)) for p in ptrs)


def default_rule(M, Co, kbytes, taps, strided, tile):
    """csrc/lut_validate.h:lut_default restated from the measured table (profiles/act_fuse_notes.md)"""
    if not tile:  # six shapes at batch 1, 64 and more output channels, maps of 196 to 12544 pixels, 1x1 and 3x3
        return int(taps in (1, 9) and Co >= 64 and 196 <= M <= 12544)
    if M < 6272:
        return 0
    if taps == 1:  # 64 -> 64 @80 at batch 32 was inside the spread
        return int(Co >= 96)
    return int(taps == 9 and strided and kbytes <= 320)  # 3x3 stride 1 loses to the row-patch kernel


def _rule_grid():
    """both sides of every number the rule could turn on, for both families"""
    Ms = (1, 399, 400, 401, 1599, 1600, 1601, 6399, 6400, 6401, 12543, 12544, 12545, 25087, 25088, 25089, 200704, 401408, (1 << 31) - 1)
    Ms = Ms + (195, 196, 197, 6271, 6272, 6273)
    return [(M, Co, kb, taps, strided, tile) for M in Ms for Co in (16, 63, 64, 65, 95, 96, 97, 240, 512, 672)
            for kb in (64, 128, 319, 320, 321, 384, 512, 1152) for taps in (1, 9, 25) for strided in (0, 1) for tile in (0, 1)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile with")
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on machines without a GPU")
def test_host_code_runs_clean_under_address_and_undefined_sanitizers(built, tmp_path):
    """csrc/lut_validate.h and the table builders of eltwise.c compiled (-fsanitize=address,undefined) into a program of its own:
    every refusal gives its status and its message, every legal call passes, the default rule answers as its restatement on
    both sides of its boundaries, and the gate tables equal the golden bytes"""
    inc = os.path.join(cases.ROOT, "include")
    csrc = os.path.join(cases.ROOT, "csi-nn2_amd", "csrc")
    opt_dir = os.path.join(cases.ROOT, "csi-nn2_amd", "source", "mi355x_opt")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "act_fuse_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + san + ["-I" + inc, "-I" + csrc, "-c", str(tmp_path / "driver.cpp"),
                    "-o", str(tmp_path / "driver.o")], check=True)
    # the builders' file as the backend compiles it; its layer callbacks, which the program never calls, are dropped at the link
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu99", "-ffp-contract=off", "-ffunction-sections"] + san +
                   ["-I" + inc, "-I" + os.path.join(inc, "csinn"), "-I" + opt_dir, "-c", os.path.join(opt_dir, "eltwise.c"),
                    "-o", str(tmp_path / "eltwise.o")], check=True)
    subprocess.run(["g++"] + san + ["-Wl,--gc-sections", str(tmp_path / "driver.o"), str(tmp_path / "eltwise.o"), "-o", exe, "-lm"], check=True)
    problems, grid = _problems(), _rule_grid()
    (tmp_path / "problems.txt").write_text("\n".join(_line(f, p) for f, p, _, _ in problems) + "\n")
    (tmp_path / "rule.txt").write_text("\n".join(" ".join(str(v) for v in row) for row in grid) + "\n")
    (tmp_path / "gates.txt").write_text("\n".join(
        "%d %d %d %d %d %r %r %r" % (ec.KIND[c["kind"]], c["x_first"], c["q"][0][1], c["q"][1][1], c["q"][2][1], c["q"][0][0], c["q"][1][0],
                                     c["q"][2][0]) for c in GATES) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe, str(tmp_path / "problems.txt"), str(tmp_path / "rule.txt"), str(tmp_path / "gates.txt")], capture_output=True,
                         text=True, env=env, timeout=120)
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
    rows = [ln.split("|") for ln in res.stdout.splitlines()]
    assert [r[1] for r in rows if r[0] == "form"] == ["wave", "tile", "-", "-"]
    answers = [default_rule(*row) for row in grid]
    assert [int(r[1]) for r in rows if r[0] == "default"] == answers and {0, 1} == set(answers)
    # the measured shapes (tools/act_bench.py): M, Co, K bytes, taps, strided, tile -> fused by default
    for row, want in (((6400, 64, 320, 9, 1, 0), 1), ((6400, 64, 64, 1, 0, 0), 1), ((1600, 128, 1152, 9, 0, 0), 1), ((400, 512, 512, 1, 0, 0), 1),
                      ((12544, 96, 64, 1, 0, 0), 1), ((196, 672, 128, 1, 0, 0), 1), ((204800, 64, 320, 9, 1, 1), 1),
                      ((204800, 64, 64, 1, 0, 1), 0), ((51200, 128, 1152, 9, 0, 1), 0), ((12800, 512, 512, 1, 0, 1), 1),
                      ((401408, 96, 64, 1, 0, 1), 1), ((6272, 672, 128, 1, 0, 1), 1)):
        assert default_rule(*row) == want, row
    golden = ac.golden()
    gates = [np.frombuffer(bytes.fromhex(r[1]), np.uint8) for r in rows if r[0] == "gate"]
    assert len(gates) == len(GATES)
    for c, tab in zip(GATES, gates):
        assert np.array_equal(ac.by_q(tab), golden[c["name"]]), c["name"]
    rows = [r for r in rows if r[0] not in ("form", "default", "gate")]
    assert len(rows) == len(problems)
    for (fields, ptrs, status, text), row in zip(problems, rows):
        assert int(row[0]) == status and text in row[1] and (status != 0 or row[1] == ""), (fields, ptrs, row)
    assert {int(r[0]) for r in rows} == {0, EINVAL, ENOTSUP}

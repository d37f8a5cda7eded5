"""Kh x Kw int8 convolutions with 1..4 input channels on the matrix cores (csrc/conv_stem_kxk.hip): bit-exact against the oracle and
against the direct kernel it replaces; layers outside its scope keep today's kernel; nothing is written outside the output.
SHL_MI355X_STEMKXK is read per plan, but one sub-process per value (shared by the cases) keeps the two sides apart."""
import functools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [
    ("7x7_s2_23x19", dict(c=3, co=64, h=23, w=19, k=(7, 7), stride=(2, 2), pad=(3, 3, 3, 3))),                     # ragged tiles, odd fragment alignment
    ("7x7_s2_co40_n2_relu_nchw", dict(c=3, co=40, h=14, w=14, k=(7, 7), stride=(2, 2), pad=(3, 3, 3, 3), n=2, act=1, layout="NCHW")),  # out_c % 16, re-layout
    ("4x4_s4_co96", dict(c=3, co=96, h=16, w=20, k=(4, 4), stride=(4, 4), pad=(0, 0, 0, 0))),                       # kernel = stride, three channel blocks
    ("16x16_s16", dict(c=3, co=32, h=32, w=48, k=(16, 16), stride=(16, 16), pad=(0, 0, 0, 0))),                     # two steps per filter row
    ("5x5_s2_c1_tf", dict(c=1, co=32, h=13, w=13, k=(5, 5), stride=(2, 2), pad=(1, 1, 2, 2))),                      # TF-style asymmetric padding
    ("3x5_s1x2_c4_perch_relu6", dict(c=4, co=16, h=9, w=11, k=(3, 5), stride=(1, 2), pad=(1, 2, 1, 2), per_channel=True, act=2)),
    ("7x7_s1_c2_div", dict(c=2, co=24, h=8, w=8, k=(7, 7), pad=(3, 3, 3, 3), exact=False)),                         # IEEE-divide epilogue
    ("1x1_c3", dict(c=3, co=16, k=(1, 1), pad=(0, 0, 0, 0))),
    ("7x7_s2_70x70", dict(c=3, co=64, h=70, w=70, k=(7, 7), stride=(2, 2), pad=(3, 3, 3, 3))),                      # several rectangles, four tiles per wave
]
OUTSIDE = [
    ("3x3_c3_nhwc", dict(c=3, co=32), "conv_stem_i8_"),
    ("c5", dict(c=5, co=16, k=(5, 5), pad=(2, 2, 2, 2)), "conv_direct_i8"),
    ("dilation2", dict(c=3, co=16, k=(5, 5), pad=(4, 4, 4, 4), dilation=(2, 2)), "conv_direct_i8"),
    ("f16", dict(c=3, co=16, k=(5, 5), pad=(2, 2, 2, 2), dtype="f16"), "conv_direct_f16"),
    ("asymmetric_weights", dict(c=3, co=16, k=(5, 5), pad=(2, 2, 2, 2), kernel_zp=True), "conv_direct_i8_wzp"),
]
GUARDED = [0, 1]
NAME = "conv_stem_kxk_i8_mfma32x32x32"

SCRIPT = r"""
import ctypes as C, os, sys, zlib
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import cases, residual_cases as rc
from cases import pkg
import test_stem_kxk as me
fe = pkg.load_frontend("standalone")
hip, opt = pkg.load_backend(fe)
dev = cases.HipDevice(hip)
made = [cases.make_case(6100 + i, **s[1]) for i, s in enumerate(me.SHAPES + me.OUTSIDE)]
for i, case in enumerate(made):
    keep = []
    got = cases.csinn_run(fe, pkg.API_MI355X, case, device=dev, keep_params=keep)
    name = opt.shl_mi355x_params_kernel_name(keep[0][0]).decode()
    n, worst = cases.mismatch_report(got, cases.oracle_run(case, "exact")) if case["dtype"] == "int8" else (0, 0)  # (binary16: the CRCs)
    print("CASE", i, name, n, worst, zlib.crc32(got.tobytes()))
    opt.shl_mi355x_release_params(keep[0][0])
if os.environ["SHL_MI355X_STEMKXK"] == "1":  # shl_mi355x_conv_forward into an output with poisoned bytes on either side
    GUARD, POISON = 256, 0x5A
    for i in me.GUARDED:
        c = made[i]
        n, desc, plan = int(np.prod(c["out_shape"])), rc.conv_desc(c), C.c_void_p()
        mult = (np.float32(c["in_scale"]) * c["k_scale"] * np.ones(c["co"])).astype(np.float32)
        bias = (c["bias"] * c["b_scale"]).astype(np.float32)
        pkg.check(hip.shl_mi355x_conv_plan_create(C.byref(desc), c["kernel"].ctypes.data, mult.ctypes.data, bias.ctypes.data, None, C.byref(plan)), hip, "plan")
        d_in, d_out = dev.alloc(c["input"].nbytes), dev.alloc(n + 2 * GUARD)
        dev.upload(d_in, c["input"]), dev.upload(d_out, np.full(n + 2 * GUARD, POISON, np.uint8))
        pkg.check(hip.shl_mi355x_conv_forward(plan, d_in, d_out + GUARD, 0, None), hip, "conv_forward")
        whole, want = dev.download(d_out, (n + 2 * GUARD,), np.uint8), cases.oracle_run(c, "exact").view(np.uint8).reshape(-1)
        guards = np.concatenate([whole[:GUARD], whole[GUARD + n:]])
        print("GUARD", i, hip.shl_mi355x_conv_plan_kernel_name(plan).decode(), int(np.count_nonzero(whole[GUARD:GUARD + n] != want)), int(np.count_nonzero(guards != POISON)))
        dev.free(d_in), dev.free(d_out), hip.shl_mi355x_conv_plan_destroy(plan)
"""


@functools.lru_cache(maxsize=None)
def run(force):
    env = dict(os.environ, SHL_MI355X_STEMKXK=force)
    res = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=ROOT)], capture_output=True, text=True, timeout=600, env=env)
    rows = [l.split() for l in res.stdout.splitlines() if l.startswith(("CASE", "GUARD"))]
    assert len(rows) == len(SHAPES) + len(OUTSIDE) + (len(GUARDED) if force == "1" else 0), res.stdout + res.stderr
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[s[0] for s in SHAPES])
def test_stem_kxk_is_bit_exact_and_equals_the_direct_kernel(i):
    m, d = run("1")[i], run("0")[i]
    assert m[2] == NAME, m
    assert "direct" in d[2], d
    assert m[3] == "0", "matrix-core stem vs oracle: %s mismatches (max %s)" % (m[3], m[4])
    assert d[3] == "0", "direct kernel vs oracle: %s mismatches (max %s)" % (d[3], d[4])
    assert m[5] == d[5]


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(len(OUTSIDE)), ids=[s[0] for s in OUTSIDE])
def test_layers_outside_the_scope_keep_their_kernel(j):
    row = run("1")[len(SHAPES) + j]
    assert row[2].startswith(OUTSIDE[j][2]) and row[2] == run("0")[len(SHAPES) + j][2], row
    assert row[3] == "0", "%s vs oracle: %s mismatches" % (row[2], row[3])
    assert row[5] == run("0")[len(SHAPES) + j][5]


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(len(GUARDED)), ids=[SHAPES[i][0] for i in GUARDED])
def test_conv_forward_writes_the_output_and_nothing_beside_it(j):
    row = run("1")[len(SHAPES) + len(OUTSIDE) + j]
    assert row[:3] == ["GUARD", str(GUARDED[j]), NAME], row
    assert row[3:] == ["0", "0"], "differing bytes, bytes written outside the output: %s" % row[3:]

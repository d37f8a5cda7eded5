"""Grouped int8 NCHW convolution on the matrix cores (csrc/conv_group_mfma.hip): bit-exact against the oracle and against the
direct kernel it replaces; layers outside its scope stay on the direct kernel; nothing is written outside the output.
SHL_MI355X_GROUPMFMA is read once per process, so the forced runs happen in sub-processes (one per value, shared by the cases)."""
import functools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [
    ("c64_g16_9x7", dict(c=64, co=64, groups=16, h=9, w=7)),                                      # 4 per group, two units, ragged 63-pixel tile
    ("c64_g8_12x9_s2_n3_relu", dict(c=64, co=64, groups=8, h=12, w=9, stride=(2, 2), n=3, act=1)),  # stride-2 patch, three images
    ("c96_g6_7x7_perch", dict(c=96, co=96, groups=6, h=7, w=7, per_channel=True)),                # 16 per group, three units
    ("c64_g2_8x8", dict(c=64, co=64, groups=2)),                                                  # 32 = 32: the narrow / wide boundary
    ("c128_co64_g2_8x8", dict(c=128, co=64, groups=2)),                                           # 64 in, 32 out: two K slabs per tap
    ("c64_co128_g2_8x8", dict(c=64, co=128, groups=2)),                                           # 32 in, 64 out: two blocks, one window
    ("c64_g4_1x1", dict(c=64, co=64, groups=4, k=(1, 1), pad=(0, 0, 0, 0))),
    ("c64_g8_5x5_s2_tf", dict(c=64, co=64, groups=8, k=(5, 5), stride=(2, 2), pad=(1, 1, 2, 2))),  # TF-style padding
    ("c64_g4_div_relu6", dict(c=64, co=64, groups=4, exact=False, act=2)),                        # IEEE-divide epilogue
    ("c32_g8_40x40_n2", dict(c=32, co=32, groups=8, h=40, w=40, n=2)),                            # several rectangles, four tiles per wave
]
OUTSIDE = [
    ("c192_g96", dict(c=192, co=192, groups=96)),          # 2 per group
    ("c32_co64_g8", dict(c=32, co=64, groups=8)),          # 4 in, 8 out
    ("nhwc", dict(c=64, co=64, groups=8, layout="NHWC")),
    ("f16", dict(c=64, co=64, groups=8, dtype="f16")),
]
GUARDED = [0, 4]
NAME, DIRECT = "conv_group_mfma_i8_mfma32x32x32", "conv_group_direct_"

SCRIPT = r"""
import ctypes as C, os, sys, zlib
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import cases, residual_cases as rc
from cases import pkg
import test_group_mfma as me
fe = pkg.load_frontend("standalone")
hip, opt = pkg.load_backend(fe)
dev = cases.HipDevice(hip)
made = [cases.make_case(5200 + i, **dict(dict(layout="NCHW"), **kw)) for i, (_, kw) in enumerate(me.SHAPES + me.OUTSIDE)]
for i, case in enumerate(made):
    keep = []
    got = cases.csinn_run(fe, pkg.API_MI355X, case, device=dev, keep_params=keep)
    name = opt.shl_mi355x_params_kernel_name(keep[0][0]).decode()
    if case["dtype"] == "int8":
        n, worst = cases.mismatch_report(got, cases.oracle_group_run(case, "exact"))
    else:
        g, w = got.astype(np.float32), cases.oracle_group_run(case, "f16").astype(np.float32)
        n, worst = int(np.count_nonzero(np.abs(g - w) > 2e-3 * np.maximum(np.abs(w), 1.0))), 0
    print("CASE", i, name, n, worst, zlib.crc32(got.tobytes()))
    for p, _ in keep:
        opt.shl_mi355x_release_params(p)
if os.environ["SHL_MI355X_GROUPMFMA"] == "1":  # shl_mi355x_conv_forward into an output with poisoned bytes on either side
    GUARD, POISON = 256, 0x5A
    for i in me.GUARDED:
        c = made[i]
        n, desc, plan = int(np.prod(c["out_shape"])), rc.conv_desc(c), C.c_void_p()
        desc.algo = 7  # SHL_MI355X_ALGO_GROUP: the automatic choice refuses a grouped layer, the operator API asks for it by name
        mult = (np.float32(c["in_scale"]) * c["k_scale"] * np.ones(c["co"])).astype(np.float32)
        bias = (c["bias"] * c["b_scale"]).astype(np.float32)
        pkg.check(hip.shl_mi355x_conv_plan_create(C.byref(desc), c["kernel"].ctypes.data, mult.ctypes.data, bias.ctypes.data, None, C.byref(plan)), hip, "plan")
        d_in, d_out = dev.alloc(c["input"].nbytes), dev.alloc(n + 2 * GUARD)
        dev.upload(d_in, c["input"])
        dev.upload(d_out, np.full(n + 2 * GUARD, POISON, np.uint8))
        name = hip.shl_mi355x_conv_plan_kernel_name(plan).decode()
        pkg.check(hip.shl_mi355x_conv_forward(plan, d_in, d_out + GUARD, 0, None), hip, "conv_forward")
        whole = dev.download(d_out, (n + 2 * GUARD,), np.uint8)
        guards = np.concatenate([whole[:GUARD], whole[GUARD + n:]])
        want = cases.oracle_group_run(c, "exact").view(np.uint8).reshape(-1)
        print("GUARD", i, name, int(np.count_nonzero(whole[GUARD:GUARD + n] != want)), int(np.count_nonzero(guards != POISON)))
        dev.free(d_in), dev.free(d_out), hip.shl_mi355x_conv_plan_destroy(plan)
"""


@functools.lru_cache(maxsize=None)
def run(force):
    env = dict(os.environ, SHL_MI355X_GROUPMFMA=force)
    res = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=ROOT)], capture_output=True, text=True, timeout=600, env=env)
    rows = [l.split() for l in res.stdout.splitlines() if l.startswith(("CASE", "GUARD"))]
    assert len(rows) == len(SHAPES) + len(OUTSIDE) + (len(GUARDED) if force == "1" else 0), res.stdout + res.stderr
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[s[0] for s in SHAPES])
def test_grouped_mfma_is_bit_exact_and_equals_the_direct_kernel(i):
    m, d = run("1")[i], run("0")[i]
    assert m[2] == NAME, m
    assert d[2] == DIRECT + "i8", d
    assert m[3] == "0", "matrix-core grouped vs oracle: %s mismatches (max %s)" % (m[3], m[4])
    assert d[3] == "0", "direct grouped vs oracle: %s mismatches (max %s)" % (d[3], d[4])
    assert m[5] == d[5]


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(len(OUTSIDE)), ids=[s[0] for s in OUTSIDE])
def test_layers_outside_the_scope_stay_on_the_direct_kernel(j):
    row = run("1")[len(SHAPES) + j]
    assert row[2].startswith(DIRECT), row
    assert row[3] == "0", "direct grouped vs oracle: %s mismatches" % row[3]


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(len(GUARDED)), ids=[SHAPES[i][0] for i in GUARDED])
def test_conv_forward_writes_the_output_and_nothing_beside_it(j):
    row = run("1")[len(SHAPES) + len(OUTSIDE) + j]
    assert row[:3] == ["GUARD", str(GUARDED[j]), NAME], row
    assert row[3:] == ["0", "0"], "differing bytes, bytes written outside the output: %s" % row[3:]

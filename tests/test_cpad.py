"""Dense int8 convolutions whose input channel count is no multiple of 16, on the matrix cores (csrc/conv_igemm_cpad.hip): bit-exact
against the oracle and the direct kernel it replaces; layers outside its scope keep today's kernel; nothing is written outside the
output; a plan serves a smaller runtime batch.  SHL_MI355X_CPAD is read per plan; one sub-process per value keeps the sides apart."""
import functools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P0 = (0, 0, 0, 0)

SHAPES = [
    ("1x1_c24_co40_9x7", dict(c=24, co=40, h=9, w=7, k=(1, 1), pad=P0)),                                         # ragged M = 63, co % 32 = 8
    ("1x1_c58_co58_n2_6x5", dict(c=58, co=58, h=6, w=5, n=2, k=(1, 1), pad=P0)),                                 # byte-granular staging, byte stores
    ("1x1_s2_c72_co24_relu", dict(c=72, co=24, h=9, w=9, k=(1, 1), stride=(2, 2), pad=P0, act=1)),              # stride 2
    ("3x3_s2_c8_co16_tf", dict(c=8, co=16, h=9, w=9, stride=(2, 2), pad=(0, 0, 1, 1))),                           # Cp = 16, nine chunks, the zero half step
    ("3x3_c40_co24_perch_relu6", dict(c=40, co=24, per_channel=True, act=2)),                                    # Cp = 48, steps straddling taps
    ("3x3_c20_co20_div", dict(c=20, co=20, exact=False)),                                                        # div_fma, 12 pad bytes per pixel
    ("5x5_s2_c12_co32_13x11", dict(c=12, co=32, h=13, w=11, k=(5, 5), stride=(2, 2), pad=(2, 2, 2, 2))),         # larger kernel, stride 2
    ("3x3_c232_co32_5x5", dict(c=232, co=32, h=5, w=5)),                                                         # 15 chunks per tap, 68 steps, two tiles
    ("3x3_c24_co32_n2_relu_nchw", dict(c=24, co=32, n=2, act=1, layout="NCHW")),                                 # the re-layout path
    ("1x1_c24_co16_70x70", dict(c=24, co=16, h=70, w=70, k=(1, 1), pad=P0)),                                     # 39 flat rectangles of four tiles, one tile per wave
    ("1x1_c24_co72_296x296", dict(c=24, co=72, h=296, w=296, k=(1, 1), pad=P0)),                                 # flat, eight tiles per workgroup: four and two per wave
    ("3x3_c24_co32_n2_20x40", dict(c=24, co=32, n=2, h=20, w=40)),                                               # 3 x 3 rectangles of 2 x 2 tiles per image, two images in grid.z
    ("3x3_c232_co32_12x16", dict(c=232, co=32, h=12, w=16)),                                                     # 2 x 2 tiles, a 43 920-byte patch: 89 % of the LDS budget
    ("3x3_c8_co72_148x296", dict(c=8, co=72, h=148, w=296)),                                                     # 19 x 19 rectangles of 2 x 2 tiles: two per wave, one in the last block
]
OUTSIDE = [
    ("3x3_c16", dict(c=16, co=16), "conv_igemm_"),
    ("5x5_c5", dict(c=5, co=16, k=(5, 5), pad=(2, 2, 2, 2)), "conv_direct_i8"),
    ("dilation2", dict(c=24, co=16, pad=(2, 2, 2, 2), dilation=(2, 2)), "conv_direct_i8"),
    ("f16", dict(c=12, co=16, dtype="f16"), "conv_direct_f16"),
    ("asymmetric_weights", dict(c=24, co=16, kernel_zp=True), "conv_direct_i8_wzp"),
]
GUARDED, BATCHES, NAME = [1, 6], (1, 3), "conv_igemm_cpad_i8_mfma32x32x32"  # (BATCHES: runtime batches of a plan created for batch 4)

SCRIPT = r"""
import ctypes as C, os, sys, zlib
sys.path[:0] = [%(root)r, %(root)r + "/tests"]
import numpy as np
import cases, golden_util, residual_cases as rc, test_cpad as me
pkg = cases.pkg
fe = pkg.load_frontend("standalone")
hip, opt = pkg.load_backend(fe)
dev = cases.HipDevice(hip)
made = [cases.make_case(7300 + i, **s[1]) for i, s in enumerate(me.SHAPES + me.OUTSIDE)]
for i, case in enumerate(made):
    keep = []
    got = cases.csinn_run(fe, pkg.API_MI355X, case, device=dev, keep_params=keep)
    name = opt.shl_mi355x_params_kernel_name(keep[0][0]).decode()
    n, worst = cases.mismatch_report(got, cases.oracle_run(case, "exact")) if case["dtype"] == "int8" else (0, 0)
    if case["dtype"] != "int8": golden_util.compare_f16_tol(got, cases.oracle_run(case), "binary16, direct kernel")  # (raises: the row is then missing)
    print("CASE", i, name, n, worst, zlib.crc32(got.tobytes()))
    opt.shl_mi355x_release_params(keep[0][0])
if os.environ["SHL_MI355X_CPAD"] == "1":
    def forward(c, batch, tag, GUARD=256, POISON=0x5A):  # shl_mi355x_conv_forward into an output with poisoned bytes on either side
        n, plan = int(np.prod(c["out_shape"])) // c["n"] * (batch or c["n"]), rc.make_plan(hip, c)
        d_in, d_out = dev.alloc(c["input"].nbytes), dev.alloc(n + 2 * GUARD)
        dev.upload(d_in, c["input"]), dev.upload(d_out, np.full(n + 2 * GUARD, POISON, np.uint8))
        pkg.check(hip.shl_mi355x_conv_forward(plan, d_in, d_out + GUARD, batch, None), hip, "conv_forward")
        whole, want = dev.download(d_out, (n + 2 * GUARD,), np.uint8), cases.oracle_run(c, "exact").view(np.uint8).reshape(-1)[:n]
        guards = np.concatenate([whole[:GUARD], whole[GUARD + n:]])
        print(tag, hip.shl_mi355x_conv_plan_kernel_name(plan).decode(), int(np.count_nonzero(whole[GUARD:GUARD + n] != want)), int(np.count_nonzero(guards != POISON)))
        dev.free(d_in), dev.free(d_out), hip.shl_mi355x_conv_plan_destroy(plan)
    for i in me.GUARDED: forward(made[i], 0, "GUARD")
    for b in me.BATCHES: forward(cases.make_case(7399, c=40, co=24, h=7, w=6, n=4, act=1), b, "BATCH")
"""


@functools.lru_cache(maxsize=None)
def run(force):
    res = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=ROOT)], capture_output=True, text=True, timeout=600, env=dict(os.environ, SHL_MI355X_CPAD=force))
    rows = [l.split() for l in res.stdout.splitlines() if l.startswith(("CASE", "GUARD", "BATCH"))]
    assert len(rows) == len(SHAPES) + len(OUTSIDE) + (len(GUARDED) + len(BATCHES) if force == "1" else 0), res.stdout + res.stderr
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[s[0] for s in SHAPES])
def test_cpad_is_bit_exact_and_equals_the_direct_kernel(i):
    m, d = run("1")[i], run("0")[i]
    assert m[2] == NAME, m
    assert "direct" in d[2], d
    assert m[3] == "0", "matrix-core kernel vs oracle: %s mismatches (max %s)" % (m[3], m[4])
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
@pytest.mark.parametrize("j", range(len(GUARDED) + len(BATCHES)), ids=[SHAPES[i][0] for i in GUARDED] + ["batch4_runs_%d" % b for b in BATCHES])
def test_conv_forward_writes_the_output_and_nothing_beside_it(j):
    row = run("1")[len(SHAPES) + len(OUTSIDE) + j]
    assert row[:2] == ["GUARD" if j < len(GUARDED) else "BATCH", NAME], row
    assert row[2:] == ["0", "0"], "differing bytes, bytes written outside the output: %s" % row[2:]

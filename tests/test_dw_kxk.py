"""Depthwise Kh x Kw other than 3x3 on the matrix cores (csrc/dwconv_kxk.hip): bit-exact against the oracle and against the
generic kernel it replaces, and its fused launch with a table activation against the two launches.  SHL_MI355X_DWKXK is read
once per process, so the forced runs happen in sub-processes (one per value, shared by the cases)."""
import functools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [
    ("c32_9x9_5x5", dict(c=32, h=9, w=9, k=(5, 5), pad=(2, 2, 2, 2))),                                # one group, one rectangle
    ("c64_12x9_5x5_s2", dict(c=64, h=12, w=9, k=(5, 5), stride=(2, 2), pad=(2, 2, 2, 2))),            # ragged last tile, stride-2 patch
    ("c96_7x7_7x7_n3", dict(c=96, h=7, w=7, n=3, k=(7, 7), pad=(3, 3, 3, 3))),                        # mostly padding, three images, cb = 32
    ("c128_9x11_5x3_s21_relu6", dict(c=128, h=9, w=11, k=(5, 3), stride=(2, 1), pad=(2, 1, 2, 1), act=2)),
    ("c64_8x8_5x5_s2_tf", dict(c=64, h=8, w=8, k=(5, 5), stride=(2, 2), pad=(1, 1, 2, 2))),           # TF-style padding
    ("c160_10x10_5x5_div", dict(c=160, h=10, w=10, k=(5, 5), pad=(2, 2, 2, 2), exact=False, act=1)),  # IEEE-divide epilogue
    ("c64_6x6_7x7_perch", dict(c=64, h=6, w=6, k=(7, 7), pad=(3, 3, 3, 3), per_channel=True)),
    ("c256_7x7_5x5", dict(c=256, h=7, w=7, k=(5, 5), pad=(2, 2, 2, 2))),                              # two channel blocks of 128
    ("c32_40x40_5x5_n2", dict(c=32, h=40, w=40, n=2, k=(5, 5), pad=(2, 2, 2, 2), act=1)),             # four tiles per wave
    ("c32_6x6_1x7", dict(c=32, h=6, w=6, k=(1, 7), pad=(0, 3, 0, 3))),                                # the degenerate axis
]
LUT_SHAPES = [0, 1, 6]  # 5x5 stride 1, 5x5 stride 2, 7x7

SCRIPT = r"""
import os, sys, zlib
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import cases, residual_cases as rc
from cases import pkg
import test_dw_kxk as me
fe = pkg.load_frontend("standalone")
hip, opt = pkg.load_backend(fe)
dev = cases.HipDevice(hip)
made = [cases.make_case(4100 + i, depthwise=True, **kw) for i, (_, kw) in enumerate(me.SHAPES)]
for i, case in enumerate(made):
    keep = []
    got = cases.csinn_run(fe, pkg.API_MI355X, case, device=dev, keep_params=keep)
    name = opt.shl_mi355x_params_kernel_name(keep[0][0]).decode()
    n, worst = cases.mismatch_report(got, cases.oracle_run(case, "exact"))
    print("CASE", i, name, n, worst, zlib.crc32(got.tobytes()))
    for p, _ in keep:
        opt.shl_mi355x_release_params(p)
if os.environ["SHL_MI355X_DWKXK"] == "1":  # the fused launch against conv_forward + unary_lut_i8 on the same buffers
    GUARD, POISON = 256, 0x5A
    table = np.random.default_rng(7).permutation(256).astype(np.uint8)  # tells every byte value and byte lane apart
    for i in me.LUT_SHAPES:
        c = made[i]
        n = int(np.prod(c["out_shape"]))
        plan = rc.make_plan(hip, c)
        d_in, d_conv, d_un, d_f = dev.alloc(c["input"].nbytes), dev.alloc(n), dev.alloc(n), dev.alloc(n + 2 * GUARD)
        dev.upload(d_in, c["input"])
        dev.upload(d_f, np.full(n + 2 * GUARD, POISON, np.uint8))
        name = hip.shl_mi355x_dwconv_lut_kernel_name(plan, 0).decode()
        pkg.check(hip.shl_mi355x_dwconv_lut_forward(plan, d_in, d_f + GUARD, 0, table.ctypes.data, None), hip, "dwconv_lut_forward")
        pkg.check(hip.shl_mi355x_conv_forward(plan, d_in, d_conv, 0, None), hip, "conv_forward")
        pkg.check(hip.shl_mi355x_unary_lut_i8(d_conv, d_un, n, table.ctypes.data, None), hip, "unary_lut_i8")
        whole, unfused = dev.download(d_f, (n + 2 * GUARD,), np.uint8), dev.download(d_un, (n,), np.uint8)
        guards = np.concatenate([whole[:GUARD], whole[GUARD + n:]])
        print("LUT", i, name, int(np.count_nonzero(whole[GUARD:GUARD + n] != unfused)), int(np.count_nonzero(guards != POISON)))
        for p in (d_in, d_conv, d_un, d_f):
            dev.free(p)
        hip.shl_mi355x_conv_plan_destroy(plan)
"""


@functools.lru_cache(maxsize=None)
def run(force):
    env = dict(os.environ, SHL_MI355X_DWKXK=force)
    res = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=ROOT)], capture_output=True, text=True, timeout=600, env=env)
    rows = [l.split() for l in res.stdout.splitlines() if l.startswith(("CASE", "LUT"))]
    assert len(rows) == len(SHAPES) + (len(LUT_SHAPES) if force == "1" else 0), res.stdout + res.stderr
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[s[0] for s in SHAPES])
def test_kxk_depthwise_is_bit_exact_and_equals_the_generic_kernel(i):
    m, d = run("1")[i], run("0")[i]
    assert m[2] == "dwconv_kxk_mfma_i8", m
    assert d[2] == "dwconv_nhwc_i8", d
    assert m[3] == "0", "kxk depthwise vs oracle: %s mismatches (max %s)" % (m[3], m[4])
    assert d[3] == "0", "generic depthwise vs oracle: %s mismatches (max %s)" % (d[3], d[4])
    assert m[5] == d[5]


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(len(LUT_SHAPES)), ids=[SHAPES[i][0] for i in LUT_SHAPES])
def test_kxk_fused_table_launch_equals_the_two_launches(j):
    row = run("1")[len(SHAPES) + j]
    assert row[:3] == ["LUT", str(LUT_SHAPES[j]), "dwconv_kxk+lut"], row
    assert row[3:] == ["0", "0"], "differing bytes, bytes written outside the output: %s" % row[3:]

"""Depthwise NCHW layers whose kernel is not 3x3 (csrc/dwconv_kxk_nchw.hip), int8 and binary16: bit-identical to the direct kernel
they ran on, int8 bit-exact against the oracle; layers outside its scope keep today's kernel; nothing is written outside the output;
a plan serves a smaller runtime batch.  SHL_MI355X_DWNCHW is read per plan, so both sides run in this process."""
import functools
import os
from unittest import mock

import numpy as np
import pytest

import cases
import golden_util
import residual_cases as rc

pkg, NCHW = cases.pkg, cases.NCHW
P2, P3 = (2, 2, 2, 2), (3, 3, 3, 3)
SHAPES = [
    ("5x5_c5_7x7", dict(c=5, h=7, w=7, k=(5, 5), pad=P2)),                                        # odd plane size, several planes per workgroup, a short last one
    ("7x7_c8_n2_9x11", dict(c=8, h=9, w=11, n=2, k=(7, 7), pad=P3)),                              # two images, two dot4s per row
    ("5x5_s2_c4_12x9", dict(c=4, h=12, w=9, k=(5, 5), stride=(2, 2), pad=P2)),                    # stride-2 windows, ragged last column group
    ("5x5_s2_c6_tf", dict(c=6, h=8, w=8, k=(5, 5), stride=(2, 2), pad=(1, 1, 2, 2))),             # TF-style asymmetric padding
    ("5x3_s2x1_c4_relu6", dict(c=4, h=9, w=11, k=(5, 3), stride=(2, 1), pad=(2, 1, 2, 1), act=2)),  # anisotropic kernel and strides
    ("1x7_c4", dict(c=4, h=6, w=6, k=(1, 7), pad=(0, 3, 0, 3))),                                  # degenerate axis
    ("7x1_c4", dict(c=4, h=6, w=6, k=(7, 1), pad=(3, 0, 3, 0))),                                  # the other one
    ("7x7_c3_6x6_perch", dict(c=3, h=6, w=6, k=(7, 7), pad=P3, per_channel=True)),                # mostly padding, per-channel records
    ("5x5_c2_n2_40x40_relu", dict(c=2, h=40, w=40, n=2, k=(5, 5), pad=P2, act=1)),                # several rectangles per plane
    ("5x5_c2_5x70", dict(c=2, h=5, w=70, k=(5, 5), pad=P2)),                                      # more than one rectangle along W
    ("4x4_c4_9x9_nopad", dict(c=4, h=9, w=9, k=(4, 4), pad=(0, 0, 0, 0))),                        # even kernel, output smaller than input
    ("5x5_c5_7x7_div", dict(c=5, h=7, w=7, k=(5, 5), pad=P2, exact=False)),                       # a converter's scales: the div_fma epilogue
]
OUTSIDE = [  # with the switch at 1 these keep today's name and bytes (exact=False keeps the fast epilogue: in scope, the last of SHAPES)
    ("3x3", dict(c=8, layout=NCHW), "dwconv3x3_nchw_", ("int8", "f16")),
    ("dilation2", dict(c=4, h=12, w=12, k=(5, 5), pad=(4, 4, 4, 4), dilation=(2, 2), layout=NCHW), "conv_direct_", ("int8", "f16")),
    ("multiplier2", dict(c=4, k=(5, 5), pad=P2, multiplier=2, layout=NCHW), "conv_direct_", ("int8", "f16")),
    ("asymmetric_weights", dict(c=4, k=(5, 5), pad=P2, kernel_zp=True, layout=NCHW), "conv_direct_i8_wzp", ("int8",)),
    ("nhwc", dict(c=8, k=(5, 5), pad=P2), "", ("int8",)),
]
NAMES = {"int8": "dwconv_kxk_nchw_i8", "f16": "dwconv_kxk_nchw_f16"}
GUARD, POISON = 256, 0x5A


def switch(value):
    return mock.patch.dict(os.environ, SHL_MI355X_DWNCHW=value)


def layer(standalone, case, value):
    """(kernel name, output) of the case through csinn_conv2d*, the plan created under SHL_MI355X_DWNCHW=value"""
    fe, hip, opt = standalone
    keep = []
    with switch(value):
        got = cases.csinn_run(fe, pkg.API_MI355X, case, device=cases.HipDevice(hip), keep_params=keep)
    name = opt.shl_mi355x_params_kernel_name(keep[0][0]).decode()
    opt.shl_mi355x_release_params(keep[0][0])
    return name, got


@functools.lru_cache(maxsize=None)
def shape_case(i, dtype):
    return cases.make_case(7500 + i, depthwise=True, layout=NCHW, dtype=dtype, **SHAPES[i][1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "f16"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[s[0] for s in SHAPES])
def test_equals_the_direct_kernel_and_the_oracle(standalone, i, dtype):
    case = shape_case(i, dtype)
    (new_name, new), (old_name, old) = layer(standalone, case, "1"), layer(standalone, case, "0")
    assert new_name == NAMES[dtype]
    assert "direct" in old_name
    if dtype == "int8":
        want = cases.oracle_run(case, "exact")
        assert cases.mismatch_report(new, want)[0] == 0 and cases.mismatch_report(old, want)[0] == 0
    else:
        golden_util.compare_f16_tol(old, cases.oracle_run(case), "binary16, direct kernel")
    assert new.tobytes() == old.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("j,dtype", [(j, dt) for j, o in enumerate(OUTSIDE) for dt in o[3]], ids=lambda v: OUTSIDE[v][0] if isinstance(v, int) else v)
def test_layers_outside_the_scope_keep_their_kernel(standalone, j, dtype):
    case = cases.make_case(7600 + j, depthwise=True, dtype=dtype, **OUTSIDE[j][1])
    (new_name, new), (old_name, old) = layer(standalone, case, "1"), layer(standalone, case, "0")
    assert new_name == old_name and new_name.startswith(OUTSIDE[j][2]) and "dwconv_kxk_nchw" not in new_name
    assert new.tobytes() == old.tobytes()


def forward(hip, case, batch, value):
    """shl_mi355x_conv_forward into an output with poisoned bytes on either side: (kernel name, output bytes, guard bytes changed)"""
    dev = cases.HipDevice(hip)
    n = int(np.prod(case["out_shape"])) // case["n"] * (batch or case["n"]) * case["input"].itemsize
    with switch(value):
        plan = rc.make_plan(hip, case)
    d_in, d_out = dev.alloc(case["input"].nbytes), dev.alloc(n + 2 * GUARD)
    dev.upload(d_in, case["input"]), dev.upload(d_out, np.full(n + 2 * GUARD, POISON, np.uint8))
    pkg.check(hip.shl_mi355x_conv_forward(plan, d_in, d_out + GUARD, batch, None), hip, "conv_forward")
    whole, name = dev.download(d_out, (n + 2 * GUARD,), np.uint8), hip.shl_mi355x_conv_plan_kernel_name(plan).decode()
    dev.free(d_in), dev.free(d_out), hip.shl_mi355x_conv_plan_destroy(plan)
    return name, whole[GUARD:GUARD + n], int(np.count_nonzero(np.concatenate([whole[:GUARD], whole[GUARD + n:]]) != POISON))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "f16"])
@pytest.mark.parametrize("which", ["5x5_c5_7x7", "5x5_s2_c4_12x9", "batch4_runs_1", "batch4_runs_3"])
def test_conv_forward_writes_the_output_and_nothing_beside_it(standalone, which, dtype):
    hip = standalone[1]
    batch = int(which[-1]) if which.startswith("batch4") else 0
    case = cases.make_case(7699, depthwise=True, layout=NCHW, dtype=dtype, c=5, h=7, w=6, n=4, k=(5, 5), pad=P2) if batch else \
        shape_case([s[0] for s in SHAPES].index(which), dtype)
    (new_name, new, new_guards), (old_name, old, old_guards) = forward(hip, case, batch, "1"), forward(hip, case, batch, "0")
    assert new_name == NAMES[dtype] and "direct" in old_name
    assert (new_guards, old_guards) == (0, 0), "bytes written outside the output"
    assert np.array_equal(new, old)
    if dtype == "int8":
        assert np.array_equal(new, cases.oracle_run(case, "exact").view(np.uint8).reshape(-1)[:new.size])


@pytest.mark.gpu
def test_binary16_specials_propagate_as_in_the_direct_kernel(standalone):
    case = dict(shape_case(0, "f16"))
    x, w = case["input"].copy(), case["kernel"].copy()
    x[0, 0, 0, 0], x[0, 1, 0, 6], x[0, 2, 6, 0], x[0, 3, 6, 6], x[0, 4, 3, 0] = np.inf, -np.inf, np.nan, -0.0, 2.0 ** -24  # corners, a border
    x[0, 0, 6, 3] = -0.0
    w[1, 0, 2, 2] = np.inf
    case["input"], case["kernel"] = x, w
    (new_name, new), (old_name, old) = layer(standalone, case, "1"), layer(standalone, case, "0")
    assert new_name == NAMES["f16"] and "direct" in old_name
    assert np.array_equal(new.view(np.uint16), old.view(np.uint16))

"""A table activation in the DEPTHWISE launch on the GPU (tests/dw_act_cases.py): shl_mi355x_dwconv_lut_forward against
shl_mi355x_conv_forward followed by shl_mi355x_unary_lut_i8 with the same table on one set of device buffers, byte for byte,
and both against the oracle chain (the oracle's depthwise convolution, then the reference's layers on the stored bytes).  The
fused output sits between poisoned guard bands; a refused call leaves it poisoned.  The kernel the library names is asserted:
the dot4 kernel and the generic one here, the matrix-core kernel in a child process under SHL_MI355X_DWMFMA=1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import dw_act_cases as dc
import residual_cases as rc
from cases import pkg

pytestmark = pytest.mark.gpu
CASES = dc.all_cases()
EINVAL, ENOTSUP = -2, -3


@pytest.fixture(scope="module")
def gpu(standalone):
    fe, hip, opt = standalone
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    return hip, opt, cases.HipDevice(hip)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fused_launch_equals_the_two_launches_and_the_oracle_chain(gpu, case):
    hip, opt, dev = gpu
    dc.check_case(hip, opt, dev, case)


def test_refused_calls_leave_the_output_alone(gpu):
    hip, opt, dev = gpu
    c = dc.conv_of("dot4_c32_2x33")
    n = int(np.prod(c["out_shape"]))
    plan = rc.make_plan(hip, c)
    table = np.arange(256, dtype=np.uint8)
    d_in, d_out = dev.alloc(c["input"].nbytes), dev.alloc(n)
    try:
        dev.upload(d_out, np.full(n, dc.POISON, np.uint8))

        def refused(args, code, text):
            assert hip.shl_mi355x_dwconv_lut_forward(*args) == code, text
            assert text.encode() in hip.shl_mi355x_last_error(), hip.shl_mi355x_last_error()
        refused((None, d_in, d_out, 0, table.ctypes.data, None), EINVAL, "NULL")
        refused((plan, d_in, None, 0, table.ctypes.data, None), EINVAL, "NULL")
        refused((plan, None, d_out, 0, table.ctypes.data, None), EINVAL, "NULL")
        refused((plan, d_in, d_out, 0, None, None), EINVAL, "NULL")
        refused((plan, d_out, d_out, 0, table.ctypes.data, None), EINVAL, "overlaps the input")
        refused((plan, d_out + n - 1, d_out, 0, table.ctypes.data, None), EINVAL, "overlaps the input")
        refused((plan, d_in, d_out, 1 << 30, table.ctypes.data, None), EINVAL, "2^31")  # 2^30 images of 66 pixels
        assert hip.shl_mi355x_dwconv_lut_fusable(plan, 1 << 30) == 0 and hip.shl_mi355x_dwconv_lut_kernel_name(plan, 1 << 30) == b""
        assert (dev.download(d_out, (n,), np.uint8) == dc.POISON).all()
    finally:
        for p in (d_in, d_out):
            dev.free(p)
        hip.shl_mi355x_conv_plan_destroy(plan)


def test_plans_outside_the_scope_have_no_fused_launch(gpu):
    """NCHW, binary16, implicit GEMM, a depth multiplier and transposed convolutions: no name, not fusable, and the call is
    ENOTSUP and leaves the output alone"""
    hip, opt, dev = gpu
    import deconv_cases as dcv
    others = [cases.make_case(1, layout=cases.NCHW, c=16, depthwise=True), cases.make_case(2, dtype="f16", c=16, depthwise=True),
              cases.make_case(3, c=16, co=16), cases.make_case(4, c=8, depthwise=True, multiplier=2)]
    plans = [rc.make_plan(hip, c) for c in others]
    dcase = next(c for c in dcv.deconv_cases() if c["name"] == "e_1x1s2_empty_phases_int8_exact_nhwc")
    mult, bias = dcv.tables(dcase)
    dplan = C.c_void_p()
    pkg.check(hip.shl_mi355x_deconv_plan_create(C.byref(dcv.deconv_desc(dcase)), dcase["kernel"].ctypes.data, mult.ctypes.data,
                                                bias.ctypes.data, None, C.byref(dplan)), hip, "deconv_plan_create")
    plans.append(dplan)
    table = np.zeros(256, np.uint8)
    n = 1 << 16
    d_in, d_out = dev.alloc(n), dev.alloc(n)
    try:
        dev.upload(d_out, np.full(n, dc.POISON, np.uint8))
        for plan in plans:
            assert hip.shl_mi355x_dwconv_lut_kernel_name(plan, 0) == b""
            assert hip.shl_mi355x_dwconv_lut_fusable(plan, 0) == 0 and hip.shl_mi355x_dwconv_lut_by_default(plan, 0) == 0
            assert hip.shl_mi355x_dwconv_lut_forward(plan, d_in, d_out, 0, table.ctypes.data, None) == ENOTSUP
            assert b"dwconv_lut_forward: the plan is" in hip.shl_mi355x_last_error()
        assert (dev.download(d_out, (n,), np.uint8) == dc.POISON).all()
    finally:
        for p in (d_in, d_out):
            dev.free(p)
        for plan in plans:
            hip.shl_mi355x_conv_plan_destroy(plan)


def test_the_convolutions_own_entry_points_still_refuse_a_depthwise_plan(gpu):
    hip, opt, dev = gpu
    plan = rc.make_plan(hip, dc.conv_of("dot4_c32_2x33"))
    try:
        assert hip.shl_mi355x_dwconv_lut_fusable(plan, 0) == 1
        assert hip.shl_mi355x_conv_lut_fusable(plan, 0) == 0 and hip.shl_mi355x_conv_lut_kernel_name(plan, 0) == b""
    finally:
        hip.shl_mi355x_conv_plan_destroy(plan)


# (map, C, kernel, stride) -> ((batch, kernel name, fused by default), ...): profiles/dw_act_fuse_notes.md
D4, MF, NH = "dwconv_dot4+lut", "dwconv_mfma+lut", "dwconv_nhwc+lut"
MEASURED = {
    (28, 240, 3, 2): ((1, D4, 1), (32, D4, 1)), (14, 200, 3, 1): ((1, D4, 1), (32, D4, 1)), (14, 184, 3, 1): ((1, D4, 1), (32, D4, 1)),
    (14, 480, 3, 1): ((1, D4, 1), (32, MF, 1)), (14, 672, 3, 1): ((1, D4, 1), (32, MF, 1)), (112, 32, 3, 1): ((1, D4, 1), (32, MF, 1)),
    (56, 144, 3, 1): ((1, D4, 1), (32, D4, 0)),  # 0.83 - 0.84 inside a spread of 13 - 15 %
    (7, 1152, 3, 1): ((1, D4, 1), (32, D4, 1)),
    (14, 672, 5, 2): ((1, NH, 1), (32, NH, 1)), (7, 960, 5, 1): ((1, NH, 1), (32, NH, 1)), (56, 144, 5, 2): ((1, NH, 1), (32, NH, 1)),
    (28, 240, 5, 1): ((1, NH, 1), (32, NH, 0)),  # 0.93 - 0.94 under spreads of 4 - 6 %
    (14, 480, 5, 1): ((1, NH, 1), (32, NH, 1)), (14, 672, 5, 1): ((1, NH, 1), (32, NH, 1)), (7, 1152, 5, 1): ((1, NH, 1), (32, NH, 1)),
}


def test_by_default_only_the_measured_classes_fuse(gpu):
    """csrc/lut_validate.h:dw_lut_default on plans of the measured shapes -- the depthwise layers that carry hswish / swish in
    MobileNetV3-Large and EfficientNet-B0 (tools/dw_act_bench.py)"""
    hip, opt, dev = gpu
    assert len(MEASURED) == 15
    for (hw, c, k, s), answers in MEASURED.items():
        plan = rc.make_plan(hip, cases.make_case(1, h=hw, w=hw, c=c, depthwise=True, k=(k, k), stride=(s, s), pad=(k // 2,) * 4))
        try:
            for batch, name, fused in answers:
                assert hip.shl_mi355x_dwconv_lut_kernel_name(plan, batch) == name.encode(), (hw, c, k, s, batch)
                assert hip.shl_mi355x_dwconv_lut_by_default(plan, batch) == fused, (hw, c, k, s, batch)
        finally:
            hip.shl_mi355x_conv_plan_destroy(plan)


def test_matrix_core_kernel_in_a_child_process():
    """SHL_MI355X_DWMFMA is read once per process: dw_act_cases.py runs its child cases under =1"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SHL_MI355X_")}
    env["SHL_MI355X_DWMFMA"] = "1"
    res = subprocess.run([sys.executable, os.path.join(cases.ROOT, "tests", "dw_act_cases.py")], capture_output=True, text=True,
                         timeout=300, env=env, cwd=cases.ROOT)
    assert res.returncode == 0 and "child ok %d" % len(dc.child_cases()) in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])

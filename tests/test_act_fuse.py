"""A table activation in the convolution's launch on the GPU (tests/act_fuse_cases.py): shl_mi355x_conv_lut_forward against
shl_mi355x_conv_forward followed by shl_mi355x_unary_lut_i8 with the same table on one set of device buffers, byte for byte,
and both against the oracle chain (the oracle's convolution, then the reference's layers on the stored bytes).  The fused
output sits between poisoned guard bands; a refused call leaves it poisoned.  Every case is forced onto its family with
SHL_MI355X_ACT_FORM and the name the library reports is asserted; the large tile flavours and the ones without producer waves
run in child processes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import act_fuse_cases as ac
import cases
import residual_cases as rc
from cases import pkg

pytestmark = pytest.mark.gpu
CASES = ac.all_cases()
EINVAL, ENOTSUP = -2, -3


@pytest.fixture(scope="module")
def gpu(standalone):
    fe, hip, opt = standalone
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    return hip, opt, cases.HipDevice(hip)


def _clean(monkeypatch):
    for var in ("SHL_MI355X_ACT_FORM", "SHL_MI355X_IGEMM"):
        monkeypatch.delenv(var, raising=False)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fused_launch_equals_the_two_launches_and_the_oracle_chain(gpu, case, monkeypatch):
    hip, opt, dev = gpu
    _clean(monkeypatch)
    monkeypatch.setenv("SHL_MI355X_ACT_FORM", case["form"])
    ac.check_case(hip, opt, dev, case, case["form"])


@pytest.mark.parametrize("form", ["wave", "tile"])
def test_either_family_takes_the_other_ones_shape(gpu, form, monkeypatch):
    """the size rule picks one family; forced, the other one computes the same bytes"""
    hip, opt, dev = gpu
    _clean(monkeypatch)
    monkeypatch.setenv("SHL_MI355X_ACT_FORM", form)
    for name in ("wave_1x1_m33_co30_elements-permutation", "wave_1x1_c256_splitk_relu6-permutation", "tile_m129_co144_staged-permutation"):
        ac.check_case(hip, opt, dev, next(c for c in CASES if c["name"] == name), form)


def test_unforced_the_size_rule_names_the_family(gpu, monkeypatch):
    hip, opt, dev = gpu
    _clean(monkeypatch)
    ac.check_case(hip, opt, dev, CASES[0], "wave")  # 33 x 36 outputs: far below one 128 x 128 tile per other CU


def test_no_fused_launch_while_a_family_is_forced_for_the_convolution(gpu, monkeypatch):
    hip, opt, dev = gpu
    _clean(monkeypatch)
    plan = rc.make_plan(hip, ac.conv_of("wave_1x1_m33_co36"))
    table = np.zeros(256, np.uint8)
    try:
        assert hip.shl_mi355x_conv_lut_fusable(plan, 0) == 1
        monkeypatch.setenv("SHL_MI355X_IGEMM", "tile")
        assert hip.shl_mi355x_conv_lut_kernel_name(plan, 0) == b"" and hip.shl_mi355x_conv_lut_fusable(plan, 0) == 0
        assert hip.shl_mi355x_conv_lut_forward(plan, 1 << 40, 1 << 41, 0, table.ctypes.data, None) == ENOTSUP
    finally:
        hip.shl_mi355x_conv_plan_destroy(plan)


def test_refused_calls_leave_the_output_alone(gpu, monkeypatch):
    hip, opt, dev = gpu
    _clean(monkeypatch)
    c = ac.conv_of("wave_1x1_m33_co36")
    n = int(np.prod(c["out_shape"]))
    plan = rc.make_plan(hip, c)
    table = np.arange(256, dtype=np.uint8)
    d_in, d_out = dev.alloc(c["input"].nbytes), dev.alloc(n)
    try:
        dev.upload(d_out, np.full(n, ac.POISON, np.uint8))

        def refused(args, code, text):
            assert hip.shl_mi355x_conv_lut_forward(*args) == code, text
            assert text.encode() in hip.shl_mi355x_last_error(), hip.shl_mi355x_last_error()
        refused((plan, d_in, None, 0, table.ctypes.data, None), EINVAL, "NULL")
        refused((plan, None, d_out, 0, table.ctypes.data, None), EINVAL, "NULL")
        refused((plan, d_in, d_out, 0, None, None), EINVAL, "NULL")
        refused((plan, d_out, d_out, 0, table.ctypes.data, None), EINVAL, "overlaps the input")
        refused((plan, d_out + n - 1, d_out, 0, table.ctypes.data, None), EINVAL, "overlaps the input")
        refused((plan, d_in, d_out, 1 << 30, table.ctypes.data, None), EINVAL, "2^31")
        assert (dev.download(d_out, (n,), np.uint8) == ac.POISON).all()
    finally:
        for p in (d_in, d_out):
            dev.free(p)
        hip.shl_mi355x_conv_plan_destroy(plan)


def test_plans_outside_the_scope_have_no_fused_launch(gpu, monkeypatch):
    """NCHW, binary16, depthwise and transposed convolutions: no name, not fusable, and the call is ENOTSUP"""
    hip, opt, dev = gpu
    _clean(monkeypatch)
    import deconv_cases as dc
    others = [cases.make_case(1, layout=cases.NCHW, c=16, co=16), cases.make_case(2, dtype="f16", c=16, co=16),
              cases.make_case(3, c=16, depthwise=True)]
    plans = [rc.make_plan(hip, c) for c in others]
    dcase = next(c for c in dc.deconv_cases() if c["name"] == "e_1x1s2_empty_phases_int8_exact_nhwc")
    mult, bias = dc.tables(dcase)
    dplan = C.c_void_p()
    pkg.check(hip.shl_mi355x_deconv_plan_create(C.byref(dc.deconv_desc(dcase)), dcase["kernel"].ctypes.data, mult.ctypes.data,
                                                bias.ctypes.data, None, C.byref(dplan)), hip, "deconv_plan_create")
    plans.append(dplan)
    table = np.zeros(256, np.uint8)
    try:
        for plan in plans:
            assert hip.shl_mi355x_conv_lut_kernel_name(plan, 0) == b""
            assert hip.shl_mi355x_conv_lut_fusable(plan, 0) == 0 and hip.shl_mi355x_conv_lut_by_default(plan, 0) == 0
            assert hip.shl_mi355x_conv_lut_forward(plan, 1 << 40, 1 << 41, 0, table.ctypes.data, None) == ENOTSUP
    finally:
        for plan in plans:
            hip.shl_mi355x_conv_plan_destroy(plan)


def test_by_default_only_the_measured_classes_fuse(gpu, monkeypatch):
    """csrc/lut_validate.h:lut_default on plans of the measured shapes (profiles/act_fuse_notes.md)"""
    hip, opt, dev = gpu
    _clean(monkeypatch)
    # (map, C, Co, kernel, stride), then (batch, family, fused by default) per batch
    for (hw, c, co, k, s), answers in (((160, 32, 64, 3, 2), ((1, "wave", 1), (32, "tile", 1))), ((80, 64, 64, 1, 1), ((1, "wave", 1), (32, "tile", 0))),
                                       ((40, 128, 128, 3, 1), ((1, "wave", 1), (32, "tile", 0))), ((20, 512, 512, 1, 1), ((1, "wave", 1), (32, "tile", 1))),
                                       ((112, 16, 96, 1, 1), ((1, "wave", 1), (32, "tile", 1))), ((14, 112, 672, 1, 1), ((1, "wave", 1), (32, "tile", 1))),
                                       ((7, 160, 960, 1, 1), ((1, "wave", 0),)), ((28, 64, 32, 1, 1), ((1, "wave", 0),))):
        plan = rc.make_plan(hip, cases.make_case(1, h=hw, w=hw, c=c, co=co, k=(k, k), stride=(s, s), pad=(k // 2,) * 4))
        try:
            for batch, family, fused in answers:
                assert hip.shl_mi355x_conv_lut_kernel_name(plan, batch) == (family + "+lut").encode(), (hw, c, co, k, batch)
                assert hip.shl_mi355x_conv_lut_by_default(plan, batch) == fused, (hw, c, co, k, batch)
        finally:
            hip.shl_mi355x_conv_plan_destroy(plan)


@pytest.mark.parametrize("extra", ac.CHILD_ENVS, ids=["-".join("%s=%s" % (k[11:], v) for k, v in sorted(e.items())) for e in ac.CHILD_ENVS])
def test_tile_flavours_in_a_child_process(extra):
    """the flavour switches of the tile kernel are read once per process: act_fuse_cases.py runs its child cases under them"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SHL_MI355X_")}
    env.update(extra)
    res = subprocess.run([sys.executable, os.path.join(cases.ROOT, "tests", "act_fuse_cases.py")], capture_output=True, text=True,
                         timeout=300, env=env, cwd=cases.ROOT)
    assert res.returncode == 0 and "child ok" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])

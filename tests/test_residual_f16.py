"""The binary16 fused residual tail on the GPU (tests/residual_f16_cases.py): shl_mi355x_conv_add_f16_forward against the layers
one by one (shl_mi355x_conv_forward, shl_mi355x_add, shl_mi355x_relu_f16) on the same device buffers, compared on bits -- NaNs,
infinities and subnormals included --, the stand-alone convolution against the oracle within the binary16 parity tolerance and
the fused output against the oracle's add and relu of the halves that convolution stored, exactly.  The fused output sits
between poisoned guard bands; a refused call leaves it poisoned.  Every case is forced onto its family with
SHL_MI355X_RESIDUAL_FORM and the name and the flavour the library reports are asserted; the large tile flavours and the ones with
other producer-wave settings run in child processes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import residual_f16_cases as rc
from cases import pkg

pytestmark = pytest.mark.gpu
CASES = rc.all_cases()
EINVAL, ENOTSUP = -2, -3


@pytest.fixture(scope="module")
def gpu(standalone):
    fe, hip, opt = standalone
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    return hip, cases.HipDevice(hip)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fused_launch_equals_the_layers_and_the_oracle_chain(gpu, case, monkeypatch):
    hip, dev = gpu
    monkeypatch.setenv("SHL_MI355X_RESIDUAL_FORM", case["form"])
    rc.check_case(hip, dev, case, case["form"])


@pytest.mark.parametrize("form", ["wave", "tile"])
def test_either_family_takes_the_other_ones_shape(gpu, form, monkeypatch):
    """the size rule picks one family; forced, the other one computes the same bits (shapes whose stand-alone convolution
    does not split K: the wave kernel's one-pass form and the tile kernels add the K steps up in one order)"""
    hip, dev = gpu
    monkeypatch.setenv("SHL_MI355X_RESIDUAL_FORM", form)
    for name in ("wave_1x1_m33_co30_elements", "wave_1x1_m33_co36", "tile_m129_co144_staged", "tile_3x3_m130_co32",
                 "wave_specials_conv_first", "tile_specials_skip_first_relu6"):
        case = next(c for c in CASES if c["name"] == name)
        assert not rc.splits_k(case)
        rc.check_case(hip, dev, case, form)


def test_unforced_the_size_rule_names_the_family(gpu, monkeypatch):
    hip, dev = gpu
    monkeypatch.delenv("SHL_MI355X_RESIDUAL_FORM", raising=False)
    rc.check_case(hip, dev, CASES[0], "wave")  # 33 x 36 outputs: far below one 128 x 128 tile per other CU
    # ... and a grid of 128 x 128 tiles names the tile kernels (host code: nothing is launched)
    plan = rc.make_plan(hip, cases.make_case(1, dtype="f16", h=56, w=56, c=64, co=256, k=(1, 1), pad=(0, 0, 0, 0)))
    try:
        assert hip.shl_mi355x_conv_add_f16_kernel_name(plan, 1) == b"wave+add"
        assert hip.shl_mi355x_conv_add_f16_kernel_name(plan, 128) == b"tile+add"
    finally:
        hip.shl_mi355x_conv_plan_destroy(plan)


def test_refused_calls_leave_the_output_alone(gpu, monkeypatch):
    hip, dev = gpu
    monkeypatch.delenv("SHL_MI355X_RESIDUAL_FORM", raising=False)
    case = CASES[0]
    c = case["conv"]
    n = int(np.prod(c["out_shape"]))
    plan = rc.make_plan(hip, c)
    d_in, d_skip, d_out = dev.alloc(c["input"].nbytes), dev.alloc(2 * n), dev.alloc(2 * n)
    try:
        dev.upload(d_out, np.full(2 * n, rc.POISON, np.uint8))
        good = rc.residual_desc(case)

        def refused(args, code, text):
            assert hip.shl_mi355x_conv_add_f16_forward(*args) == code, text
            assert text.encode() in hip.shl_mi355x_last_error(), hip.shl_mi355x_last_error()
        for act in (-1, 3):
            bad_act = rc.residual_desc(case)
            bad_act.act = act
            refused((plan, d_in, d_skip, d_out, 0, C.byref(bad_act), None), EINVAL, "act")
        refused((plan, d_in, d_skip, None, 0, C.byref(good), None), EINVAL, "NULL")
        refused((plan, d_in, None, d_out, 0, C.byref(good), None), EINVAL, "NULL")
        refused((plan, None, d_skip, d_out, 0, C.byref(good), None), EINVAL, "NULL")
        refused((plan, d_in, d_skip, d_out, 0, None, None), EINVAL, "NULL")
        refused((None, d_in, d_skip, d_out, 0, C.byref(good), None), EINVAL, "NULL")
        refused((plan, d_out, d_skip, d_out, 0, C.byref(good), None), EINVAL, "overlaps the input")
        refused((plan, d_in, d_out + 2 * n - 2, d_out, 0, C.byref(good), None), EINVAL, "overlaps the skip tensor")  # (2-byte elements)
        refused((plan, d_in, d_skip + 1, d_out, 0, C.byref(good), None), EINVAL, "2-byte aligned")
        refused((plan, d_in, d_skip, d_out, 1 << 30, C.byref(good), None), EINVAL, "2^31")
        refused((plan, d_in, d_skip, (1 << 64) - 64, 0, C.byref(good), None), EINVAL, "wraps around")
        assert (dev.download(d_out, (2 * n,), np.uint8) == rc.POISON).all()
    finally:
        for p in (d_in, d_skip, d_out):
            dev.free(p)
        hip.shl_mi355x_conv_plan_destroy(plan)


def test_plans_outside_the_scope_have_no_fused_launch(gpu, monkeypatch):
    """int8, NCHW, depthwise and transposed convolutions: no name, not fusable, and the call is ENOTSUP; the int8 entry points
    say the same of a binary16 plan"""
    hip, dev = gpu
    monkeypatch.delenv("SHL_MI355X_RESIDUAL_FORM", raising=False)
    import deconv_cases as dc
    others = [cases.make_case(1, c=16, co=16), cases.make_case(2, dtype="f16", layout=cases.NCHW, c=16, co=16),
              cases.make_case(3, dtype="f16", c=16, depthwise=True), cases.make_case(4, c=16, depthwise=True)]
    plans = [rc.make_plan(hip, c) for c in others]
    dcase = next(c for c in dc.deconv_cases() if c["name"] == "e_1x1s2_empty_phases_int8_exact_nhwc")
    mult, bias = dc.tables(dcase)
    dplan = C.c_void_p()
    pkg.check(hip.shl_mi355x_deconv_plan_create(C.byref(dc.deconv_desc(dcase)), dcase["kernel"].ctypes.data, mult.ctypes.data,
                                                bias.ctypes.data, None, C.byref(dplan)), hip, "deconv_plan_create")
    plans.append(dplan)
    good = rc.residual_desc(CASES[0])
    far = (1 << 40, 1 << 41, 1 << 42)
    try:
        for plan in plans:
            assert hip.shl_mi355x_conv_add_f16_kernel_name(plan, 0) == b""
            assert hip.shl_mi355x_conv_add_f16_fusable(plan, 0) == 0 and hip.shl_mi355x_conv_add_f16_by_default(plan, 0) == 0
            assert hip.shl_mi355x_conv_add_f16_forward(plan, *far, 0, C.byref(good), None) == ENOTSUP
    finally:
        for plan in plans:
            hip.shl_mi355x_conv_plan_destroy(plan)
    plan = rc.make_plan(hip, CASES[0]["conv"])
    try:
        assert hip.shl_mi355x_conv_add_f16_fusable(plan, 0) == 1 and hip.shl_mi355x_conv_add_fusable(plan, 0) == 0
        assert hip.shl_mi355x_conv_add_kernel_name(plan, 0) == b""
    finally:
        hip.shl_mi355x_conv_plan_destroy(plan)


def test_by_default_only_the_measured_classes_fuse(gpu, monkeypatch):
    """csrc/residual_validate.h:residual_f16_default restated (tests/test_residual_f16_cpu.py checks the restatement against
    the header's own answers) on plans of the measured shapes (profiles/residual_f16_notes.md)"""
    import test_residual_f16_cpu as cpu
    hip, dev = gpu
    monkeypatch.delenv("SHL_MI355X_RESIDUAL_FORM", raising=False)
    for hw, c, co, k in ((14, 256, 1024, 1), (7, 512, 2048, 1), (56, 64, 256, 1), (7, 512, 512, 3), (56, 64, 64, 3), (56, 144, 24, 1),
                         (14, 384, 64, 1), (7, 960, 160, 1)):
        plan = rc.make_plan(hip, cases.make_case(1, dtype="f16", h=hw, w=hw, c=c, co=co, k=(k, k), pad=(k // 2,) * 4))
        try:
            for batch in (1, 32, 128):
                name = hip.shl_mi355x_conv_add_f16_kernel_name(plan, batch).decode()
                assert name in ("wave+add", "tile+add")
                kbytes = (k * k * c * 2 + 63) // 64 * 64
                want = cpu.default_rule(batch * hw * hw, co, kbytes, k * k, name == "tile+add")
                assert hip.shl_mi355x_conv_add_f16_by_default(plan, batch) == int(want), (hw, c, co, k, batch)
        finally:
            hip.shl_mi355x_conv_plan_destroy(plan)


@pytest.mark.parametrize("extra", rc.CHILD_ENVS, ids=["-".join("%s=%s" % (k[11:], v) for k, v in sorted(e.items())) for e in rc.CHILD_ENVS])
def test_tile_flavours_in_a_child_process(extra):
    """the flavour switches of the tile kernel are read once per process: residual_f16_cases.py runs its child cases under them"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SHL_MI355X_")}
    env.update(extra)
    res = subprocess.run([sys.executable, os.path.join(cases.ROOT, "tests", "residual_f16_cases.py")], capture_output=True, text=True,
                         timeout=300, env=env, cwd=cases.ROOT)
    assert res.returncode == 0 and "child ok" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])

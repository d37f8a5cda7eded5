"""The fused residual tail on the GPU (tests/residual_cases.py): shl_mi355x_conv_add_forward against the layers one by one
(shl_mi355x_conv_forward, shl_mi355x_add, shl_mi355x_relu_i8) on the same device buffers, both byte for byte against the oracle
chain (the oracle's convolution, then the reference's add and relu on the stored bytes).  The fused output sits between poisoned
guard bands; a refused call leaves it poisoned.  Every case is forced onto its family with SHL_MI355X_RESIDUAL_FORM and the
name the library reports is asserted; the large tile flavours and the ones without producer waves run in child processes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import residual_cases as rc
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
    """the size rule picks one family; forced, the other one computes the same bytes"""
    hip, dev = gpu
    monkeypatch.setenv("SHL_MI355X_RESIDUAL_FORM", form)
    for name in ("wave_1x1_m33_co30_elements", "wave_1x1_c256_splitk", "tile_m129_co144_staged"):
        rc.check_case(hip, dev, next(c for c in CASES if c["name"] == name), form)


def test_unforced_the_size_rule_names_the_family(gpu, monkeypatch):
    hip, dev = gpu
    monkeypatch.delenv("SHL_MI355X_RESIDUAL_FORM", raising=False)
    rc.check_case(hip, dev, CASES[0], "wave")  # 33 x 36 outputs: far below one 128 x 128 tile per other CU


def test_refused_calls_leave_the_output_alone(gpu, monkeypatch):
    hip, dev = gpu
    monkeypatch.delenv("SHL_MI355X_RESIDUAL_FORM", raising=False)
    case = CASES[0]
    c = case["conv"]
    n = int(np.prod(c["out_shape"]))
    plan = rc.make_plan(hip, c)
    d_in, d_skip, d_out = dev.alloc(c["input"].nbytes), dev.alloc(n), dev.alloc(n)
    try:
        dev.upload(d_out, np.full(n, rc.POISON, np.uint8))
        good = rc.residual_desc(case)

        def refused(args, code, text):
            assert hip.shl_mi355x_conv_add_forward(*args) == code, text
            assert text.encode() in hip.shl_mi355x_last_error(), hip.shl_mi355x_last_error()
        bad_act = rc.residual_desc(case)
        bad_act.act = 3
        bad_scale = rc.residual_desc(case)
        bad_scale.sum_scale = float("nan")
        neg_scale = rc.residual_desc(case)
        neg_scale.skip_scale = -1.0
        refused((plan, d_in, d_skip, d_out, 0, C.byref(bad_act), None), EINVAL, "act")
        refused((plan, d_in, d_skip, d_out, 0, C.byref(bad_scale), None), EINVAL, "scale")
        refused((plan, d_in, d_skip, d_out, 0, C.byref(neg_scale), None), EINVAL, "scale")
        refused((plan, d_in, d_skip, None, 0, C.byref(good), None), EINVAL, "NULL")
        refused((plan, d_in, None, d_out, 0, C.byref(good), None), EINVAL, "NULL")
        refused((plan, d_in, d_skip, d_out, 0, None, None), EINVAL, "NULL")
        refused((plan, d_out, d_skip, d_out, 0, C.byref(good), None), EINVAL, "overlaps the input")
        refused((plan, d_in, d_out + 4, d_out, 0, C.byref(good), None), EINVAL, "overlaps the skip tensor")
        refused((plan, d_in, d_skip, d_out, 1 << 30, C.byref(good), None), EINVAL, "2^31")
        assert (dev.download(d_out, (n,), np.uint8) == rc.POISON).all()
    finally:
        for p in (d_in, d_skip, d_out):
            dev.free(p)
        hip.shl_mi355x_conv_plan_destroy(plan)


def test_plans_outside_the_scope_have_no_fused_launch(gpu, monkeypatch):
    """NCHW, binary16, depthwise and transposed convolutions: no name, not fusable, and the call is ENOTSUP"""
    hip, dev = gpu
    monkeypatch.delenv("SHL_MI355X_RESIDUAL_FORM", raising=False)
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
    good = rc.residual_desc(CASES[0])
    far = (1 << 40, 1 << 41, 1 << 42)
    try:
        for plan in plans:
            assert hip.shl_mi355x_conv_add_kernel_name(plan, 0) == b""
            assert hip.shl_mi355x_conv_add_fusable(plan, 0) == 0 and hip.shl_mi355x_conv_add_by_default(plan, 0) == 0
            assert hip.shl_mi355x_conv_add_forward(plan, *far, 0, C.byref(good), None) == ENOTSUP
    finally:
        for plan in plans:
            hip.shl_mi355x_conv_plan_destroy(plan)


def test_by_default_only_the_measured_classes_fuse(gpu, monkeypatch):
    """csrc/residual_validate.h:residual_default restated on plans of the measured shapes (profiles/residual_notes.md)"""
    hip, dev = gpu
    monkeypatch.delenv("SHL_MI355X_RESIDUAL_FORM", raising=False)
    # (map, C, Co, kernel), then (batch, family, fused by default) per batch
    for (hw, c, co, k), answers in (((14, 256, 1024, 1), ((1, "wave", 1), (128, "tile", 1))),
                                    ((7, 512, 2048, 1), ((1, "wave", 1), (128, "tile", 0))),
                                    ((56, 64, 256, 1), ((1, "wave", 1), (128, "tile", 1))),
                                    ((7, 512, 512, 3), ((1, "wave", 1), (128, "tile", 0))),
                                    ((56, 144, 24, 1), ((1, "wave", 0),)), ((28, 192, 32, 1), ((1, "wave", 0),)),
                                    ((14, 384, 64, 1), ((1, "wave", 1),)), ((7, 960, 160, 1), ((1, "wave", 1),))):
        plan = rc.make_plan(hip, cases.make_case(1, h=hw, w=hw, c=c, co=co, k=(k, k), pad=(k // 2,) * 4))
        try:
            for batch, family, fused in answers:
                assert hip.shl_mi355x_conv_add_kernel_name(plan, batch) == (family + "+add").encode(), (hw, c, co, k, batch)
                assert hip.shl_mi355x_conv_add_by_default(plan, batch) == fused, (hw, c, co, k, batch)
        finally:
            hip.shl_mi355x_conv_plan_destroy(plan)


@pytest.mark.parametrize("extra", rc.CHILD_ENVS, ids=["-".join("%s=%s" % (k[11:], v) for k, v in sorted(e.items())) for e in rc.CHILD_ENVS])
def test_tile_flavours_in_a_child_process(extra):
    """the flavour switches of the tile kernel are read once per process: residual_cases.py runs its child cases under them"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SHL_MI355X_")}
    env.update(extra)
    res = subprocess.run([sys.executable, os.path.join(cases.ROOT, "tests", "residual_cases.py")], capture_output=True, text=True,
                         timeout=300, env=env, cwd=cases.ROOT)
    assert res.returncode == 0 and "child ok" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])

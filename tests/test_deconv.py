"""Transposed convolution on the GPU (-m gpu): every case of deconv_cases.deconv_cases(), each kernel form it is eligible for
forced by SHL_MI355X_DECONV_FORM, through the C ABI (plan + forward, guard bands around the output), through csinn_deconv2d
on host tensors (the staging path) and on DMABUF tensors, against the numpy restatement that tests/test_deconv_cpu.py ties to
the genuine library: int8 bit for bit in both regimes, binary16 with exact sums bit for bit in either form, the one
normally distributed binary16 case within the project's 1e-3 relative."""
import numpy as np
import pytest

import cases
import deconv_cases as dc
from cases import pkg

CASES = dc.deconv_cases()
RUNS = [(c, f) for c in CASES for f in dc.forms_of(c)]
RUN_IDS = ["%s-%s" % (c["name"], f) for c, f in RUNS]
NORMAL = "g_4x4s2p1_deep_f16_normal_nhwc"
NAMES = {("int8", dc.PHASE): "deconv_phase_i8_mfma32x32x32", ("f16", dc.PHASE): "deconv_phase_f16_mfma32x32x16",
         ("int8", dc.GATHER): "deconv_gather_i8", ("f16", dc.GATHER): "deconv_gather_f16"}
ALGOS = {dc.GATHER: pkg.ALGO_DECONV_GATHER, dc.PHASE: pkg.ALGO_DECONV_PHASE}


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt, cases.HipDevice(hip)


@pytest.fixture(scope="module")
def want():
    """the restatement's answers, computed once per case"""
    memo = {}

    def get(case):
        if case["name"] not in memo:
            memo[case["name"]] = dc.deconv_scatter(case)
            memo[case["name"]].setflags(write=False)
        return memo[case["name"]]
    return get


def check(got, case, want, route):
    if case["name"] == NORMAL:
        assert dc.matches(got, want(case), "f16"), "%s, %s: beyond 1e-3 of the restatement" % (case["name"], route)
    else:
        dc.assert_same(got, want(case), "%s, %s vs the restatement" % (case["name"], route))


@pytest.mark.gpu
@pytest.mark.parametrize("case,form", RUNS, ids=RUN_IDS)
def test_deconv_matches_the_restatement_through_every_route(gpu, want, case, form, monkeypatch):
    fe, hip, opt, dev = gpu
    monkeypatch.setenv("SHL_MI355X_DECONV_FORM", form)  # read per plan
    got, name, algo = dc.cabi_run(hip, dev, case)
    assert name == NAMES[case["dtype"], form] and algo == ALGOS[form]
    check(got, case, want, "C ABI, " + form)
    if case["n"] > 1:  # a second forward with the batch overridden to 1 on the same kind of plan
        got1, _, _ = dc.cabi_run(hip, dev, case, batch=1)
        one = lambda c: np.ascontiguousarray(want(c)[:1])
        check(got1, case, one, "C ABI, %s, batch overridden to 1" % form)
    if case["act"]:
        return  # the operator API has no fused deconvolution op: the fold is the session's (tests/test_deconv_session.py)
    kept = []
    check(dc.csinn_run(fe, pkg.API_MI355X, case, keep_params=kept), case, want, "csinn on host tensors, " + form)
    assert opt.shl_mi355x_params_kernel_name(kept[0][0]).decode() == NAMES[case["dtype"], form]
    check(dc.csinn_run(fe, pkg.API_MI355X, case, device=dev), case, want, "csinn on DMABUF tensors, " + form)


@pytest.mark.gpu
def test_fusion_queries_answer_no_for_a_deconvolution_plan(gpu, monkeypatch):
    import ctypes as C
    fe, hip, opt, dev = gpu
    monkeypatch.delenv("SHL_MI355X_DECONV_FORM", raising=False)
    case = next(c for c in CASES if c["name"] == "e_1x1s2_empty_phases_int8_exact_nhwc")
    mult, bias = dc.tables(case)
    plan = C.c_void_p()
    pkg.check(hip.shl_mi355x_deconv_plan_create(C.byref(dc.deconv_desc(case)), case["kernel"].ctypes.data, mult.ctypes.data, bias.ctypes.data,
                                                None, C.byref(plan)), hip, "deconv_plan_create")
    assert hip.shl_mi355x_pool_conv_fusable(plan, 1, 1) == 0 and hip.shl_mi355x_conv_pool_fusable(plan, 1) == 0
    assert hip.shl_mi355x_pwdw_fusable(plan, plan, 1) == 0 and hip.shl_mi355x_pwdw_form(plan, plan, 1) == 0
    assert hip.shl_mi355x_conv_plan_bytes(plan) > 0 and hip.shl_mi355x_conv_plan_adopt_block(plan, None) == 0
    hip.shl_mi355x_conv_plan_destroy(plan)

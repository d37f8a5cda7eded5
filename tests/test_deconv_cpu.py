"""Transposed convolution, the part that needs no GPU: the numpy restatement of the contract (deconv_cases.deconv_scatter)
against the genuine library's golden outputs and, where it is built, the live library; the phase decomposition against the
scatter and against shl_mi355x_deconv_geometry over a sweep of kernels, strides and pads; the form rule and its switch; the
refusals of the C ABI and of the backend; the op ids and the params block; the exported symbols; shape inference; the
decoder's oracle chain against the genuine graph executor."""
import ctypes as C
import importlib.util
import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import deconv_cases as dc
from cases import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = dc.deconv_cases()
IDS = [c["name"] for c in CASES]
BY = {c["name"]: c for c in CASES}
GOLD = dc.golden()
EINVAL, ENOTSUP = -2, -3
NAMES = {("int8", dc.PHASE): "deconv_phase_i8_mfma32x32x32", ("f16", dc.PHASE): "deconv_phase_f16_mfma32x32x16",
         ("int8", dc.GATHER): "deconv_gather_i8", ("f16", dc.GATHER): "deconv_gather_f16"}
NORMAL = "g_4x4s2p1_deep_f16_normal_nhwc"


def test_golden_covers_the_case_list():
    assert sorted(GOLD) == sorted(IDS) and len(set(IDS)) == len(IDS)
    assert os.path.getsize(os.path.join(HERE, "golden", "deconv_cases.npz")) <= 305686  # no larger than the resize one


def test_case_list_covers_what_it_must():
    def has(**kw):
        return [c for c in CASES if all(c[k] == v for k, v in kw.items())]
    for dtype in ("int8", "f16"):
        for regime in (("exact", "general") if dtype == "int8" else ("exact",)):
            for kw in list(dc.SHAPES.values()) + list(dc.GATHER_ONLY.values()):
                assert has(dtype=dtype, regime=regime, layout="NHWC", dw=False, h=kw["h"], w=kw["w"], c=kw["c"], co=kw["co"]), (dtype, regime, kw)
            for layout in ("NHWC", "NCHW"):  # every weight layout: group 1 and depthwise in both
                assert has(dtype=dtype, regime=regime, layout=layout, dw=True, c=19) and has(dtype=dtype, regime=regime, layout=layout, dw=True, c=64)
                assert has(dtype=dtype, regime=regime, layout=layout, dw=False)
            assert has(dtype=dtype, regime=regime, act=1) and has(dtype=dtype, regime=regime, act=2) and has(dtype=dtype, regime=regime, has_bias=False)
        assert {f for c in has(dtype=dtype) for f in dc.forms_of(c)} == {dc.PHASE, dc.GATHER}
    assert {c["in_q"][1] for c in has(dtype="int8")} >= {-128, 127}
    assert has(dtype="int8", per_channel=True, dw=False, layout="NHWC") and has(dtype="int8", per_channel=True, dw=True, layout="NCHW")
    assert not has(per_channel=True, dw=False, layout="NCHW")  # refused: the records run along the input channel
    a = BY["a_unet_2x2s2_int8_exact_nhwc"]
    assert a["n"] * a["h"] * a["w"] == 70  # pixels of each of its four phases: a ragged tile
    rows, _, _ = dc.phase_table(BY["c_3x3s2p1_outpad_int8_exact_nhwc"])
    assert sorted(r[2] * r[3] for r in rows) == [1, 2, 2, 4]
    rows, _, _ = dc.phase_table(BY["e_1x1s2_empty_phases_int8_exact_nhwc"])
    assert sorted(r[2] * r[3] for r in rows) == [0, 0, 0, 1]
    for c in has(dtype="f16"):  # multiples of 2^-4 in [-2, 2], the one normally distributed case apart
        if c["name"] != NORMAL:
            for key in ("x", "kernel", "bias"):
                v = c[key].astype(np.float64) * 16
                assert np.all(v == np.rint(v)) and np.abs(v).max() <= 32, (c["name"], key)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scatter_restatement_against_the_golden_file(case):
    """exact regime: bit for bit.  general regime: DESIGN 2's gate -- |delta| <= 1 LSB on at most max(2, 2e-4 n) outputs"""
    got, want = dc.bits(dc.deconv_scatter(case)), GOLD[case["name"]]
    assert got.shape == want.shape
    if case["regime"] == "exact":
        dc.assert_same(got, want, case["name"] + " vs golden")
    else:
        delta = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert delta.max() <= 1 and int((delta != 0).sum()) <= max(2, int(2e-4 * got.size)), (case["name"], int(delta.max()), int((delta != 0).sum()))


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_live_reference_equals_the_golden_file():
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)
    for case in CASES:
        dc.assert_same(dc.reference_run(fe, case), GOLD[case["name"]], case["name"] + ": live reference vs golden")


@pytest.mark.parametrize("case", [c for c in CASES if not c["dw"]], ids=[c["name"] for c in CASES if not c["dw"]])
def test_phase_restatement_equals_the_scatter(case):
    """pad-page taps and the acc_init fold cancel: (zp - zp) w = 0.  binary16 with exact sums: bit for bit in any order"""
    got, want = dc.deconv_phase(case), dc.deconv_scatter(case)
    if case["name"] == NORMAL:
        assert dc.matches(got, want, "f16"), "phase order and the reference's order differ by more than 1e-3 on the test's own inputs"
    else:
        dc.assert_same(got, want, case["name"] + ": phase vs scatter")


def _sweep():
    """every kernel 1..5 x stride 1..3 pair with seeded pads 0..2, maps up to 6 x 6 and an output_padding below the stride
    (drawn again while the output would be empty)"""
    rng = np.random.default_rng(20261019)
    for kh, kw, sh, sw in itertools.product(range(1, 6), range(1, 6), range(1, 4), range(1, 4)):
        while True:
            pt, pl, pd, pr = (int(v) for v in rng.integers(0, 3, 4))
            h, w = int(rng.integers(1, 7)), int(rng.integers(1, 7))
            op = (int(rng.integers(0, sh)), int(rng.integers(0, sw)))
            if dc.out_extent(h, kh, sh, pt, pd, op[0]) >= 1 and dc.out_extent(w, kw, sw, pl, pr, op[1]) >= 1:
                break
        yield dict(h=h, w=w, k=(kh, kw), stride=(sh, sw), pad=(pt, pl, pd, pr), out_pad=op, n=int(rng.integers(1, 3)))


def test_phase_restatement_equals_the_scatter_on_a_seeded_sweep():
    """kernel 1..5 x stride 1..3 x pad 0..2 on maps up to 6 x 6, int8 with both extreme zero points"""
    n = 0
    for i, kw in enumerate(_sweep()):
        case = dc.make("sweep_%d" % i, c=4, co=3, in_zp=(-128, 127)[i & 1], regime=("exact", "general")[(i >> 1) & 1], **kw)
        assert np.array_equal(dc.phase_sums(case), dc.scatter_sums(case)), kw
        n += 1
    assert n == 225


def test_geometry_equals_the_numpy_phase_table(built):
    hip = pkg.load_hip()
    buf = (C.c_int32 * 64)()
    for i, kw in enumerate(_sweep()):
        case = dc.make("sweep_%d" % i, c=32, co=(24, 70)[i & 1], **kw)
        assert hip.shl_mi355x_deconv_geometry(C.byref(dc.deconv_desc(case)), buf, 64) == 0, hip.shl_mi355x_last_error()
        rows, tiles, wgs = dc.phase_table(case)
        want = [1, len(rows)] + [v for r in rows for v in r] + [tiles, wgs]
        assert list(buf[:len(want)]) == want, (kw, list(buf[:len(want)]), want)
    case = BY["a_unet_2x2s2_int8_exact_nhwc"]
    assert hip.shl_mi355x_deconv_geometry(C.byref(dc.deconv_desc(case)), buf, 27) == EINVAL  # 4 + 6 * 4 values are needed
    assert hip.shl_mi355x_deconv_geometry(C.byref(dc.deconv_desc(case)), buf, 28) == 0
    assert list(buf[:2]) == [1, 4] and buf[26] == 4 * 3 and buf[27] == 4  # 70 pixels: three tiles per phase, one workgroup each


def test_form_rule_and_the_forced_switch(built, monkeypatch):
    hip = pkg.load_hip()
    name = lambda c: hip.shl_mi355x_deconv_kernel_name(C.byref(dc.deconv_desc(c))).decode()
    monkeypatch.delenv("SHL_MI355X_DECONV_FORM", raising=False)
    seen = set()
    for c in CASES:  # eligible -> phase
        form = dc.PHASE if dc.phase_eligible(c) else dc.GATHER
        assert name(c) == NAMES[c["dtype"], form], c["name"]
        seen.add((c["dtype"], form, c["layout"], c["dw"]))
    assert seen == {(d, dc.PHASE, "NHWC", False) for d in ("int8", "f16")} | \
        {(d, dc.GATHER, l, w) for d in ("int8", "f16") for l in ("NHWC", "NCHW") for w in (False, True)}
    monkeypatch.setenv("SHL_MI355X_DECONV_FORM", "gather")
    assert all(name(c) == NAMES[c["dtype"], dc.GATHER] for c in CASES)
    monkeypatch.setenv("SHL_MI355X_DECONV_FORM", "phase")
    buf = (C.c_int32 * 64)()
    for c in CASES:  # a forced phase form on a layer it does not take is refused, not silently replaced
        if dc.phase_eligible(c):
            assert name(c) == NAMES[c["dtype"], dc.PHASE]
        else:
            assert name(c) == ""
            assert hip.shl_mi355x_deconv_geometry(C.byref(dc.deconv_desc(c)), buf, 64) == ENOTSUP
            plan = C.c_void_p()
            mult, bias = dc.tables(c)
            assert hip.shl_mi355x_deconv_plan_create(C.byref(dc.deconv_desc(c)), c["kernel"].ctypes.data, mult.ctypes.data, bias.ctypes.data,
                                                     None, C.byref(plan)) == ENOTSUP and not plan.value
            assert b"SHL_MI355X_DECONV_FORM=phase" in hip.shl_mi355x_last_error()
    monkeypatch.setenv("SHL_MI355X_DECONV_FORM", "anything else")
    assert name(BY["a_unet_2x2s2_int8_exact_nhwc"]) == NAMES["int8", dc.PHASE]


def test_plan_refusals_happen_before_any_device_call(built, monkeypatch):
    """EINVAL / ENOTSUP with a last_error text, on a machine that may have no device at all"""
    monkeypatch.delenv("SHL_MI355X_DECONV_FORM", raising=False)
    hip = pkg.load_hip()
    case = BY["b_4x4s2p1_int8_exact_nhwc"]
    mult, bias = dc.tables(case)

    def create(**override):
        plan = C.c_void_p()
        d = dc.deconv_desc(case, **override)
        rc = hip.shl_mi355x_deconv_plan_create(C.byref(d), case["kernel"].ctypes.data, mult.ctypes.data, bias.ctypes.data, None, C.byref(plan))
        assert not plan.value and hip.shl_mi355x_deconv_kernel_name(C.byref(d)) == b""
        return rc, hip.shl_mi355x_last_error()
    for override, status, text in ((dict(dilation_h=2), ENOTSUP, b"dilat"), (dict(dilation_w=3), ENOTSUP, b"dilat"),
                                   (dict(group=2), ENOTSUP, b"group"), (dict(group=24), ENOTSUP, b"group"),
                                   (dict(in_h=0), EINVAL, b"extent"), (dict(out_w=-1), EINVAL, b"extent"), (dict(out_c=0), EINVAL, b"extent"),
                                   (dict(kernel_h=0), EINVAL, b"kernel"), (dict(stride_w=0), EINVAL, b"stride"),
                                   (dict(out_h=(6 - 1) * 2 + 4 + 2 + 1), EINVAL, b"larger"), (dict(out_w=(5 - 1) * 2 + 4 + 2 + 1), EINVAL, b"larger"),
                                   (dict(layout=2), EINVAL, b"layout"), (dict(dtype=2), EINVAL, b"dtype"), (dict(out_scale=0.0), EINVAL, b"scale")):
        rc, msg = create(**override)
        assert rc == status and text in msg, (override, rc, msg)
    # the largest output the guard admits is a descriptor like any other
    d = dc.deconv_desc(case, out_h=(6 - 1) * 2 + 4 + 2)
    assert hip.shl_mi355x_deconv_kernel_name(C.byref(d)) == NAMES["int8", dc.PHASE].encode()
    assert hip.shl_mi355x_deconv_plan_create(None, None, None, None, None, None) == EINVAL
    dwc = BY["j_dw19_4x4_int8_exact_nhwc"]
    assert hip.shl_mi355x_deconv_kernel_name(C.byref(dc.deconv_desc(dwc, out_c=38))) == b""  # depthwise: out_c == in_c


REFUSALS = [
    ("group_deconv2d", "a_unet_2x2s2_int8_exact_nhwc", dict(group=32, _c=64), "group_deconv2d"),
    ("kernel zero point", "a_unet_2x2s2_int8_exact_nhwc", dict(k_zps=(3,)), "kernel zero point"),
    ("per-channel kernel records, NCHW group 1", "k_a_unet_2x2s2_int8_exact_nchw", dict(k_scales=tuple([2.0 ** -7] * 32)), "INPUT channel"),
    ("per-channel activations", "a_unet_2x2s2_int8_exact_nhwc", dict(in_scales=tuple([2.0 ** -4] * 32)), "per-channel quantised activations"),
    ("binary16 input scale", "a_unet_2x2s2_f16_exact_nhwc", dict(in_scales=(0.5,)), "scale != 1"),
    ("binary16 kernel scale", "a_unet_2x2s2_f16_exact_nhwc", dict(k_scales=(0.5,)), "scale != 1"),
    ("binary16 bias scale", "a_unet_2x2s2_f16_exact_nhwc", dict(b_scales=(0.5,)), "scale != 1"),
    ("float32 tensors", "a_unet_2x2s2_int8_exact_nhwc", dict(dtype=pkg.DTYPE_FLOAT32), None),
    ("kernel not host resident", "a_unet_2x2s2_int8_exact_nhwc", dict(kernel_dmabuf=True), "host resident"),
    ("dilation", "a_unet_2x2s2_int8_exact_nhwc", dict(dilation=(2, 2)), "dilat"),
]


@pytest.mark.parametrize("what,name,override,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_backend_refusals_through_the_standalone_front_end(standalone, capfd, what, name, override, text):
    """csinn_deconv2d_init drops the init callback's status, as the reference's does: the refusal is the error message at init
    and a csinn_deconv2d that fails.  Without libshl next to it there is nothing to fall through to."""
    fe, hip, opt = standalone
    case = dict(BY[name])
    override = dict(override)
    if "_c" in override:  # a grouped deconvolution: group == Cout != Cin
        c = override.pop("_c")
        case.update(c=c, in_shape=(2, 5, 7, c), x=np.zeros((2, 5, 7, c), np.int8))
    capfd.readouterr()
    before = opt.shl_mi355x_plans_created()
    rc_init, rc = dc.csinn_run(fe, pkg.API_MI355X, case, status=True, **override)
    err = capfd.readouterr().err
    assert rc_init == pkg.CSINN_TRUE and rc != pkg.CSINN_TRUE, what
    assert opt.shl_mi355x_plans_created() == before, "a plan was made for a refused layer"
    if text is None:  # no callback is registered for the dtype at all
        assert "no callback" in err or "mi355x" in err, err
    else:
        assert text in err, (what, err)


def test_front_end_picks_the_op_as_the_reference_does(standalone):
    fe, hip, opt = standalone
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, pkg.API_MI355X, keep)
    case = BY["a_unet_2x2s2_int8_exact_nhwc"]
    tensors, _, _ = dc.csinn_tensors(fe, keep, sess, case)
    p = pkg.deconv_params(fe, keep, pkg.API_MI355X, pkg.LAYOUT_NHWC, group=5, sess=sess)  # neither 1, Cin nor Cout
    assert fe.csinn_deconv2d_init(*tensors, p) != pkg.CSINN_TRUE


def test_op_ids_and_params_block_match_the_reference():
    want = json.load(open(os.path.join(HERE, "golden", "deconv_op_ids.json")))
    assert want == {"CSINN_OP_DECONV2D": 54, "CSINN_OP_DEPTHWISE_DECONV2D": 55, "CSINN_OP_GROUP_DECONV2D": 56, "CSINN_LAYOUT_IOHW": 31,
                    "sizeof csinn_conv2d_params": 104, "offsetof csinn_conv2d_params.group": 40,
                    "offsetof csinn_conv2d_params.out_pad_height": 76, "offsetof csinn_conv2d_params.conv_extra": 88}
    spec = importlib.util.spec_from_file_location("make_deconv_golden", os.path.join(HERE, "golden", "make_deconv_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    inc = os.path.join(cases.ROOT, "include")
    assert mod.measure([inc, os.path.join(inc, "csinn")]) == want  # this repository's own headers
    text = open(os.path.join(inc, "csinn", "csinn_data_structure.h")).read()
    for key in ("CSINN_OP_DECONV2D", "CSINN_OP_DEPTHWISE_DECONV2D", "CSINN_OP_GROUP_DECONV2D", "CSINN_LAYOUT_IOHW"):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % key, text).group(1)) == want[key]
    assert (pkg.OP_DECONV2D, pkg.OP_DEPTHWISE_DECONV2D, pkg.OP_GROUP_DECONV2D, pkg.LAYOUT_IOHW) == (54, 55, 56, 31)
    assert C.sizeof(pkg.Conv2dParams) == 104 and pkg.Conv2dParams.out_pad_height.offset == 76
    assert (pkg.ALGO_DECONV_GATHER, pkg.ALGO_DECONV_PHASE) == (8, 9)
    header = open(os.path.join(inc, "shl_mi355x.h")).read()
    assert re.search(r"SHL_MI355X_ALGO_DECONV_GATHER = 8,.*\n\s*SHL_MI355X_ALGO_DECONV_PHASE = 9\s", header)
    assert "#define SHL_MI355X_ABI_VERSION 1" in header


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_libraries_export_the_new_entry_points(built):
    assert {"csinn_deconv2d_init", "csinn_deconv2d", "shl_gref_deconv2d", "shl_gref_depthwise_deconv2d", "shl_gref_group_deconv2d",
            "shl_gref_deconv2d_infer_shape"} <= _exports(pkg.lib_path("libcsinn_nn2.so"))
    assert {"shl_mi355x_deconv2d_init", "shl_mi355x_deconv2d_exec", "shl_mi355x_deconv2d_perf", "shl_mi355x_deconv2d_fold_activation"} <= \
        _exports(pkg.lib_path("libshl_mi355x_opt.so"))
    assert {"shl_mi355x_deconv_plan_create", "shl_mi355x_deconv_geometry", "shl_mi355x_deconv_kernel_name"} <= \
        _exports(pkg.lib_path("libshl_mi355x.so"))


def test_graph_executor_infers_the_formula(standalone):
    fe, hip, opt = standalone
    tp = C.POINTER(pkg.Tensor)
    fe.shl_gref_deconv2d_infer_shape.restype = C.c_int
    fe.shl_gref_deconv2d_infer_shape.argtypes = [tp, tp, tp, tp, C.c_void_p]
    for name in ("b_4x4s2p1_int8_exact_nhwc", "f_2x3_s21_p01_int8_exact_nhwc", "k_a_unet_2x2s2_int8_exact_nchw", "j_dw19_4x4_int8_exact_nchw",
                 "j_dw19_4x4_int8_exact_nhwc", "h_2x2_s32_f16_exact_nhwc"):
        case = BY[name]
        keep = pkg.Keep()
        sess = pkg.layer_session(fe, pkg.API_MI355X, keep)
        tensors, _, _ = dc.csinn_tensors(fe, keep, sess, case)
        for i in range(4):
            tensors[1].contents.dim[i] = 0
        nhwc = case["layout"] == "NHWC"
        p = pkg.deconv_params(fe, keep, pkg.API_MI355X, pkg.LAYOUT_NHWC if nhwc else pkg.LAYOUT_NCHW, case["stride"], case["pad"], (0, 0),
                              case["group"], (1, 1), sess)
        assert fe.shl_gref_deconv2d_infer_shape(*tensors, p) == pkg.CSINN_TRUE
        assert tuple(tensors[1].contents.dim[:4]) == tuple(case["out_shape"]) and tensors[1].contents.dim_count == 4, name


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
@pytest.mark.parametrize("dtype,layout", [("int8", "NHWC"), ("f16", "NCHW")])
def test_decoder_oracle_chain_equals_the_genuine_graph_executor(dtype, layout):
    """the yardstick of tests/test_deconv_session.py: DecoderNet through the genuine front-end, graph executor and C kernels"""
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)
    net = dc.DecoderNet(dtype, layout)
    net.build(fe, pkg.API_REF)
    for k in (0, 1):
        x = net.input(k)
        got, want = net.run(fe, x), net.oracle(x)
        if dtype == "int8":
            dc.assert_same(got, want, "DecoderNet %s %s input %d" % (dtype, layout, k))
        else:  # the C oracle's binary16 convolutions sum in another order than the library's NCHW path
            assert dc.matches(got, want, dtype), "DecoderNet %s %s input %d" % (dtype, layout, k)
    assert not np.array_equal(net.oracle(net.input(0)), net.oracle(net.input(1))), "the two inputs must tell runs apart"
    net.close(fe)

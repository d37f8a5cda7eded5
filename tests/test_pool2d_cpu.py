"""Windowed max / average pooling, the part that needs no GPU: the numpy restatement of the reference
(pool_cases.pool_numpy) against the genuine library's golden outputs and, where it is built, the live library;
the op ids; the exported symbols; the kernel-form rules."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import pool_cases
from cases import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = pool_cases.pool_cases()
IDS = [c["name"] for c in CASES]
GOLD = pool_cases.golden()


def test_golden_covers_the_case_list():
    assert sorted(GOLD) == sorted(IDS)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_numpy_restatement_matches_the_reference_golden(case):
    pool_cases.assert_same(pool_cases.pool_numpy(case), GOLD[case["name"]], case["name"] + " vs golden")


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_numpy_restatement_matches_the_live_reference():
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)  # errors only: the library warns about every binary16 saturation
    for case in CASES:
        got = pool_cases.pool_run(fe, pkg.API_REF, case)
        pool_cases.assert_same(pool_cases.pool_numpy(case), got, case["name"] + " vs live reference")
        pool_cases.assert_same(got, GOLD[case["name"]], case["name"] + ": live reference vs golden")


def test_op_ids_match_the_reference():
    want = json.load(open(os.path.join(HERE, "golden", "pool_op_ids.json")))
    assert want == {"CSINN_OP_AVGPOOL2D": 14, "CSINN_OP_MAXPOOL2D": 98}
    text = open(os.path.join(cases.ROOT, "include", "csinn", "csinn_data_structure.h")).read()
    got = {name: int(val) for name, val in re.findall(r"\b(CSINN_OP_(?:AVG|MAX)POOL2D)\s*=\s*(\d+)", text)}
    assert got == want
    assert (pkg.OP_AVGPOOL2D, pkg.OP_MAXPOOL2D) == (14, 98)
    assert int(re.search(r"\bCSINN_OP_SIZE\s*=\s*(\d+)", text).group(1)) == 194
    import ctypes as C
    assert C.sizeof(pkg.PoolParams) == 104


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_libraries_export_the_pool_entry_points(built):
    nn2 = _exports(pkg.lib_path("libcsinn_nn2.so"))
    assert {"csinn_maxpool2d_init", "csinn_maxpool2d", "csinn_avgpool2d_init", "csinn_avgpool2d",
            "shl_gref_maxpool2d", "shl_gref_avgpool2d"} <= nn2
    assert {"shl_mi355x_maxpool2d_exec", "shl_mi355x_avgpool2d_exec"} <= _exports(pkg.lib_path("libshl_mi355x_opt.so"))
    assert {"shl_mi355x_pool2d", "shl_mi355x_pool2d_kernel_name"} <= _exports(pkg.lib_path("libshl_mi355x.so"))
    import ctypes as C
    assert C.sizeof(pkg.PoolDesc) == 24 * 4 and pkg.PoolDesc.in_scale.offset == 18 * 4


def _name(hip, **kw):
    case = dict(kind="max", dtype="int8", layout="NHWC", n=1, c=16, h=8, w=8, ho=4, wo=4, kernel=(3, 3), stride=(2, 2),
                pad=(1, 1, 1, 1), cip=0, in_q=(0.0625, -5), out_q=(0.0625, -5))
    case.update(kw)
    import ctypes as C
    return hip.shl_mi355x_pool2d_kernel_name(C.byref(pool_cases.pool_desc(case))).decode()


def test_kernel_form_rules(built, monkeypatch):
    """pure host code: no device is initialised"""
    monkeypatch.delenv("SHL_MI355X_POOL_FORM", raising=False)
    hip = pkg.load_hip()
    vec, row, gen = "pool2d_nhwc_vec", "pool2d_nchw_row", "pool2d_generic"
    assert _name(hip, c=16) == vec and _name(hip, c=48, kind="avg") == vec
    assert _name(hip, c=20) == gen and _name(hip, c=3) == gen and _name(hip, c=8) == gen
    assert _name(hip, dtype="f16", c=8) == vec and _name(hip, dtype="f16", c=24) == vec and _name(hip, dtype="f16", c=12) == gen
    for c in (1, 3, 16):
        assert _name(hip, layout="NCHW", c=c) == row and _name(hip, layout="NCHW", c=c, dtype="f16", kind="avg") == row
    # the integer-domain max of the vector and row forms needs a positive finite input scale
    assert _name(hip, c=16, in_q=(-0.5, 0)) == gen and _name(hip, layout="NCHW", in_q=(0.0, 0)) == gen
    assert _name(hip, c=16, in_q=(-0.5, 0), kind="avg") == vec
    assert _name(hip, c=16, kernel=(0, 3)) == ""          # an invalid descriptor has no kernel
    monkeypatch.setenv("SHL_MI355X_POOL_FORM", "generic")
    assert _name(hip, c=16) == gen and _name(hip, layout="NCHW") == gen


def test_invalid_descriptors_and_empty_windows_are_refused_before_touching_the_device(built):
    import ctypes as C
    hip = pkg.load_hip()
    buf = np.zeros(64, np.int8)
    case = dict(kind="max", dtype="int8", layout="NHWC", n=1, c=16, h=4, w=4, ho=2, wo=2, kernel=(2, 2), stride=(2, 2),
                pad=(0, 0, 0, 0), cip=0, in_q=(0.0625, -5), out_q=(0.0625, -5))
    d = pool_cases.pool_desc(case)
    assert hip.shl_mi355x_pool2d(None, buf.ctypes.data, C.byref(d), None) == -2    # SHL_MI355X_EINVAL
    assert hip.shl_mi355x_pool2d(buf.ctypes.data, buf.ctypes.data, None, None) == -2
    # 3 output rows of a 2x2 stride-2 window on 4 rows: the third window lies below the image
    d = pool_cases.pool_desc(dict(case, ho=3))
    assert hip.shl_mi355x_pool2d(buf.ctypes.data, buf.ctypes.data, C.byref(d), None) == -2
    assert b"holds no input element" in hip.shl_mi355x_last_error()
    # a pad as large as the window: the first column's window lies left of the image
    d = pool_cases.pool_desc(dict(case, pad=(0, 2, 0, 0)))
    assert hip.shl_mi355x_pool2d(buf.ctypes.data, buf.ctypes.data, C.byref(d), None) == -2
    assert not buf.any()


def test_perf_callbacks_name_the_kernel_form(standalone, monkeypatch):
    """the backend's perf callback of both ops has the single-input signature and reports the form the rules choose"""
    import ctypes as C
    monkeypatch.delenv("SHL_MI355X_POOL_FORM", raising=False)
    fe, hip, opt = standalone
    opt.shl_cb_map_mi355x.restype = C.POINTER(pkg.Callback)
    opt.shl_cb_map_mi355x.argtypes = [C.c_int, C.c_int]
    tp = C.POINTER(pkg.Tensor)
    perf_t = C.CFUNCTYPE(C.c_int, tp, tp, C.c_void_p, C.POINTER(C.c_char_p))
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, pkg.API_MI355X, keep)
    for op in (pkg.OP_MAXPOOL2D, pkg.OP_AVGPOOL2D):
        for dt, layout, shape, out_shape, want in (
                (pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, (1, 8, 8, 16), (1, 4, 4, 16), b"pool2d_nhwc_vec"),
                (pkg.DTYPE_FLOAT16, pkg.LAYOUT_NCHW, (1, 3, 8, 8), (1, 3, 4, 4), b"pool2d_nchw_row"),
                (pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, (1, 8, 8, 20), (1, 4, 4, 20), b"pool2d_generic")):
            cb = opt.shl_cb_map_mi355x(op, dt)
            assert cb and cb.contents.perf and cb.contents.exec and not cb.contents.init
            t_in = pkg.make_tensor(fe, keep, shape, dt, layout, sess=sess)
            t_out = pkg.make_tensor(fe, keep, out_shape, dt, layout, sess=sess)
            p = pkg.pool_params(fe, keep, pkg.API_MI355X, layout, (2, 2), (2, 2), sess=sess)
            name = C.c_char_p()
            assert perf_t(cb.contents.perf)(t_in, t_out, p, C.byref(name)) == pkg.CSINN_TRUE
            assert name.value == want

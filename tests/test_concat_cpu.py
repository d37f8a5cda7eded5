"""Concat, the part that needs no GPU: the numpy restatement of the reference (concat_cases.concat_numpy) against the
genuine library's golden outputs and, where it is built, the live library; the op id and the params block; the exported
symbols; the kernel-form rules; refusals."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import concat_cases
from cases import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = concat_cases.concat_cases()
IDS = [c["name"] for c in CASES]
GOLD = concat_cases.golden()
VEC, GEN = "concat_vec", "concat_generic"


def test_golden_covers_the_case_list():
    assert sorted(GOLD) == sorted(IDS)


def test_case_list_covers_what_it_must():
    by = {c["name"]: c for c in CASES}
    assert {len(c["xs"]) for c in CASES} >= {1, 2, 4, 8, 9, 17}
    assert {c["axis"] for c in CASES} >= {-1, 0, 1, 2, 3} and {len(c["out_shape"]) for c in CASES} >= {1, 2, 4}
    assert any(len(set(c["alias"])) < len(c["alias"]) for c in CASES), "the same tensor given twice"
    assert any(0 in [x.size for x in c["xs"]] for c in CASES), "a zero-length input"
    assert by["exhaustive_f16_vec"]["xs"][0].size == 65536
    assert np.array_equal(by["exhaustive_f16_vec"]["xs"][0].view(np.uint16).ravel(), np.arange(65536, dtype=np.uint16))
    for key in concat_cases.RECORD_PAIRS:
        for x in by["exhaustive_i8_" + key]["xs"]:
            assert sorted(x.ravel().tolist()) == list(range(-128, 128))
    # every (input record, output record) pair of the int8 cases is walked exhaustively
    walked = {(q, by["exhaustive_i8_" + k]["out_q"]) for k in concat_cases.RECORD_PAIRS for q in by["exhaustive_i8_" + k]["in_qs"]}
    used = {(q, c["out_q"]) for c in CASES if c["dtype"] == "int8" for q in c["in_qs"]}
    assert used <= walked, used - walked


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_numpy_restatement_matches_the_reference_golden(case):
    concat_cases.assert_same(concat_cases.concat_numpy(case), GOLD[case["name"]], case["name"] + " vs golden")


def test_binary16_round_trip_changes_only_infinities_and_nans():
    """what the issue derives from the conversion's code, pinned by the genuine library's output"""
    got = GOLD["exhaustive_f16_vec"].ravel()[:65536].astype(np.uint32)
    h = np.arange(65536, dtype=np.uint32)
    mag, sign = h & 0x7FFF, h & 0x8000
    want = np.where(mag == 0x7C00, 0x7BFF | sign, np.where(mag > 0x7C00, 0x7FFF | sign, h))
    assert np.array_equal(got, want)
    assert int((got != h).sum()) == 2046


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_numpy_restatement_matches_the_live_reference():
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)  # errors only: the library warns about every binary16 saturation
    for case in CASES:
        got = concat_cases.concat_run(fe, pkg.API_REF, case)
        concat_cases.assert_same(concat_cases.concat_numpy(case), got, case["name"] + " vs live reference")
        concat_cases.assert_same(got, GOLD[case["name"]], case["name"] + ": live reference vs golden")


def _probe():
    spec = importlib.util.spec_from_file_location("make_concat_golden", os.path.join(HERE, "golden", "make_concat_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_op_id_and_params_block_match_the_reference():
    want = json.load(open(os.path.join(HERE, "golden", "concat_op_ids.json")))
    assert want == {"CSINN_OP_CONCAT": 26, "sizeof csinn_concat_params": 48, "offsetof csinn_concat_params.inputs_count": 40,
                    "offsetof csinn_concat_params.axis": 44}
    inc = os.path.join(cases.ROOT, "include")
    assert _probe().measure([inc, os.path.join(inc, "csinn")]) == want  # this repository's headers, compiled
    text = open(os.path.join(inc, "csinn", "csinn_data_structure.h")).read()
    assert int(re.search(r"\bCSINN_OP_CONCAT\s*=\s*(\d+)", text).group(1)) == 26
    assert pkg.OP_CONCAT == 26
    assert C.sizeof(pkg.ConcatParams) == 48
    assert (pkg.ConcatParams.inputs_count.offset, pkg.ConcatParams.axis.offset) == (40, 44)


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_libraries_export_the_concat_entry_points(built):
    assert {"csinn_concat_init", "csinn_concat", "shl_gref_concat"} <= _exports(pkg.lib_path("libcsinn_nn2.so"))
    assert {"shl_mi355x_concat_exec", "shl_mi355x_concat_perf"} <= _exports(pkg.lib_path("libshl_mi355x_opt.so"))
    assert {"shl_mi355x_concat", "shl_mi355x_concat_kernel_name"} <= _exports(pkg.lib_path("libshl_mi355x.so"))
    assert C.sizeof(pkg.ConcatDesc) == 40 and pkg.ConcatDesc.outer.offset == 8 and pkg.ConcatDesc.out_scale.offset == 16


def _case(dtype, lens, outer=3, in_qs=None, out_q=(0.0625, -5)):
    n = len(lens)
    return dict(dtype=dtype, axis=1, shapes=[(outer, c) for c in lens], out_shape=(outer, sum(lens)),
                in_qs=in_qs or [(0.0625, -5)] * n, out_q=out_q)


def _name(hip, dtype, lens, ptrs=None, out=1 << 30, **kw):
    ptrs = ptrs or [(i + 1) << 20 for i in range(len(lens))]  # made-up, aligned, disjoint: nothing is dereferenced
    return concat_cases.CabiArgs(_case(dtype, lens, **kw), ptrs).name(hip, out)


def test_kernel_form_rules(built, monkeypatch):
    """pure host code: no device is initialised, no pointer is followed"""
    monkeypatch.delenv("SHL_MI355X_CONCAT_FORM", raising=False)
    hip = pkg.load_hip()
    assert _name(hip, "int8", (16, 16)) == VEC and _name(hip, "int8", (16, 32, 48)) == VEC
    assert _name(hip, "int8", (16, 20)) == GEN      # the second length
    assert _name(hip, "int8", (20, 16)) == GEN      # the first length, so the second offset
    assert _name(hip, "int8", (3, 5)) == GEN
    assert _name(hip, "f16", (8, 8)) == VEC and _name(hip, "f16", (8, 24)) == VEC and _name(hip, "f16", (8, 12)) == GEN
    assert _name(hip, "int8", (16, 0, 16)) == VEC   # a zero-length input is dropped, whatever its pointer
    assert _name(hip, "int8", (16, 0, 16), ptrs=[1 << 20, 0, 3 << 20]) == VEC
    assert _name(hip, "int8", [16] * 17) == VEC and _name(hip, "int8", [16] * 16 + [8]) == GEN
    # pointer alignment: an input, and separately the output, one element off the 16-byte grid
    assert _name(hip, "int8", (16, 16), ptrs=[(1 << 20) + 1, 2 << 20]) == GEN
    assert _name(hip, "int8", (16, 16), out=(1 << 30) + 1) == GEN
    assert _name(hip, "f16", (8, 8), ptrs=[1 << 20, (2 << 20) + 2]) == GEN
    assert _name(hip, "f16", (8, 8), out=(1 << 30) + 2) == GEN
    assert _name(hip, "f16", (8, 8), out=(1 << 30) + 16) == VEC
    monkeypatch.setenv("SHL_MI355X_CONCAT_FORM", "generic")
    assert _name(hip, "int8", (16, 16)) == GEN and _name(hip, "f16", (8, 24)) == GEN
    monkeypatch.setenv("SHL_MI355X_CONCAT_FORM", "vec")  # only `generic` means anything
    assert _name(hip, "int8", (16, 16)) == VEC and _name(hip, "int8", (3, 5)) == GEN


POISON = 0x5A


def test_invalid_arguments_are_refused_before_touching_the_device(built):
    hip = pkg.load_hip()
    a = np.arange(48, dtype=np.int8)
    b = np.arange(48, dtype=np.int8)
    out = np.full(256, POISON, np.uint8)
    case = _case("int8", (16, 16))
    ok = concat_cases.CabiArgs(case, [a.ctypes.data, b.ctypes.data])
    EINVAL = -2

    def refused(args, out_ptr, text, call=None):
        rc = call() if call else args.run(hip, out_ptr)
        assert rc == EINVAL, (text, rc)
        assert text.encode() in hip.shl_mi355x_last_error(), (text, hip.shl_mi355x_last_error())
        if call is None:
            assert args.name(hip, out_ptr) == ""
    o = out.ctypes.data
    refused(ok, None, "NULL argument")
    refused(concat_cases.CabiArgs(case, [a.ctypes.data, None]), o, "NULL input")
    refused(ok, o, "NULL argument", call=lambda: hip.shl_mi355x_concat(None, ok.len, ok.scale, ok.zp, o, C.byref(ok.desc), None))
    refused(ok, o, "NULL argument", call=lambda: hip.shl_mi355x_concat(ok.ptrs, None, ok.scale, ok.zp, o, C.byref(ok.desc), None))
    refused(ok, o, "NULL argument", call=lambda: hip.shl_mi355x_concat(ok.ptrs, ok.len, None, ok.zp, o, C.byref(ok.desc), None))
    refused(ok, o, "NULL argument", call=lambda: hip.shl_mi355x_concat(ok.ptrs, ok.len, ok.scale, ok.zp, o, None, None))
    bad = concat_cases.CabiArgs(case, [a.ctypes.data, b.ctypes.data])
    bad.desc.n_inputs = 0
    refused(bad, o, "n_inputs < 1")
    bad = concat_cases.CabiArgs(case, [a.ctypes.data, b.ctypes.data])
    bad.len[1] = -16
    refused(bad, o, "negative length")
    bad = concat_cases.CabiArgs(case, [a.ctypes.data, b.ctypes.data])
    bad.desc.dtype = 2
    refused(bad, o, "dtype")
    bad = concat_cases.CabiArgs(case, [a.ctypes.data, b.ctypes.data])
    bad.desc.outer = -1
    refused(bad, o, "negative outer")
    # the output aliasing an input: the same address, and an overlap by the last byte of the input
    refused(concat_cases.CabiArgs(case, [a.ctypes.data, o]), o, "overlaps an input")
    refused(concat_cases.CabiArgs(case, [a.ctypes.data, o - 47]), o, "overlaps an input")
    assert np.all(out == POISON) and np.array_equal(a, np.arange(48, dtype=np.int8))
    # ... while an input that ends where the output begins, and the same input given twice, are fine to NAME
    assert concat_cases.CabiArgs(case, [a.ctypes.data, o - 48]).name(hip, o) != ""
    assert concat_cases.CabiArgs(case, [a.ctypes.data, a.ctypes.data]).name(hip, o) != ""


def _layer(fe, keep, sess, shapes, out_shape, axis, count=None, dtype=None, scales=None, in_dt=None):
    dt = dtype or pkg.DTYPE_INT8
    np_dt = np.int8 if dt == pkg.DTYPE_INT8 else np.float16
    ins = [pkg.make_tensor(fe, keep, s, in_dt or dt, pkg.LAYOUT_NHWC, data=np.zeros(s, np_dt), scales=scales or (0.5,), sess=sess)
           for s in shapes]
    out = np.zeros(out_shape, np_dt)
    out.view(np.uint8)[...] = POISON
    t_out = pkg.make_tensor(fe, keep, out_shape, dt, pkg.LAYOUT_NHWC, data=out, scales=(0.5,), sess=sess)
    p = pkg.concat_params(fe, keep, pkg.API_MI355X, pkg.LAYOUT_NHWC, len(shapes) if count is None else count, axis, sess)
    return pkg.tensor_array(keep, ins), t_out, p, out


@pytest.mark.parametrize("what,shapes,out_shape,axis,extra", [
    ("axis out of range", [(2, 4), (2, 4)], (2, 8), 2, {}),
    ("axis below -1", [(2, 4), (2, 4)], (2, 8), -2, {}),
    ("a non-axis dim differs", [(2, 4), (3, 4)], (2, 8), 1, {}),
    ("the axis dims do not sum to the output's", [(2, 4), (2, 4)], (2, 9), 1, {}),
    ("dim_count differs", [(2, 4), (1, 2, 4)], (2, 8), 1, {}),
    ("no input", [(2, 4)], (2, 4), 1, dict(count=0)),
    ("per-channel activation records", [(2, 4), (2, 4)], (2, 8), 1, dict(scales=(0.5,) * 4)),
    ("an input of another dtype", [(2, 4), (2, 4)], (2, 8), 1, dict(in_dt=pkg.DTYPE_FLOAT16)),
])
def test_mismatched_layers_are_refused_by_the_callback(standalone, what, shapes, out_shape, axis, extra):
    """where the reference would read past a buffer; refused before anything is staged, so no device is needed"""
    fe, _, _ = standalone
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, pkg.API_MI355X, keep)
    ins, t_out, p, out = _layer(fe, keep, sess, shapes, out_shape, axis, **extra)
    assert fe.csinn_concat_init(ins, t_out, p) == pkg.CSINN_TRUE
    assert fe.csinn_concat(ins, t_out, p) != pkg.CSINN_TRUE, what
    assert np.all(out.view(np.uint8) == POISON), what


def test_axis_minus_one_leaves_the_params_block_alone(standalone):
    fe, _, opt = standalone
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, pkg.API_MI355X, keep)
    ins, t_out, p, _ = _layer(fe, keep, sess, [(2, 3, 16), (2, 3, 16)], (2, 3, 32), -1)
    name = C.c_char_p()
    tp = C.POINTER(pkg.Tensor)
    opt.shl_mi355x_concat_perf.argtypes = [C.POINTER(tp), tp, C.c_void_p, C.POINTER(C.c_char_p)]
    assert opt.shl_mi355x_concat_perf(ins, t_out, p, C.byref(name)) == pkg.CSINN_TRUE
    assert name.value == VEC.encode()
    assert C.cast(p, C.POINTER(pkg.ConcatParams)).contents.axis == -1


def test_perf_callback_names_the_kernel_form(standalone, monkeypatch):
    """the backend's perf callback has the array-of-inputs signature and reports the form the rules choose"""
    monkeypatch.delenv("SHL_MI355X_CONCAT_FORM", raising=False)
    fe, hip, opt = standalone
    opt.shl_cb_map_mi355x.restype = C.POINTER(pkg.Callback)
    opt.shl_cb_map_mi355x.argtypes = [C.c_int, C.c_int]
    tp = C.POINTER(pkg.Tensor)
    perf_t = C.CFUNCTYPE(C.c_int, C.POINTER(tp), tp, C.c_void_p, C.POINTER(C.c_char_p))
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, pkg.API_MI355X, keep)
    for dt, shapes, out_shape, axis, want in (
            (pkg.DTYPE_INT8, [(1, 2, 2, 16), (1, 2, 2, 32)], (1, 2, 2, 48), 3, VEC),
            (pkg.DTYPE_INT8, [(1, 2, 2, 16), (1, 2, 2, 20)], (1, 2, 2, 36), 3, GEN),
            (pkg.DTYPE_FLOAT16, [(1, 2, 4, 4), (1, 4, 4, 4)], (1, 6, 4, 4), 1, VEC),
            (pkg.DTYPE_FLOAT16, [(1, 2, 3, 3), (1, 4, 3, 3)], (1, 6, 3, 3), 1, GEN)):
        cb = opt.shl_cb_map_mi355x(pkg.OP_CONCAT, dt)
        assert cb and cb.contents.perf and cb.contents.exec and cb.contents.est and not cb.contents.init
        ins, t_out, p, _ = _layer(fe, keep, sess, shapes, out_shape, axis, dtype=dt, scales=(1.0,) if dt == pkg.DTYPE_FLOAT16 else None)
        if dt == pkg.DTYPE_FLOAT16:
            t_out.contents.qinfo.contents.scale = 1.0
        name = C.c_char_p()
        assert perf_t(cb.contents.perf)(ins, t_out, p, C.byref(name)) == pkg.CSINN_TRUE
        assert name.value == want.encode()
    monkeypatch.setenv("SHL_MI355X_CONCAT_FORM", "generic")
    assert perf_t(cb.contents.perf)(ins, t_out, p, C.byref(name)) == pkg.CSINN_TRUE and name.value == GEN.encode()


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
@pytest.mark.parametrize("dtype,layout,const", [("int8", "NHWC", False), ("int8", "NHWC", True), ("f16", "NCHW", False),
                                                ("f16", "NCHW", True)])
def test_branchnet_oracle_chain_equals_the_genuine_graph_executor(dtype, layout, const):
    """the yardstick of tests/test_concat_session.py: BranchNet through the genuine front-end, graph executor and C
    kernels (CSINN_REF) gives the oracle chain's answer bit for bit, both dtypes, with and without the constant input"""
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)
    net = concat_cases.BranchNet(dtype, layout, const_input=const)
    net.build(fe, pkg.API_REF)
    for k in (0, 1):
        x = net.input(k)
        concat_cases.assert_same(net.run(fe, x), net.oracle(x), "BranchNet %s %s input %d" % (dtype, layout, k))
    net.close(fe)

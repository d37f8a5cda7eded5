"""Sigmoid family, leaky_relu and mul, the part that needs no GPU: the numpy restatement of the reference
(eltwise_cases.eltwise_numpy) against the genuine library's golden outputs and, where it is built, the live library; the op
ids and the params blocks; the exported symbols; the host-side table builders; the kernel-form rules; refusals."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import eltwise_cases
from cases import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = eltwise_cases.eltwise_cases()
IDS = [c["name"] for c in CASES]
BY = {c["name"]: c for c in CASES}
GOLD = eltwise_cases.golden()
VEC, ROW, GEN = "mul_vec", "mul_row", "mul_generic"
POISON = 0x5A
EINVAL = -2


def test_golden_covers_the_case_list():
    assert sorted(GOLD) == sorted(IDS)


def test_case_list_covers_what_it_must():
    every = list(range(-128, 128))
    for op in eltwise_cases.UNARY:
        for key in eltwise_cases.RECORD_PAIRS:
            names = [n for n in IDS if n.startswith("%s_i8_all_%s" % (op, key))]
            assert len(names) == (3 if op == "leaky_relu" else 1)
            for n in names:
                assert BY[n]["x"].ravel().tolist() == every and (BY[n]["in_q"], BY[n]["out_q"]) == eltwise_cases.RECORD_PAIRS[key]
        assert {BY[n]["x"].size for n in IDS if n.startswith(op + "_i8_count")} == {1, 15, 16, 17, 4101}
        assert {BY[n]["x"].size for n in IDS if n.startswith(op + "_f16_count")} == {1, 7, 8, 9}
        assert np.array_equal(BY[op + "_f16_all"]["x"].view(np.uint16), np.arange(65536, dtype=np.uint16))
    assert sorted({c["n"] for c in CASES if c["op"] == "leaky_relu" and "_all_" in c["name"] and c["dtype"] == "int8"}) == \
        sorted(float(np.float32(n)) for n in eltwise_cases.SLOPES)
    for key in eltwise_cases.RECORD_TRIPLES:
        c = BY["mul_i8_grid_" + key]
        pairs = set(zip(c["x"].ravel().tolist(), c["y"].ravel().tolist()))
        assert len(pairs) == 65536
    for key, h in eltwise_cases.F16_SCALARS.items():
        c = BY["mul_f16_all_by_" + key]
        assert c["y"].view(np.uint16).tolist() == [h] and np.array_equal(c["x"].view(np.uint16), np.arange(65536, dtype=np.uint16))
    assert any(c.get("small_first") for c in CASES) and any(c.get("b_const") for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_numpy_restatement_matches_the_reference_golden(case):
    eltwise_cases.assert_same(eltwise_cases.eltwise_numpy(case), GOLD[case["name"]], case["name"] + " vs golden")


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_numpy_restatement_matches_the_live_reference():
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)  # errors only: the library warns about every binary16 saturation
    for case in CASES:
        got = eltwise_cases.eltwise_run(fe, pkg.API_REF, case)
        eltwise_cases.assert_same(eltwise_cases.eltwise_numpy(case), got, case["name"] + " vs live reference")
        eltwise_cases.assert_same(got, GOLD[case["name"]], case["name"] + ": live reference vs golden")


def _probe():
    spec = importlib.util.spec_from_file_location("make_eltwise_golden", os.path.join(HERE, "golden", "make_eltwise_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_op_ids_and_params_blocks_match_the_reference():
    want = json.load(open(os.path.join(HERE, "golden", "eltwise_op_ids.json")))
    assert want == {"CSINN_OP_SIGMOID": 154, "CSINN_OP_HARD_SIGMOID": 78, "CSINN_OP_SILU": 190, "CSINN_OP_LEAKY_RELU": 84,
                    "CSINN_OP_MUL": 107, "sizeof csinn_sigmoid_params": 40, "sizeof csinn_relu_params": 56,
                    "sizeof csinn_diso_params": 40, "offsetof csinn_relu_params.n": 40}
    inc = os.path.join(cases.ROOT, "include")
    assert _probe().measure([inc, os.path.join(inc, "csinn")]) == want  # this repository's headers, compiled
    text = open(os.path.join(inc, "csinn", "csinn_data_structure.h")).read()
    for name in ("SIGMOID", "HARD_SIGMOID", "SILU", "LEAKY_RELU", "MUL"):
        assert int(re.search(r"\bCSINN_OP_%s\s*=\s*(\d+)" % name, text).group(1)) == want["CSINN_OP_" + name]
        assert getattr(pkg, "OP_" + name) == want["CSINN_OP_" + name]
    assert C.sizeof(pkg.SigmoidParams) == 40 and C.sizeof(pkg.ReluParams) == 56 and pkg.ReluParams.n.offset == 40
    assert C.sizeof(pkg.DisoParams) == 40


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_libraries_export_the_new_entry_points(built):
    ops = ("sigmoid", "hard_sigmoid", "silu", "leaky_relu", "mul")
    nn2 = _exports(pkg.lib_path("libcsinn_nn2.so"))
    opt = _exports(pkg.lib_path("libshl_mi355x_opt.so"))
    for op in ops:
        assert {"csinn_%s_init" % op, "csinn_" + op, "shl_gref_" + op} <= nn2, op
        assert {"shl_mi355x_%s_exec" % op, "shl_mi355x_%s_perf" % op} <= opt, op
        if op != "mul":
            assert "shl_mi355x_%s_table_i8" % op in opt
    assert {"shl_mi355x_unary_lut_i8", "shl_mi355x_unary_lut_i8_kernel_name", "shl_mi355x_unary_f16", "shl_mi355x_mul",
            "shl_mi355x_mul_kernel_name"} <= _exports(pkg.lib_path("libshl_mi355x.so"))
    assert C.sizeof(pkg.MulDesc) == 120 and pkg.MulDesc.b_stride.offset == 40 and pkg.MulDesc.a_scale.offset == 72


def _table(opt, case):
    t = (C.c_uint8 * 256)()
    a = (case["in_q"][0], case["in_q"][1], case["out_q"][0], case["out_q"][1])
    if case["op"] == "leaky_relu":
        opt.shl_mi355x_leaky_relu_table_i8(*a, case["n"], t)
    else:
        getattr(opt, "shl_mi355x_%s_table_i8" % case["op"])(*a, t)
    return np.frombuffer(t, dtype=np.uint8).view(np.int8).copy()


@pytest.mark.parametrize("name", [n for n in IDS if "_i8_all_" in n])
def test_host_table_builder_gives_the_reference_outputs(standalone, name):
    """the 256 entries the device looks up ARE the genuine library's outputs: no device needed to know the int8 ops exact"""
    _, _, opt = standalone
    case = BY[name]
    table = _table(opt, case)
    assert np.array_equal(table[case["x"].view(np.uint8)], GOLD[name].ravel()), name


def test_host_table_serves_every_int8_unary_case(standalone):
    _, _, opt = standalone
    for case in CASES:
        if case["dtype"] == "int8" and case["op"] != "mul":
            assert np.array_equal(_table(opt, case)[case["x"].view(np.uint8)], GOLD[case["name"]]), case["name"]


# ------------------------------------------------------------------------------------ kernel-form rules
A, B, O = 1 << 40, 2 << 40, 3 << 40  # made-up, aligned, disjoint: nothing is dereferenced


def _name(hip, dtype, a_shape, b_shape, a=A, b=B, out=O):
    case = dict(dtype=dtype, in_q=(0.0625, -5), in1_q=(0.0625, 3), out_q=(0.125, 1))
    return hip.shl_mi355x_mul_kernel_name(C.byref(eltwise_cases.mul_desc(case, a_shape, b_shape)), a, b, out).decode()


def test_mul_kernel_form_rules(built, monkeypatch):
    """pure host code: no device is initialised, no pointer is followed"""
    monkeypatch.delenv("SHL_MI355X_MUL_FORM", raising=False)
    hip = pkg.load_hip()
    for dtype, e in (("int8", 16), ("f16", 8)):
        es = 16 // e
        assert _name(hip, dtype, (2, 3, 5, 2 * e), (2, 1, 1, 2 * e)) == VEC      # NHWC gate
        assert _name(hip, dtype, (2, 3, 5, e + 4), (2, 1, 1, e + 4)) == GEN      # channels no whole pieces
        assert _name(hip, dtype, (2, 3, 5, e), (e,)) == VEC and _name(hip, dtype, (2, 3, 5, e), (1, 1, 1, e)) == VEC
        assert _name(hip, dtype, (2, 3, 5, e), (1,)) == VEC and _name(hip, dtype, (3, 7, 5), (1,)) == VEC  # a scalar, any count
        assert _name(hip, dtype, (3, 7, 5), (3, 7, 5)) == VEC                    # same shape, any count
        assert _name(hip, dtype, (2, 3, 4, 5), (2, 3, 1, 1)) == ROW and _name(hip, dtype, (2, 3, 4, 5), (1, 3, 1, 1)) == ROW
        assert _name(hip, dtype, (2, 3, 1, 37), (2, 3, 1, 1)) == ROW
        assert _name(hip, dtype, (2, 3, 1, 1), (2, 3, 1, 1)) == VEC              # H W = 1: nothing is broadcast
        assert _name(hip, dtype, (2, 3, 4, 5), (1, 1, 4, 1)) == ROW              # the innermost group is broadcast
        assert _name(hip, dtype, (2, 3, 4, 5), (1, 3, 1, 5)) == GEN              # b varies along a short innermost group
        # pointers one element off the 16-byte grid: a, out, and b where b is read in pieces
        assert _name(hip, dtype, (2, 3, 5, e), (e,), a=A + es) == GEN and _name(hip, dtype, (2, 3, 5, e), (e,), out=O + es) == GEN
        assert _name(hip, dtype, (2, 3, 5, e), (e,), b=B + es) == GEN and _name(hip, dtype, (4, e), (4, e), b=B + es) == GEN
        assert _name(hip, dtype, (2, 3, 5, e), (1,), b=B + es) == VEC            # a scalar b may lie anywhere
        assert _name(hip, dtype, (2, 3, 4, 5), (2, 3, 1, 1), b=B + es) == ROW    # ... and so may the row form's
        assert _name(hip, dtype, (2, 3, 4, 5), (2, 3, 1, 1), a=A + es) == GEN
        assert _name(hip, dtype, (2, 3, 5, e), (e,), a=A + 16, b=B + 32, out=O + 48) == VEC
    monkeypatch.setenv("SHL_MI355X_MUL_FORM", "generic")
    assert _name(hip, "int8", (2, 3, 5, 16), (16,)) == GEN and _name(hip, "f16", (2, 3, 4, 5), (2, 3, 1, 1)) == GEN
    monkeypatch.setenv("SHL_MI355X_MUL_FORM", "vec")  # only `generic` means anything
    assert _name(hip, "int8", (2, 3, 5, 16), (16,)) == VEC and _name(hip, "int8", (2, 3, 4, 5), (1, 3, 1, 5)) == GEN
    assert hip.shl_mi355x_unary_lut_i8_kernel_name(A, O) == b"unary_lut_i8_vec"
    assert hip.shl_mi355x_unary_lut_i8_kernel_name(A + 1, O) == b"unary_lut_i8_byte"
    assert hip.shl_mi355x_unary_lut_i8_kernel_name(A, O + 8) == b"unary_lut_i8_byte"


def test_every_mul_form_is_exercised_by_the_case_list(built, monkeypatch):
    monkeypatch.delenv("SHL_MI355X_MUL_FORM", raising=False)
    hip = pkg.load_hip()
    seen = {(hip.shl_mi355x_mul_kernel_name(C.byref(eltwise_cases.mul_desc(c)), A, B, O).decode(), c["dtype"])
            for c in CASES if c["op"] == "mul"}
    assert seen == {(f, d) for f in (VEC, ROW, GEN) for d in ("int8", "f16")}


# ------------------------------------------------------------------------------------ refusals
def test_invalid_arguments_are_refused_before_touching_the_device(built):
    hip = pkg.load_hip()
    a = np.arange(64, dtype=np.int8)
    b = np.arange(64, dtype=np.int8)
    out = np.full(256, POISON, np.uint8)
    table = np.zeros(256, np.uint8)
    o = out.ctypes.data

    def refused(rc, text):
        assert rc == EINVAL, (text, rc)
        assert text.encode() in hip.shl_mi355x_last_error(), (text, hip.shl_mi355x_last_error())
    refused(hip.shl_mi355x_unary_lut_i8(None, o, 64, table.ctypes.data, None), "NULL argument")
    refused(hip.shl_mi355x_unary_lut_i8(a.ctypes.data, None, 64, table.ctypes.data, None), "NULL argument")
    refused(hip.shl_mi355x_unary_lut_i8(a.ctypes.data, o, 64, None, None), "NULL argument")
    refused(hip.shl_mi355x_unary_lut_i8(a.ctypes.data, o, C.c_size_t(-1), table.ctypes.data, None), "negative count")
    refused(hip.shl_mi355x_unary_lut_i8(o + 63, o, 64, table.ctypes.data, None), "overlaps")
    refused(hip.shl_mi355x_unary_f16(None, o, 32, 0, 0.0, None), "NULL argument")
    refused(hip.shl_mi355x_unary_f16(a.ctypes.data, o, 32, 4, 0.0, None), "unknown kind")
    refused(hip.shl_mi355x_unary_f16(a.ctypes.data, o, 32, -1, 0.0, None), "unknown kind")
    refused(hip.shl_mi355x_unary_f16(a.ctypes.data, o, C.c_size_t(-1), 0, 0.0, None), "negative count")
    refused(hip.shl_mi355x_unary_f16(o + 2, o, 32, 0, 0.0, None), "overlaps")
    assert hip.shl_mi355x_unary_lut_i8(a.ctypes.data, o, 0, table.ctypes.data, None) == 0   # nothing to do: no launch
    assert hip.shl_mi355x_unary_f16(a.ctypes.data, o, 0, 0, 0.0, None) == 0
    case = dict(dtype="int8", in_q=(0.0625, -5), in1_q=(0.0625, 3), out_q=(0.125, 1))

    def mul(d, pa=a.ctypes.data, pb=b.ctypes.data, po=o):
        rc = hip.shl_mi355x_mul(pa, pb, po, C.byref(d) if d is not None else None, None)
        if rc != 0:
            assert hip.shl_mi355x_mul_kernel_name(C.byref(d) if d is not None else None, pa, pb, po) == b""
        return rc
    ok = eltwise_cases.mul_desc(case, (4, 16), (16,))
    refused(mul(None), "NULL argument")
    refused(mul(ok, pa=None), "NULL argument")
    refused(mul(ok, pb=None), "NULL argument")
    refused(mul(ok, po=None), "NULL argument")
    bad = eltwise_cases.mul_desc(case, (4, 16), (16,))
    bad.dtype = 2
    refused(mul(bad), "dtype")
    for n in (0, 5):
        bad = eltwise_cases.mul_desc(case, (4, 16), (16,))
        bad.ngroups = n
        refused(mul(bad), "ngroups")
    bad = eltwise_cases.mul_desc(case, (4, 16), (16,))
    bad.dim[0] = -4
    refused(mul(bad), "negative size")
    bad = eltwise_cases.mul_desc(case, (4, 16), (16,))
    bad.b_stride[1] = -1
    refused(mul(bad), "negative size")
    refused(mul(ok, pa=o + 63), "overlaps an input")
    refused(mul(ok, pb=o - 15), "overlaps an input")   # b holds 16 elements: its last byte is the output's first
    assert hip.shl_mi355x_mul_kernel_name(C.byref(ok), a.ctypes.data, o - 16, o) != b""
    empty = eltwise_cases.mul_desc(case, (4, 16), (16,))
    empty.dim[0] = 0
    assert mul(empty) == 0                             # no element: OK, no launch
    assert np.all(out == POISON) and np.array_equal(a, np.arange(64, dtype=np.int8))


REFUSALS = [
    ("both operands broadcast", "mul_i8_nhwc_gate_c16", dict(out_shape=(2, 3, 5, 16)), dict(x_shape=(2, 3, 1, 16))),
    ("the rule broken", "mul_i8_nhwc_gate_c16", dict(), dict(y_shape=(2, 1, 1, 8))),
    ("a higher-rank operand", "mul_i8_nhwc_channels", dict(), dict(y_shape=(1, 1, 1, 1, 16))),
    ("the second input of another dtype", "mul_i8_nhwc_channels", dict(in1_dtype="f16"), dict()),
    ("the output of another dtype", "mul_i8_nhwc_channels", dict(out_dtype="f16"), dict()),
    ("per-channel activation records", "mul_i8_nhwc_channels", dict(scales=(0.5,) * 4), dict()),
    ("fp16 scale != 1", "mul_f16_nhwc_channels", dict(out_q=(0.5, 0)), dict()),
    ("unary: the output of another dtype", "silu_i8_count16", dict(out_dtype="f16"), dict()),
    ("unary: per-channel activation records", "sigmoid_i8_count16", dict(scales=(0.5,) * 4), dict()),
    ("unary: fp16 scale != 1", "hard_sigmoid_f16_count8", dict(out_q=(2.0, 0)), dict()),
    ("unary: element counts differ", "leaky_relu_i8_count16", dict(out_shape=(17,)), dict()),
]


@pytest.mark.parametrize("what,name,override,reshape", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_mismatched_layers_are_refused_by_the_callback(standalone, what, name, override, reshape):
    """refused before anything is staged, so no device is needed; the output keeps its bytes"""
    fe, _, _ = standalone
    case = dict(BY[name])
    if "x_shape" in reshape:
        case["x"] = np.zeros(reshape["x_shape"], case["x"].dtype)
    if "y_shape" in reshape:
        case["y"] = np.zeros(reshape["y_shape"], case["y"].dtype)
    rc, out = eltwise_cases.eltwise_run(fe, pkg.API_MI355X, case, poison=POISON, **override)
    assert rc != pkg.CSINN_TRUE, what
    assert np.all(out.view(np.uint8) == POISON), what


def test_perf_callbacks_name_the_kernel_form(standalone, monkeypatch):
    monkeypatch.delenv("SHL_MI355X_MUL_FORM", raising=False)
    fe, hip, opt = standalone
    opt.shl_cb_map_mi355x.restype = C.POINTER(pkg.Callback)
    opt.shl_cb_map_mi355x.argtypes = [C.c_int, C.c_int]
    tp = C.POINTER(pkg.Tensor)
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, pkg.API_MI355X, keep)

    def T(shape, dt):
        np_dt = np.int8 if dt == pkg.DTYPE_INT8 else np.float16
        return pkg.make_tensor(fe, keep, shape, dt, pkg.LAYOUT_NHWC, data=np.zeros(shape, np_dt), sess=sess)
    for dt in (pkg.DTYPE_INT8, pkg.DTYPE_FLOAT16):
        for op in eltwise_cases.UNARY:
            cb = opt.shl_cb_map_mi355x(eltwise_cases.OPS[op], dt)
            assert cb and cb.contents.perf and cb.contents.exec and cb.contents.est and not cb.contents.init
            name = C.c_char_p()
            perf = C.CFUNCTYPE(C.c_int, tp, tp, C.c_void_p, C.POINTER(C.c_char_p))(cb.contents.perf)
            p = pkg.siso_params(fe, keep, pkg.API_MI355X, op, pkg.LAYOUT_NHWC, 1, sess)
            assert perf(T((2, 8), dt), T((2, 8), dt), p, C.byref(name)) == pkg.CSINN_TRUE
            assert name.value == (b"unary_lut_i8_vec" if dt == pkg.DTYPE_INT8 else b"unary_f16")
        cb = opt.shl_cb_map_mi355x(pkg.OP_MUL, dt)
        assert cb and cb.contents.perf and cb.contents.exec and cb.contents.est and not cb.contents.init
        perf = C.CFUNCTYPE(C.c_int, tp, tp, tp, C.c_void_p, C.POINTER(C.c_char_p))(cb.contents.perf)
        p = pkg.siso_params(fe, keep, pkg.API_MI355X, "mul", pkg.LAYOUT_NHWC, 1, sess)
        for a_shape, b_shape, want in (((2, 3, 5, 16), (2, 1, 1, 16), VEC), ((2, 3, 4, 5), (2, 3, 1, 1), ROW),
                                       ((2, 3, 5, 20), (2, 1, 1, 20), GEN)):
            name = C.c_char_p()
            assert perf(T(a_shape, dt), T(b_shape, dt), T(a_shape, dt), p, C.byref(name)) == pkg.CSINN_TRUE
            assert name.value == want.encode()
            assert perf(T(b_shape, dt), T(a_shape, dt), T(a_shape, dt), p, C.byref(name)) == pkg.CSINN_TRUE  # the small one first
            assert name.value == want.encode()


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
@pytest.mark.parametrize("dtype,layout,variant", [("int8", "NHWC", 0), ("int8", "NHWC", 1), ("f16", "NCHW", 0), ("f16", "NCHW", 1)])
def test_senet_oracle_chain_equals_the_genuine_graph_executor(dtype, layout, variant):
    """the yardstick of tests/test_eltwise_session.py: SeNet through the genuine front-end, graph executor and C kernels
    (CSINN_REF) gives the oracle chain's answer bit for bit, both dtypes, both variants"""
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)
    net = eltwise_cases.SeNet(dtype, layout, variant)
    net.build(fe, pkg.API_REF)
    for k in (0, 1):
        x = net.input(k)
        eltwise_cases.assert_same(net.run(fe, x), net.oracle(x), "SeNet %s %s variant %d input %d" % (dtype, layout, variant, k))
    assert not np.array_equal(net.oracle(net.input(0)), net.oracle(net.input(1))), "the two inputs must tell runs apart"
    net.close(fe)

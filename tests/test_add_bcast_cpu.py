"""The broadcasting add, the part that needs no GPU: the numpy restatement of the reference (add_bcast_cases.add_numpy)
against the genuine library's golden outputs and, where it is built, the live library; the exported symbols; the kernel-form
rule through shl_mi355x_add_bcast_kernel_name and through the perf callback of csinn_add; refusals, which write nothing."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import add_bcast_cases
import cases
import eltwise_cases
from cases import pkg

CASES = add_bcast_cases.add_cases()
IDS = [c["name"] for c in CASES]
BY = {c["name"]: c for c in CASES}
GOLD = add_bcast_cases.golden()
VEC, ROW, GEN = "add_vec", "add_row", "add_generic"
POISON = 0x5A
EINVAL = -2
# the form the rule picks for each geometry case on aligned pointers, int8 / binary16
FORMS = {
    "bias_n16": (VEC, VEC), "bias_n20": (GEN, GEN), "bias_2x17x64": (VEC, VEC), "posemb_2x17x64": (VEC, VEC),
    "attn_bias_2x2x17x17": (GEN, GEN),            # 2 17 17 = 578 elements per broadcast step: no whole pieces
    "nhwc_gate_c16": (VEC, VEC), "scalar": (VEC, VEC), "scalar_tail": (VEC, VEC),
    "nchw_channels": (ROW, ROW), "nchw_gate": (ROW, ROW), "nchw_hw1": (VEC, VEC),  # H W = 1: nothing is broadcast
    "nchw_hw4": (ROW, ROW), "nchw_hw37": (ROW, ROW), "nchw_middle": (ROW, ROW),
    "small_first_nhwc": (VEC, VEC), "small_first_nchw": (ROW, ROW), "const_bias": (VEC, VEC), "const_nchw": (ROW, ROW),
    "const_first_bias": (VEC, VEC), "const_first_nchw": (ROW, ROW),
}
GEOMETRY = [(("add_i8_" if k == 0 else "add_f16_") + key, forms[k]) for key, forms in FORMS.items() for k in (0, 1)]
A, B, O = 1 << 40, 2 << 40, 3 << 40  # made-up, aligned, disjoint: nothing is dereferenced


def test_golden_covers_the_case_list():
    assert sorted(GOLD) == sorted(IDS)


def test_case_list_covers_what_it_must():
    for key, q in eltwise_cases.RECORD_TRIPLES.items():
        c = BY["add_i8_grid_" + key]
        assert c["x"].shape == (256, 256) and c["y"].shape == (256,) and (c["in_q"], c["in1_q"], c["out_q"]) == q
        pairs = set(zip(c["x"].ravel().tolist(), np.broadcast_to(c["y"], c["x"].shape).ravel().tolist()))
        assert len(pairs) == 65536
    for key, h in eltwise_cases.F16_SCALARS.items():
        c = BY["add_f16_all_by_" + key]
        assert c["y"].view(np.uint16).tolist() == [h] and np.array_equal(c["x"].view(np.uint16), np.arange(65536, dtype=np.uint16))
    for name in ("add_f16_specials", "add_f16_specials_small_first"):
        c = BY[name]
        pairs = set(zip(c["x"].view(np.uint16).ravel().tolist(), np.broadcast_to(c["y"].view(np.uint16), c["x"].shape).ravel().tolist()))
        s = add_bcast_cases.F16_SPECIALS
        assert pairs == {(a, b) for a in s for b in s}
        assert (0x7C00, 0xFC00) in pairs and (0xFC00, 0x7C00) in pairs and (0x7E00, 0xFE00) in pairs and (0xFE00, 0x7E00) in pairs
    assert {n for n, _ in GEOMETRY} <= set(IDS)
    assert set(IDS) - {n for n, _ in GEOMETRY} == {n for n in IDS if "_grid_" in n or "_all_by_" in n or "_specials" in n or "x56x" in n
                                                   or "x28x" in n}
    shapes = {(c["x"].shape, c["y"].shape) for c in CASES}
    for pair in (((2, 3, 5, 16), (16,)), ((2, 3, 5, 20), (20,)), ((2, 17, 64), (64,)), ((2, 17, 64), (1, 17, 64)),
                 ((2, 2, 17, 17), (1, 2, 17, 17)), ((2, 3, 5, 16), (2, 1, 1, 16)), ((2, 3, 5, 16), (1,)), ((3, 7, 5), (1,)),
                 ((2, 3, 4, 5), (1, 3, 1, 1)), ((2, 3, 4, 5), (2, 3, 1, 1)), ((2, 3, 1, 1), (2, 3, 1, 1)), ((2, 3, 2, 2), (2, 3, 1, 1)),
                 ((2, 3, 1, 37), (2, 3, 1, 1)), ((2, 3, 4, 5), (1, 1, 4, 1)), ((2, 56, 56, 64), (64,)), ((2, 64, 28, 28), (1, 64, 1, 1))):
        assert pair in shapes, pair
    for dt in ("int8", "f16"):
        flags = {(c["small_first"], c["b_const"]) for c in CASES if c["dtype"] == dt}
        assert flags == {(False, False), (True, False), (False, True), (True, True)}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_numpy_restatement_matches_the_reference_golden(case):
    add_bcast_cases.assert_same(add_bcast_cases.add_numpy(case), GOLD[case["name"]], case["name"] + " vs golden")


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_numpy_restatement_matches_the_live_reference():
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)  # errors only: the library warns about every binary16 saturation
    for case in CASES:
        got = add_bcast_cases.add_run(fe, pkg.API_REF, case)
        add_bcast_cases.assert_same(add_bcast_cases.add_numpy(case), got, case["name"] + " vs live reference")
        add_bcast_cases.assert_same(got, GOLD[case["name"]], case["name"] + ": live reference vs golden")


def test_libraries_export_the_new_entry_points(built):
    def exports(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"shl_mi355x_add", "shl_mi355x_add_bcast", "shl_mi355x_add_bcast_kernel_name", "shl_mi355x_matmul_bias",
            "shl_mi355x_matmul_bias_kernel_name"} <= exports(pkg.lib_path("libshl_mi355x.so"))
    assert {"shl_mi355x_add_exec", "shl_mi355x_add_perf", "shl_mi355x_session_fused_linears"} <= exports(pkg.lib_path("libshl_mi355x_opt.so"))
    assert C.sizeof(pkg.MulDesc) == 120  # the descriptor is mul's, unchanged


# ------------------------------------------------------------------------------------ the form rule
def _name(hip, dtype, a_shape, b_shape, a=A, b=B, out=O):
    case = dict(dtype=dtype, in_q=(0.0625, -5), in1_q=(0.0625, 3), out_q=(0.125, 1))
    return hip.shl_mi355x_add_bcast_kernel_name(C.byref(add_bcast_cases.add_desc(case, a_shape, b_shape)), a, b, out).decode()


@pytest.mark.parametrize("name,want", GEOMETRY, ids=[n for n, _ in GEOMETRY])
def test_kernel_name_names_the_form_of_each_geometry_case(built, monkeypatch, name, want):
    """pure host code: no device is initialised, no pointer is followed"""
    hip = pkg.load_hip()
    monkeypatch.delenv("SHL_MI355X_ADD_FORM", raising=False)
    desc = add_bcast_cases.add_desc(BY[name])
    assert hip.shl_mi355x_add_bcast_kernel_name(C.byref(desc), A, B, O).decode() == want
    monkeypatch.setenv("SHL_MI355X_MUL_FORM", "generic")  # mul's switch is not add's
    assert hip.shl_mi355x_add_bcast_kernel_name(C.byref(desc), A, B, O).decode() == want
    monkeypatch.setenv("SHL_MI355X_ADD_FORM", "generic")
    assert hip.shl_mi355x_add_bcast_kernel_name(C.byref(desc), A, B, O).decode() == GEN
    monkeypatch.delenv("SHL_MI355X_MUL_FORM")
    assert hip.shl_mi355x_mul_kernel_name(C.byref(desc), A, B, O).decode() == want.replace("add_", "mul_")  # ... and the reverse


def test_every_form_is_exercised_by_the_case_list_and_the_large_cases_take_the_fast_forms(built, monkeypatch):
    monkeypatch.delenv("SHL_MI355X_ADD_FORM", raising=False)
    hip = pkg.load_hip()
    name = lambda c: hip.shl_mi355x_add_bcast_kernel_name(C.byref(add_bcast_cases.add_desc(c)), A, B, O).decode()
    assert {(name(c), c["dtype"]) for c in CASES} == {(f, d) for f in (VEC, ROW, GEN) for d in ("int8", "f16")}
    assert name(BY["add_i8_2x56x56x64_bias"]) == VEC and name(BY["add_f16_2x64x28x28_channels"]) == ROW
    for key in eltwise_cases.RECORD_TRIPLES:
        assert name(BY["add_i8_grid_" + key]) == VEC
    assert name(BY["add_f16_specials"]) == VEC and name(BY["add_f16_all_by_nan"]) == VEC


def test_form_rule_on_pointers_off_the_16_byte_grid(built, monkeypatch):
    monkeypatch.delenv("SHL_MI355X_ADD_FORM", raising=False)
    hip = pkg.load_hip()
    for dtype, e in (("int8", 16), ("f16", 8)):
        es = 16 // e
        assert _name(hip, dtype, (2, 17, 4 * e), (4 * e,)) == VEC                  # [.., N] + [N]: the bias
        assert _name(hip, dtype, (197, 768), (768,)) == VEC and _name(hip, dtype, (8, 197, 768), (1, 197, 768)) == VEC
        assert _name(hip, dtype, (2, 3, 5, e), (e,), a=A + es) == GEN and _name(hip, dtype, (2, 3, 5, e), (e,), out=O + es) == GEN
        assert _name(hip, dtype, (2, 3, 5, e), (e,), b=B + es) == GEN              # b is read in pieces
        assert _name(hip, dtype, (2, 3, 5, e), (1,), b=B + es) == VEC              # a scalar b may lie anywhere
        assert _name(hip, dtype, (2, 3, 4, 5), (1, 3, 1, 1), b=B + es) == ROW      # ... and so may the row form's
        assert _name(hip, dtype, (2, 3, 4, 5), (1, 3, 1, 1), a=A + es) == GEN
        assert _name(hip, dtype, (2, 3, 5, e), (e,), a=A + 16, b=B + 32, out=O + 48) == VEC
        assert _name(hip, dtype, (2, 3, 4, 5), (1, 3, 1, 5)) == GEN                # b varies along a short innermost group


def test_invalid_descriptors_are_refused_before_touching_the_device(built):
    hip = pkg.load_hip()
    a = np.arange(64, dtype=np.int8)
    b = np.arange(64, dtype=np.int8)
    out = np.full(256, POISON, np.uint8)
    o = out.ctypes.data
    case = dict(dtype="int8", in_q=(0.0625, -5), in1_q=(0.0625, 3), out_q=(0.125, 1))

    def add(d, pa=a.ctypes.data, pb=b.ctypes.data, po=o):
        ref = C.byref(d) if d is not None else None
        rc = hip.shl_mi355x_add_bcast(pa, pb, po, ref, None)
        assert (hip.shl_mi355x_add_bcast_kernel_name(ref, pa, pb, po) == b"") == (rc != 0)
        return rc

    def refused(rc, text):
        assert rc == EINVAL, (text, rc)
        assert b"add_bcast: " in hip.shl_mi355x_last_error() and text.encode() in hip.shl_mi355x_last_error(), hip.shl_mi355x_last_error()
    fresh = lambda: add_bcast_cases.add_desc(case, (4, 16), (16,))
    ok = fresh()
    refused(add(None), "NULL argument")
    refused(add(ok, pa=None), "NULL argument")
    refused(add(ok, pb=None), "NULL argument")
    refused(add(ok, po=None), "NULL argument")
    bad = fresh()
    bad.dtype = 2
    refused(add(bad), "dtype")
    for n in (0, 5):  # five groups
        bad = fresh()
        bad.ngroups = n
        refused(add(bad), "ngroups")
    bad = fresh()
    bad.dim[0] = -4
    refused(add(bad), "negative size")
    bad = fresh()
    bad.b_stride[1] = -1
    refused(add(bad), "negative size")
    bad = fresh()
    bad.dim[0], bad.dim[1] = 1 << 40, 1 << 40
    refused(add(bad), "too large")
    refused(add(ok, pa=o + 63), "overlaps an input")
    refused(add(ok, pb=o - 15), "overlaps an input")   # b holds 16 elements: its last byte is the output's first
    assert hip.shl_mi355x_add_bcast_kernel_name(C.byref(ok), a.ctypes.data, o - 16, o) != b""
    empty = fresh()
    empty.dim[0] = 0
    assert add(empty) == 0                             # no element: OK, no launch
    assert np.all(out == POISON) and np.array_equal(a, np.arange(64, dtype=np.int8))


REFUSALS = [
    ("both operands broadcast", "add_i8_nhwc_gate_c16", dict(out_shape=(2, 3, 5, 16)), dict(x_shape=(2, 3, 1, 16))),
    ("a dim that is neither equal nor 1", "add_i8_nhwc_gate_c16", dict(), dict(y_shape=(2, 1, 1, 8))),
    ("more than four groups", "add_i8_bias_n16", dict(out_shape=(2, 3, 2, 3, 2)), dict(x_shape=(2, 3, 2, 3, 2), y_shape=(2, 1, 2, 1, 2))),
    ("a higher-rank operand", "add_i8_bias_n16", dict(), dict(y_shape=(1, 1, 1, 1, 16))),
    ("the second input of another dtype", "add_i8_bias_n16", dict(in1_dtype="f16"), dict()),
    ("the output of another dtype", "add_i8_bias_n16", dict(out_dtype="f16"), dict()),
    ("per-channel records", "add_i8_bias_n16", dict(scales=(0.5,) * 4), dict()),
    ("fp16 scale != 1", "add_f16_bias_n16", dict(out_q=(0.5, 0)), dict()),
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
    rc, out = add_bcast_cases.add_run(fe, pkg.API_MI355X, case, poison=POISON, **override)
    assert rc != pkg.CSINN_TRUE, what
    assert np.all(out.view(np.uint8) == POISON), what


def _perf(fe, opt, dt):
    opt.shl_cb_map_mi355x.restype = C.POINTER(pkg.Callback)
    opt.shl_cb_map_mi355x.argtypes = [C.c_int, C.c_int]
    cb = opt.shl_cb_map_mi355x(3, dt)  # CSINN_OP_ADD
    assert cb and cb.contents.perf and cb.contents.exec and cb.contents.est and not cb.contents.init
    tp = C.POINTER(pkg.Tensor)
    return C.CFUNCTYPE(C.c_int, tp, tp, tp, C.c_void_p, C.POINTER(C.c_char_p))(cb.contents.perf)


@pytest.mark.parametrize("name,want", GEOMETRY, ids=[n for n, _ in GEOMETRY])
def test_perf_callback_of_csinn_add_names_the_form(standalone, monkeypatch, name, want):
    fe, hip, opt = standalone
    case = BY[name]
    dt = pkg.DTYPE_INT8 if case["dtype"] == "int8" else pkg.DTYPE_FLOAT16
    perf = _perf(fe, opt, dt)
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, pkg.API_MI355X, keep)
    T = lambda arr, const=0: pkg.make_tensor(fe, keep, arr.shape, dt, pkg.LAYOUT_NHWC, data=np.zeros_like(arr), sess=sess, is_const=const)
    p = pkg.siso_params(fe, keep, pkg.API_MI355X, "add", pkg.LAYOUT_NHWC, 1, sess)
    t_x, t_y, t_out = T(case["x"]), T(case["y"], 1 if case["b_const"] else 0), T(case["x"])
    args = (t_y, t_x) if case["small_first"] else (t_x, t_y)
    same_shape = case["x"].shape == case["y"].shape  # (H W = 1) such a layer is the residual add's: no form to name
    for force, expect in ((None, "" if same_shape else want), ("generic", "" if same_shape else GEN)):
        if force:
            monkeypatch.setenv("SHL_MI355X_ADD_FORM", force)
        else:
            monkeypatch.delenv("SHL_MI355X_ADD_FORM", raising=False)
        got = C.c_char_p()
        assert perf(*args, t_out, p, C.byref(got)) == pkg.CSINN_TRUE
        assert got.value == expect.encode()


def test_perf_callback_of_a_same_shape_add_reports_what_it_did(standalone, monkeypatch):
    """a residual add has no plan under its params block: the name is empty, as before, whatever the switch says"""
    fe, hip, opt = standalone
    monkeypatch.setenv("SHL_MI355X_ADD_FORM", "generic")
    for dt, np_dt in ((pkg.DTYPE_INT8, np.int8), (pkg.DTYPE_FLOAT16, np.float16)):
        perf = _perf(fe, opt, dt)
        keep = pkg.Keep()
        sess = pkg.layer_session(fe, pkg.API_MI355X, keep)
        T = lambda shape: pkg.make_tensor(fe, keep, shape, dt, pkg.LAYOUT_NHWC, data=np.zeros(shape, np_dt), sess=sess)
        p = pkg.siso_params(fe, keep, pkg.API_MI355X, "add", pkg.LAYOUT_NHWC, 1, sess)
        got = C.c_char_p(b"untouched")
        assert perf(T((2, 3, 5, 16)), T((2, 3, 5, 16)), T((2, 3, 5, 16)), p, C.byref(got)) == pkg.CSINN_TRUE
        assert got.value == opt.shl_mi355x_params_kernel_name(p) == b""

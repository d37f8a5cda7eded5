"""Resize, the part that needs no GPU: the numpy restatement of the reference (resize_cases.resize_numpy) against the genuine
library's golden outputs and, where it is built, the live library over a sweep of sizes; the op id, the mode enum and the
params block; the exported symbols; the host-side scale and table; the kernel-form rules; refusals."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import resize_cases
from cases import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = resize_cases.resize_cases()
IDS = [c["name"] for c in CASES]
BY = {c["name"]: c for c in CASES}
GOLD = resize_cases.golden()
VEC, ROW, GEN = "resize_nhwc_vec", "resize_nchw_row", "resize_generic"
POISON = 0x5A
EINVAL = -2
SWEEP = range(1, 25)  # n x n -> m x m for n, m in 1 .. 24


def test_golden_covers_the_case_list():
    assert sorted(GOLD) == sorted(IDS)
    assert os.path.getsize(os.path.join(HERE, "golden", "resize_cases.npz")) < 1 << 20


def test_case_list_covers_what_it_must():
    def has(**kw):
        return [c for c in CASES if all(c[k] == v for k, v in kw.items())]
    geometries = {(1, 1, 3, 4), (2, 2, 4, 4), (3, 5, 6, 10), (3, 5, 7, 11), (7, 9, 3, 4), (4, 6, 4, 6), (13, 17, 29, 37)}
    for mode in resize_cases.MODES:
        for h, w, ho, wo in geometries:
            for align in (False, True):
                for dtype in ("int8", "f16"):
                    for layout in ("NHWC", "NCHW"):
                        assert has(mode=mode, h=h, w=w, ho=ho, wo=wo, align=align, dtype=dtype, layout=layout), (mode, h, w, ho, wo, align)
        assert has(mode=mode, h=5, w=4, ho=1, wo=1, align=False) and not has(mode=mode, ho=1, align=True)
        assert {c["c"] for c in has(mode=mode, dtype="int8", layout="NHWC")} >= {1, 15, 16, 17, 32}
        assert {c["c"] for c in has(mode=mode, dtype="f16", layout="NHWC")} >= {7, 8, 9, 16}
        for dtype in ("int8", "f16"):
            assert {c["wo"] for c in has(mode=mode, dtype=dtype, layout="NCHW", c=3)} >= {1, 4, 37}
            for layout in ("NHWC", "NCHW"):
                assert has(mode=mode, dtype=dtype, layout=layout, n=2)
        every = list(range(-128, 128))
        for key, q in resize_cases.RECORD_PAIRS.items():
            for name, size, align in (("%s_i8_all_%s_to_32x32" % (mode, key), 32, False), ("%s_ac_i8_all_%s_to_31x31" % (mode, key), 31, True)):
                c = BY[name]
                assert sorted(c["x"].ravel().tolist()) == every and (c["in_q"], c["out_q"]) == q
                assert (c["ho"], c["wo"], c["align"]) == (size, size, align)
        specials = has(mode=mode, dtype="f16", h=4, w=4)
        assert any((c["ho"], c["wo"]) == (4, 4) for c in specials) and any((c["ho"], c["wo"]) != (4, 4) for c in specials)
        for c in specials:
            assert set(resize_cases.SPECIALS) <= set(c["x"].view(np.uint16).ravel().tolist())
        assert has(mode=mode, dtype="int8", layout="NHWC", n=1, c=32, h=28, w=28, ho=56, wo=56)
        assert has(mode=mode, dtype="f16", layout="NCHW", n=1, c=32, h=14, w=14, ho=28, wo=28)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_numpy_restatement_matches_the_reference_golden(case):
    resize_cases.assert_same(resize_cases.resize_numpy(case), GOLD[case["name"]], case["name"] + " vs golden")


def test_fused_multiply_add_model_rounds_once():
    """fma32 against exact rational arithmetic, including a sum that float64 would round twice"""
    import fractions
    rng = np.random.default_rng(3)
    a = rng.standard_normal(2000).astype(np.float32)
    b = rng.standard_normal(2000).astype(np.float32)
    c = (rng.standard_normal(2000) * 2.0 ** rng.integers(-30, 30, 2000)).astype(np.float32)
    # 2^24 + 2 - (1 - 2^-46) = 2^24 + 1 + 2^-46: float64 rounds it to the tie 2^24 + 1, which goes to the even 2^24; one
    # rounding gives 2^24 + 2
    a[0], b[0], c[0] = np.float32(1 + 2.0 ** -23), np.float32(-(1 - 2.0 ** -23)), np.float32(2.0 ** 24 + 2)
    got = resize_cases.fma32(a, b, c)
    assert got[0] == np.float32(2.0 ** 24 + 2)
    F = fractions.Fraction
    for i in range(a.size):
        assert got[i] == resize_cases._round_to_f32(F(float(a[i])) * F(float(b[i])) + F(float(c[i]))), i
    assert np.signbit(resize_cases.fma32(np.float32(-0.0), np.float32(1.0), np.float32(-0.0)))
    assert not np.signbit(resize_cases.fma32(np.float32(-0.0), np.float32(1.0), np.float32(0.0)))


def _sweep_case(mode, align, n, m, dtype="int8"):
    x = ((np.arange(n * n, dtype=np.int64) * 37 + 11) % 251 - 125).astype(np.int8).reshape(1, n, n, 1)
    q = resize_cases.RECORD_PAIRS["conv"] if dtype == "int8" else resize_cases.Q_F16
    if dtype == "f32":
        x = (x.astype(np.float32) * np.float32(0.0473) + np.float32(1 / 3)).astype(np.float32)
    return dict(name="sweep", mode=mode, align=align, dtype=dtype, layout="NHWC", n=1, c=1, h=n, w=n, ho=m, wo=m,
                in_q=q[0], out_q=q[1], x=x, out_shape=(1, m, m, 1))


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_numpy_restatement_matches_the_live_reference():
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)  # errors only: the library warns about every binary16 saturation
    for case in CASES:
        got = resize_cases.reference_run(fe, case)
        resize_cases.assert_same(resize_cases.resize_numpy(case), got, case["name"] + " vs live reference")
        resize_cases.assert_same(got, GOLD[case["name"]], case["name"] + ": live reference vs golden")


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
@pytest.mark.parametrize("mode", list(resize_cases.MODES))
def test_index_arithmetic_matches_the_live_reference_at_every_ratio(mode):
    """n x n -> m x m for n, m in 1 .. 24, one channel, int8: the index arithmetic at every ratio; bilinear in float32 as
    well, where no requantisation hides a rounding of the sum (which settles how the reference's build fuses it)"""
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)
    for n in SWEEP:
        for m in SWEEP:
            for align in (False, True):
                if align and m == 1:
                    continue  # the reference divides by zero
                case = _sweep_case(mode, align, n, m)
                what = "%s %dx%d -> %dx%d align_corners=%d" % (mode, n, n, m, m, align)
                resize_cases.assert_same(resize_cases.resize_numpy(case), resize_cases.resize_run(fe, pkg.API_REF, case), what)
                if mode == "bilinear":
                    case = _sweep_case(mode, align, n, m, "f32")
                    got = resize_cases.resize_run(fe, pkg.API_REF, case)
                    want = resize_cases.bilinear_f32(case["x"], m, m, align)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what + ", float32"


def _probe():
    spec = importlib.util.spec_from_file_location("make_resize_golden", os.path.join(HERE, "golden", "make_resize_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_op_id_enum_and_params_block_match_the_reference():
    want = json.load(open(os.path.join(HERE, "golden", "resize_op_ids.json")))
    assert want == {"CSINN_OP_RESIZE": 133, "CSINN_RESIZE_BILINEAR": 0, "CSINN_RESIZE_NEAREST_NEIGHBOR": 1,
                    "CSINN_RESIZE_NEAREST_BICUBIC": 2, "sizeof csinn_resize_params": 48,
                    "offsetof csinn_resize_params.resize_mode": 40, "offsetof csinn_resize_params.align_corners": 44}
    inc = os.path.join(cases.ROOT, "include")
    assert _probe().measure([inc, os.path.join(inc, "csinn")]) == want  # this repository's headers, compiled
    text = open(os.path.join(inc, "csinn", "csinn_data_structure.h")).read()
    assert int(re.search(r"\bCSINN_OP_RESIZE\s*=\s*(\d+)", text).group(1)) == want["CSINN_OP_RESIZE"] == pkg.OP_RESIZE
    assert (pkg.RESIZE_BILINEAR, pkg.RESIZE_NEAREST_NEIGHBOR, pkg.RESIZE_NEAREST_BICUBIC) == (0, 1, 2)
    assert C.sizeof(pkg.ResizeParams) == 48 and pkg.ResizeParams.resize_mode.offset == 40
    assert pkg.ResizeParams.align_corners.offset == 44


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_libraries_export_the_new_entry_points(built):
    assert {"csinn_resize_init", "csinn_resize", "shl_gref_resize"} <= _exports(pkg.lib_path("libcsinn_nn2.so"))
    assert {"shl_mi355x_resize_exec", "shl_mi355x_resize_perf", "shl_mi355x_resize_table_i8", "shl_mi355x_resize_scale"} <= \
        _exports(pkg.lib_path("libshl_mi355x_opt.so"))
    assert {"shl_mi355x_resize", "shl_mi355x_resize_kernel_name"} <= _exports(pkg.lib_path("libshl_mi355x.so"))
    assert C.sizeof(pkg.ResizeDesc) == 336 and pkg.ResizeDesc.height_scale.offset == 40 and pkg.ResizeDesc.table.offset == 64
    assert pkg.ResizeDesc.reserved.offset == 320


def test_host_scale_and_table_are_the_restatements(standalone):
    """what the backend computes on the host: the two scales (one float division each) and the int8 nearest table"""
    _, _, opt = standalone
    for i in SWEEP:
        for o in SWEEP:
            assert opt.shl_mi355x_resize_scale(i, o, 0) == float(resize_cases.scale_of(i, o, False)), (i, o)
            if o > 1:
                assert opt.shl_mi355x_resize_scale(i, o, 1) == float(resize_cases.scale_of(i, o, True)), (i, o)
    for key in resize_cases.RECORD_PAIRS:
        case = BY["nearest_i8_all_%s_to_32x32" % key]
        t = (C.c_uint8 * 256)()
        opt.shl_mi355x_resize_table_i8(case["in_q"][0], case["in_q"][1], case["out_q"][0], case["out_q"][1], t)
        assert bytes(t) == bytes(resize_cases.resize_desc(case).table), key
        # ... and the table alone gives the genuine library's nearest output
        table = np.frombuffer(t, dtype=np.uint8).view(np.int8)
        iy = resize_cases.nearest_indices(16, 32, False)
        assert np.array_equal(table[case["x"].view(np.uint8)][:, iy][:, :, iy], GOLD[case["name"]]), key


# ------------------------------------------------------------------------------------ kernel-form rules
A, O = 1 << 40, 3 << 40  # made-up, aligned, disjoint: nothing is dereferenced


def _name(hip, dtype, layout, c, a=A, out=O, **kw):
    case = dict(dtype=dtype, layout=layout, n=2, c=c, h=3, w=5, ho=7, wo=11, mode="bilinear", align=False, in_q=(0.0625, -5),
                out_q=(0.125, 1))
    case.update(kw)
    return hip.shl_mi355x_resize_kernel_name(C.byref(resize_cases.resize_desc(case)), a, out).decode()


def test_resize_kernel_form_rules(built, monkeypatch):
    """pure host code: no device is initialised, no pointer is followed"""
    monkeypatch.delenv("SHL_MI355X_RESIZE_FORM", raising=False)
    hip = pkg.load_hip()
    for dtype, e in (("int8", 16), ("f16", 8)):
        es = 16 // e
        for mode in resize_cases.MODES:
            # NHWC: C modulo the 16-byte piece, both pointers on the 16-byte grid
            assert _name(hip, dtype, "NHWC", e, mode=mode) == VEC and _name(hip, dtype, "NHWC", 3 * e, mode=mode) == VEC
            assert _name(hip, dtype, "NHWC", e - 1, mode=mode) == GEN and _name(hip, dtype, "NHWC", e + e // 2, mode=mode) == GEN
            assert _name(hip, dtype, "NHWC", 1, mode=mode) == GEN
            assert _name(hip, dtype, "NHWC", e, a=A + es, mode=mode) == GEN and _name(hip, dtype, "NHWC", e, out=O + es, mode=mode) == GEN
            assert _name(hip, dtype, "NHWC", e, a=A + 16, out=O + 48, mode=mode) == VEC
            # NCHW: any channel count; the output on the 4-byte grid, the input anywhere
            assert _name(hip, dtype, "NCHW", 3, mode=mode) == ROW and _name(hip, dtype, "NCHW", e, mode=mode) == ROW
            assert _name(hip, dtype, "NCHW", 3, wo=1, ho=1, mode=mode) == ROW
            assert _name(hip, dtype, "NCHW", 3, out=O + es, mode=mode) == GEN
            assert _name(hip, dtype, "NCHW", 3, a=A + es, mode=mode) == ROW
            assert _name(hip, dtype, "NCHW", 3, a=A + 16, out=O + 4, mode=mode) == ROW
    monkeypatch.setenv("SHL_MI355X_RESIZE_FORM", "generic")
    assert _name(hip, "int8", "NHWC", 16) == GEN and _name(hip, "f16", "NCHW", 3) == GEN
    monkeypatch.setenv("SHL_MI355X_RESIZE_FORM", "vec")  # only `generic` means anything
    assert _name(hip, "int8", "NHWC", 16) == VEC and _name(hip, "int8", "NHWC", 15) == GEN and _name(hip, "f16", "NCHW", 3) == ROW


def test_every_form_is_exercised_by_the_case_list(built, monkeypatch):
    monkeypatch.delenv("SHL_MI355X_RESIZE_FORM", raising=False)
    hip = pkg.load_hip()
    seen = {(hip.shl_mi355x_resize_kernel_name(C.byref(resize_cases.resize_desc(c)), A, O).decode(), c["dtype"], c["mode"])
            for c in CASES}
    assert seen == {(f, d, m) for f in (VEC, ROW, GEN) for d in ("int8", "f16") for m in resize_cases.MODES}


# ------------------------------------------------------------------------------------ refusals
def test_invalid_arguments_are_refused_before_touching_the_device(built):
    hip = pkg.load_hip()
    case = BY["bilinear_3x5_to_7x11_i8_nhwc_c16"]
    a = np.ascontiguousarray(case["x"])
    out = np.full(case["ho"] * case["wo"] * case["c"] + 64, POISON, np.uint8)
    o = out.ctypes.data

    def call(d, pa=a.ctypes.data, po=o):
        ref = C.byref(d) if d is not None else None
        rc = hip.shl_mi355x_resize(pa, po, ref, None)
        if rc != 0:
            assert hip.shl_mi355x_resize_kernel_name(ref, pa, po) == b""
        return rc

    def refused(rc, text):
        assert rc == EINVAL, (text, rc)
        assert text.encode() in hip.shl_mi355x_last_error(), (text, hip.shl_mi355x_last_error())
    ok = resize_cases.resize_desc(case)
    assert hip.shl_mi355x_resize_kernel_name(C.byref(ok), a.ctypes.data, o) != b""
    refused(call(None), "NULL argument")
    refused(call(ok, pa=None), "NULL argument")
    refused(call(ok, po=None), "NULL argument")
    refused(call(resize_cases.resize_desc(case, dtype=2)), "dtype")
    refused(call(resize_cases.resize_desc(case, layout=2)), "layout")
    refused(call(resize_cases.resize_desc(case, mode=pkg.RESIZE_NEAREST_BICUBIC)), "bicubic")
    refused(call(resize_cases.resize_desc(case, mode=3)), "unknown mode")
    refused(call(resize_cases.resize_desc(case, align_corners=2)), "align_corners")
    refused(call(resize_cases.resize_desc(case, align_corners=1, out_h=1)), "align_corners with an output extent of 1")
    refused(call(resize_cases.resize_desc(case, align_corners=1, out_w=1)), "align_corners with an output extent of 1")
    refused(call(resize_cases.resize_desc(case, n=-1)), "negative size")
    refused(call(resize_cases.resize_desc(case, out_w=-3)), "negative size")
    refused(call(resize_cases.resize_desc(case, in_h=0)), "an input without pixels")
    for field in ("height_scale", "width_scale"):
        for bad in (-0.5, float("nan"), float("inf"), 64.0):
            d = resize_cases.resize_desc(case)
            setattr(d, field, bad)
            refused(call(d), "a scale that is")
    d = resize_cases.resize_desc(case)
    d.reserved[2] = 1
    refused(call(d), "reserved")
    refused(call(ok, pa=o + 63), "overlaps the input")
    refused(call(ok, po=a.ctypes.data + a.nbytes - 1), "overlaps the input")
    assert hip.shl_mi355x_resize_kernel_name(C.byref(ok), o - a.nbytes, o) != b""   # touching is not overlapping
    assert call(resize_cases.resize_desc(case, n=0)) == 0 and call(resize_cases.resize_desc(case, out_h=0)) == 0  # no element: no launch
    assert np.all(out == POISON) and np.array_equal(a, case["x"])


REFUSALS = [
    ("align_corners with an output height of 1", "bilinear_5x4_to_1x1_i8_nhwc_c16", dict(align=True)),
    ("align_corners with an output width of 1", "nearest_3x5_to_7x11_f16_nchw_c3", dict(align=True, out_shape=(1, 3, 7, 1))),
    ("bicubic", "nearest_3x5_to_7x11_i8_nhwc_c16", dict(mode=pkg.RESIZE_NEAREST_BICUBIC)),
    ("batch counts differ", "nearest_3x5_to_6x10_i8_nhwc_c16", dict(out_shape=(1, 6, 10, 16))),
    ("channel counts differ", "bilinear_3x5_to_7x11_f16_nchw_c3", dict(out_shape=(1, 4, 7, 11))),
    ("channel counts differ, NHWC", "bilinear_3x5_to_7x11_i8_nhwc_c16", dict(out_shape=(1, 7, 11, 15))),
    ("a 3-d tensor", "nearest_3x5_to_7x11_i8_nhwc_c16", dict(in_shape=(3, 5, 16), out_shape=(7, 11, 16))),
    ("a 5-d output", "nearest_3x5_to_7x11_i8_nhwc_c16", dict(out_shape=(1, 1, 7, 11, 16))),
    ("float32", "nearest_3x5_to_7x11_i8_nhwc_c16", dict(in_dtype="f32")),
    ("the output of another dtype", "bilinear_3x5_to_7x11_i8_nhwc_c16", dict(out_dtype="f16")),
    ("per-channel activation records", "bilinear_3x5_to_7x11_i8_nhwc_c16", dict(scales=(0.5,) * 4)),
    ("fp16 scale != 1", "bilinear_3x5_to_7x11_f16_nhwc_c8", dict(out_q=(0.5, 0))),
]


@pytest.mark.parametrize("what,name,override", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_mismatched_layers_are_refused_by_the_callback(standalone, what, name, override):
    """refused before anything is staged, so no device is needed; the output keeps its bytes"""
    fe, _, _ = standalone
    rc, out = resize_cases.resize_run(fe, pkg.API_MI355X, BY[name], poison=POISON, **override)
    assert rc != pkg.CSINN_TRUE, what
    assert np.all(out.view(np.uint8) == POISON), what


def test_perf_callback_names_the_kernel_form(standalone, monkeypatch):
    monkeypatch.delenv("SHL_MI355X_RESIZE_FORM", raising=False)
    fe, hip, opt = standalone
    opt.shl_cb_map_mi355x.restype = C.POINTER(pkg.Callback)
    opt.shl_cb_map_mi355x.argtypes = [C.c_int, C.c_int]
    tp = C.POINTER(pkg.Tensor)
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, pkg.API_MI355X, keep)

    def T(shape, dt, layout):
        np_dt = np.int8 if dt == pkg.DTYPE_INT8 else np.float16
        return pkg.make_tensor(fe, keep, shape, dt, layout, data=np.zeros(shape, np_dt), sess=sess)
    for dt, e in ((pkg.DTYPE_INT8, 16), (pkg.DTYPE_FLOAT16, 8)):
        cb = opt.shl_cb_map_mi355x(pkg.OP_RESIZE, dt)
        assert cb and cb.contents.perf and cb.contents.exec and cb.contents.est and not cb.contents.init
        perf = C.CFUNCTYPE(C.c_int, tp, tp, C.c_void_p, C.POINTER(C.c_char_p))(cb.contents.perf)
        for layout, shape_in, shape_out, want in ((pkg.LAYOUT_NHWC, (1, 3, 5, e), (1, 6, 10, e), VEC),
                                                  (pkg.LAYOUT_NHWC, (1, 3, 5, e + 1), (1, 6, 10, e + 1), GEN),
                                                  (pkg.LAYOUT_NCHW, (1, 3, 3, 5), (1, 3, 6, 10), ROW)):
            for mode in resize_cases.MODES.values():
                name = C.c_char_p()
                p = pkg.resize_params(fe, keep, pkg.API_MI355X, layout, mode, False, sess)
                assert perf(T(shape_in, dt, layout), T(shape_out, dt, layout), p, C.byref(name)) == pkg.CSINN_TRUE
                assert name.value == want.encode()
        p = pkg.resize_params(fe, keep, pkg.API_MI355X, pkg.LAYOUT_NHWC, pkg.RESIZE_NEAREST_BICUBIC, False, sess)
        assert perf(T((1, 3, 5, e), dt, pkg.LAYOUT_NHWC), T((1, 6, 10, e), dt, pkg.LAYOUT_NHWC), p, C.byref(C.c_char_p())) != pkg.CSINN_TRUE
    assert not opt.shl_cb_map_mi355x(pkg.OP_RESIZE, pkg.DTYPE_FLOAT32)


NETS = [("int8", "NHWC", 0), ("int8", "NHWC", 1), ("f16", "NCHW", 0), ("f16", "NCHW", 1)]


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
@pytest.mark.parametrize("dtype,layout,variant", NETS)
def test_pyramidnet_oracle_chain_equals_the_genuine_graph_executor(dtype, layout, variant):
    """the yardstick of tests/test_resize_session.py: PyramidNet through the genuine front-end, graph executor and C kernels
    (CSINN_REF) gives the oracle chain's answer bit for bit, both dtypes, both variants"""
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)
    net = resize_cases.PyramidNet(dtype, layout, variant)
    net.build(fe, pkg.API_REF)
    for k in (0, 1):
        x = net.input(k)
        resize_cases.assert_same(net.run(fe, x), net.oracle(x), "PyramidNet %s %s variant %d input %d" % (dtype, layout, variant, k))
    assert not np.array_equal(net.oracle(net.input(0)), net.oracle(net.input(1))), "the two inputs must tell runs apart"
    net.close(fe)

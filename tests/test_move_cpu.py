"""Transpose, pad, reshape and flatten, the part that needs no GPU: the numpy restatements of the reference against the genuine
library's golden outputs and, where it is built, the live library; the op ids and the params blocks; the exported symbols;
the stand-alone front-end and graph executor; canonicalisation and the kernel-form rules; refusals; the host code that takes
descriptors apart under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import cases
import move_cases as mc
from cases import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = mc.all_cases()
IDS = [mc.case_id(c) for c in CASES]
GOLD = mc.golden()
BY_KEY = {mc.golden_key(c): c for c in CASES}
POISON = 0x5A
EINVAL = -2
TP = C.POINTER(pkg.Tensor)


def test_golden_covers_the_case_list():
    assert sorted(GOLD) == sorted(mc.golden_key(c) for c in CASES)
    size = os.path.getsize(os.path.join(HERE, "golden", "move_cases.npz"))
    assert size < os.path.getsize(os.path.join(HERE, "golden", "split_shuffle_cases.npz"))


def test_case_list_covers_what_it_must():
    tr = [c for c in CASES if c["op"] == "transpose"]
    shapes = {(c["x"].shape, c["perm"]) for c in tr}
    assert shapes >= {((3, 5), (1, 0)), ((64, 64), (1, 0)), ((65, 67), (1, 0)), ((128, 4), (1, 0)), ((4, 128), (1, 0)),
                      ((2, 3, 5, 7), (0, 2, 3, 1)), ((2, 3, 5, 7), (0, 3, 1, 2)), ((1, 64, 8, 8), (0, 2, 3, 1)),
                      ((2, 16, 7, 7), (0, 2, 3, 1)), ((1, 3, 8, 4, 4), (0, 1, 3, 4, 2)), ((2, 5, 4, 16), (0, 2, 1, 3)),
                      ((2, 5, 4, 6), (0, 2, 1, 3)), ((2, 3, 4, 5), (3, 2, 1, 0)), ((2, 3, 4, 5), (2, 0, 3, 1)),
                      ((1, 1, 7, 3), (3, 1, 2, 0)), ((2, 3, 4, 5), (0, 1, 2, 3)), ((2, 2, 3, 2, 2, 3), (0, 3, 1, 4, 2, 5))}
    assert any(c["x"].ndim == 8 and c["x"].size == 256 for c in tr)
    for op in ("transpose", "pad", "reshape", "flatten"):
        mine = [c for c in CASES if c["op"] == op]
        assert {c["dtype"] for c in mine} == {"int8", "f16"}
        recs = {(c["in_q"], c["out_q"]) for c in mine if c["dtype"] == "int8"}
        assert recs >= set(mc.RECORDS.values()), op
    # binary16 inputs carry +-inf, NaNs of both signs, subnormals and +-0 wherever the tensor has room for them
    for c in CASES:
        if c["dtype"] == "f16":
            have = set(c["x"].view(np.uint16).ravel().tolist())
            assert len(have & set(mc.F16_SPECIALS.tolist())) == min(len(mc.F16_SPECIALS), c["x"].size), mc.case_id(c)
    pads = [c for c in CASES if c["op"] == "pad"]
    assert {c["layout"] for c in pads} == {"NHWC", "NCHW"}
    assert {c["value"] for c in pads} >= {0.0, -1.5, 1000.0, -1000.0, -np.inf}
    for c in pads:  # the reference's own float-to-int conversion of the pad value is defined
        if c["dtype"] == "int8":
            assert abs(c["value"] / c["out_q"][0]) < 2 ** 20, mc.case_id(c)
    assert {c["x"].size for c in CASES if c["op"] in ("reshape", "flatten")} >= {1, 15, 16, 17, 4099, 48, 384}
    # the division path: an output scale div_by_scale does not admit
    assert mc.RECORDS["div"][1][0] < 2.0 ** -40


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_numpy_restatement_matches_the_reference_golden(case):
    mc.assert_same(mc.move_numpy(case), GOLD[mc.golden_key(case)], mc.case_id(case) + " vs golden")


def test_pad_elements_of_the_golden_are_the_documented_ones():
    g = GOLD["pad.value_minus_inf_nhwc_f16"]
    assert g[0, 0, 0, 0] == 0xFBFF and GOLD["pad.value_plus_inf_nhwc_f16"][0, 0, 0, 0] == 0x7BFF
    assert GOLD["pad.saturates_up_nhwc_i8_eq"][0, 0, 0, 0] == 127 and GOLD["pad.saturates_down_nhwc_i8_eq"][0, 0, 0, 0] == -128


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_numpy_restatement_matches_the_live_reference_and_the_generator_is_reproducible():
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)  # errors only: the library warns about every binary16 saturation
    for case in CASES:
        got = mc.layer_run(fe, pkg.API_REF, case)
        mc.assert_same(mc.move_numpy(case), got, mc.case_id(case) + " vs live reference")
        mc.assert_same(got, GOLD[mc.golden_key(case)], mc.case_id(case) + ": live reference vs golden")
    again = mc.all_cases()
    for a, b in zip(CASES, again):
        assert np.array_equal(mc.bits(a["x"]), mc.bits(b["x"])), "inputs are regenerated from seeds"


def _probe():
    spec = importlib.util.spec_from_file_location("make_move_golden", os.path.join(HERE, "golden", "make_move_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_op_ids_and_params_blocks_match_the_reference():
    want = json.load(open(os.path.join(HERE, "golden", "move_op_ids.json")))
    assert want == {"CSINN_OP_TRANSPOSE": 179, "CSINN_OP_RESHAPE": 132, "CSINN_OP_FLATTEN": 66, "CSINN_OP_PAD": 115,
                    "CSINN_PAD_CONSTANT": 0, "CSINN_PAD_EDGE": 1, "CSINN_PAD_REFLECT": 2,
                    "sizeof csinn_transpose_params": 56, "offsetof csinn_transpose_params.permute": 40,
                    "offsetof csinn_transpose_params.permute_num": 48,
                    "sizeof csinn_reshape_params": 56, "offsetof csinn_reshape_params.shape": 40,
                    "offsetof csinn_reshape_params.shape_num": 48,
                    "sizeof csinn_flatten_params": 48, "offsetof csinn_flatten_params.axis": 40,
                    "sizeof csinn_pad_params": 72, "offsetof csinn_pad_params.pad_before": 40,
                    "offsetof csinn_pad_params.pad_after": 48, "offsetof csinn_pad_params.pad_num": 56,
                    "offsetof csinn_pad_params.pad_value": 60, "offsetof csinn_pad_params.pad_mode": 64}
    inc = os.path.join(cases.ROOT, "include")
    assert _probe().measure([inc, os.path.join(inc, "csinn")]) == want  # this repository's headers, compiled
    text = open(os.path.join(inc, "csinn", "csinn_data_structure.h")).read()
    for op in ("TRANSPOSE", "RESHAPE", "FLATTEN", "PAD"):
        assert int(re.search(r"\bCSINN_OP_%s\s*=\s*(\d+)" % op, text).group(1)) == want["CSINN_OP_" + op]
    assert (pkg.OP_TRANSPOSE, pkg.OP_RESHAPE, pkg.OP_FLATTEN, pkg.OP_PAD) == (179, 132, 66, 115)
    assert (pkg.PAD_CONSTANT, pkg.PAD_EDGE, pkg.PAD_REFLECT) == (0, 1, 2)
    for cls, name in ((pkg.TransposeParams, "csinn_transpose_params"), (pkg.ReshapeParams, "csinn_reshape_params"),
                      (pkg.FlattenParams, "csinn_flatten_params"), (pkg.PadParams, "csinn_pad_params")):
        assert C.sizeof(cls) == want["sizeof " + name]
        for field, _ in cls._fields_[1:]:
            assert getattr(cls, field).offset == want["offsetof %s.%s" % (name, field)], (name, field)


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_libraries_export_the_entry_points(built):
    ops = ("transpose", "reshape", "flatten", "pad")
    front = {"csinn_%s%s" % (op, s) for op in ops for s in ("", "_init")} | {"shl_gref_" + op for op in ops}
    assert front <= _exports(pkg.lib_path("libcsinn_nn2.so"))
    back = {"shl_mi355x_%s_%s" % (op, s) for op in ops for s in ("init", "exec", "perf")}
    assert back <= _exports(pkg.lib_path("libshl_mi355x_opt.so"))
    assert {"shl_mi355x_transpose", "shl_mi355x_transpose_kernel_name", "shl_mi355x_move", "shl_mi355x_move_kernel_name",
            "shl_mi355x_pad", "shl_mi355x_pad_kernel_name", "shl_mi355x_pad_element"} <= _exports(pkg.lib_path("libshl_mi355x.so"))
    assert C.sizeof(pkg.TransposeDesc) == 104 and pkg.TransposeDesc.perm.offset == 40 and pkg.TransposeDesc.in_scale.offset == 72
    assert C.sizeof(pkg.MoveDesc) == 32 and pkg.MoveDesc.out_zp.offset == 16
    assert C.sizeof(pkg.PadDesc) == 88 and pkg.PadDesc.pad_value.offset == 52 and pkg.PadDesc.out_zp.offset == 68


# ------------------------------------------------------------------------------------ front-end and graph executor
FAKE_API = 6  # an unused slot of the dispatch tables
KEEP_ALIVE = []  # the C side keeps the callbacks' addresses


class Node(C.Structure):
    """struct shl_node (include/shl_gref.h)"""


Node._fields_ = [("type", C.c_int), ("in_", C.POINTER(C.POINTER(Node))), ("out", C.POINTER(C.POINTER(Node))),
                 ("subgraph_idx", C.c_int), ("in_num", C.c_int), ("out_num", C.c_int), ("name", C.c_char_p), ("data", C.c_void_p)]


class HostBackend:
    """the four ops on the host, in numpy, registered in slot FAKE_API: what the graph executor's host path calls; records
    every call"""

    def __init__(self, fe):
        self.fe, self.log, self.table = fe, [], {}
        fe.shl_gref_runtime_callback.restype = C.c_void_p
        fe.shl_gref_runtime_callback.argtypes = [C.c_int]

        def view(t):
            tc = t.contents
            shape = tuple(tc.dim[i] for i in range(tc.dim_count))
            return np.ctypeslib.as_array(C.cast(tc.data, C.POINTER(C.c_int8)), shape)

        def rec(t):
            return (t.contents.qinfo.contents.scale, t.contents.qinfo.contents.zero_point)

        def make(op):
            def run(i, o, p):
                x, out = view(i), view(o)
                case = dict(op=op, dtype="int8", in_q=rec(i), out_q=rec(o), x=x, out_shape=out.shape)
                if op == "transpose":
                    pc = C.cast(p, C.POINTER(pkg.TransposeParams)).contents
                    case["perm"] = [pc.permute[k] for k in range(pc.permute_num)]
                elif op == "pad":
                    pc = C.cast(p, C.POINTER(pkg.PadParams)).contents
                    case["before"] = [pc.pad_before[k] for k in range(pc.pad_num)]
                    case["after"] = [pc.pad_after[k] for k in range(pc.pad_num)]
                    case["value"] = pc.pad_value
                self.log.append(op)
                out[...] = mc.move_numpy(case)
                return 1
            return C.CFUNCTYPE(C.c_int, TP, TP, C.c_void_p)(run)
        ids = {pkg.OP_TRANSPOSE: "transpose", pkg.OP_RESHAPE: "reshape", pkg.OP_FLATTEN: "flatten", pkg.OP_PAD: "pad"}
        fns = {op: (make(name), getattr(fe, "shl_gref_" + name)) for op, name in ids.items()}

        def op_map(op, dtype):
            if op not in fns:
                return None
            if op not in self.table:
                cb = pkg.Callback()
                cb.exec = C.cast(fns[op][0], C.c_void_p).value
                cb.est = C.cast(fns[op][1], C.c_void_p).value
                self.table[op] = cb
            return C.addressof(self.table[op])
        self.map_fn = C.CFUNCTYPE(C.c_void_p, C.c_int, C.c_int)(op_map)
        self.rt_fn = C.CFUNCTYPE(C.c_void_p, C.c_int)(lambda op: fe.shl_gref_runtime_callback(op))
        KEEP_ALIVE.append((self, fns))
        fe.shl_register_op_callback(FAKE_API, C.cast(self.map_fn, C.c_void_p))
        fe.shl_register_runtime_callback(FAKE_API, C.cast(self.rt_fn, C.c_void_p))


def test_the_front_end_records_the_four_ops_and_the_host_path_runs_them(built):
    """graph mode: csinn_pad / _reshape / _transpose / _flatten land in their shl_gref_* entries, each appending one layer
    with one input and one output; the stand-in executor's host path then runs them in order.
    data [1,4,4,6] -> pad (H, W by 0 / 1) [1,5,5,6] -> reshape [1,25,2,3] -> transpose (0,2,1,3) [1,2,25,3] -> flatten [1,150]"""
    fe = pkg.load_frontend("standalone")
    back = HostBackend(fe)
    keep = pkg.Keep()
    sess = fe.csinn_alloc_session()
    sc = sess.contents
    sc.base_api, sc.base_run_mode, sc.base_dtype = FAKE_API, pkg.RM_CPU_GRAPH, pkg.DTYPE_INT8
    sc.base_quant_type = pkg.QUANT_INT8_ASYM_W_SYM
    fe.csinn_session_init(sess)
    fe.csinn_set_input_number(1, sess)
    fe.csinn_set_output_number(1, sess)
    recs = [mc.RECORDS["both"][1], mc.RECORDS["both"][0], mc.RECORDS["eq"][0], mc.RECORDS["zp"][1], mc.RECORDS["scale"][1]]
    shapes = [(1, 4, 4, 6), (1, 5, 5, 6), (1, 25, 2, 3), (1, 2, 25, 3), (1, 150)]
    T = lambda shape, q, name: pkg.make_tensor(fe, keep, shape, pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, scales=(q[0],), zps=(q[1],),
                                               name=name, sess=sess)
    ts = [T(s, q, b"t%d" % i) for i, (s, q) in enumerate(zip(shapes, recs))]
    steps = [dict(op="pad", before=[0, 0, 0, 0], after=[0, 1, 1, 0], value=-1.5), dict(op="reshape"),
             dict(op="transpose", perm=(0, 2, 1, 3)), dict(op="flatten")]
    params = []
    for i, step in enumerate(steps):
        case = dict(step, layout="NHWC", out_shape=shapes[i + 1])
        params.append(mc.op_params(fe, keep, FAKE_API, case, sess))
        assert getattr(fe, "csinn_%s_init" % step["op"])(ts[i], ts[i + 1], params[-1]) == pkg.CSINN_TRUE
    fe.csinn_set_tensor_entry(ts[0], sess)
    fe.csinn_set_input(0, ts[0], sess)
    for i, step in enumerate(steps):
        assert getattr(fe, "csinn_" + step["op"])(ts[i], ts[i + 1], params[i]) == pkg.CSINN_TRUE
    assert back.log == []  # recorded, not run
    ids = [pkg.OP_PAD, pkg.OP_RESHAPE, pkg.OP_TRANSPOSE, pkg.OP_FLATTEN]
    for i, op in enumerate(ids):
        node = C.cast(ts[i + 1].contents.data, C.POINTER(Node)).contents
        layer = node.in_[0].contents
        assert (layer.type, layer.in_num, layer.out_num) == (op, 1, 1)
        assert C.addressof(layer.in_[0].contents) == ts[i].contents.data
    fe.csinn_set_output(0, ts[-1], sess)
    assert fe.csinn_session_setup(sess) == pkg.CSINN_TRUE
    x = mc._data("host graph", "int8", shapes[0])
    want = x
    for i, step in enumerate(steps):
        want = mc.move_numpy(dict(step, dtype="int8", in_q=recs[i], out_q=recs[i + 1], out_shape=shapes[i + 1]), want)
    for _ in range(2):
        fe.csinn_update_input(0, pkg.make_tensor(fe, keep, x.shape, pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, data=x, sess=sess), sess)
        assert fe.csinn_session_run(sess) == pkg.CSINN_TRUE
        got = pkg.make_tensor(fe, keep, (1,), pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, sess=sess)
        fe.csinn_get_output(0, got, sess)
        data = np.ctypeslib.as_array(C.cast(got.contents.data, C.POINTER(C.c_int8)), (want.size,)).copy()
        fe.shl_mem_free(got.contents.data)
        assert np.array_equal(data.reshape(want.shape), want)
    assert back.log == ["pad", "reshape", "transpose", "flatten"] * 2
    fe.csinn_session_deinit(sess)
    fe.csinn_free_session(sess)


# ------------------------------------------------------------------------------------ canonicalisation, kernel-form rules
def test_canonicalisation():
    assert mc.canonical((2, 3, 4, 5), (0, 1, 2, 3)) == [(120, 1)]                  # the identity: one dim
    assert mc.canonical((1, 1, 7, 3), (3, 1, 2, 0)) == [(3, 1), (7, 3)]            # unit dims dropped
    assert mc.canonical((1, 3, 8, 4, 4), (0, 1, 3, 4, 2)) == [(3, 128), (16, 1), (8, 16)]  # H and W merge
    assert mc.canonical((2, 5, 4, 16), (0, 2, 1, 3)) == [(2, 320), (4, 16), (5, 64), (16, 1)]
    assert mc.canonical((2, 3, 5, 7), (0, 2, 3, 1)) == [(2, 105), (35, 1), (3, 35)]
    assert mc.canonical((1, 64, 8, 8), (0, 2, 3, 1)) == [(64, 1), (64, 64)]        # a batch of 1 leaves a plain 2-d transpose
    assert len(mc.canonical((2,) * 8, (7, 6, 5, 4, 3, 2, 1, 0))) == 8
    assert mc.canonical((1, 1), (1, 0)) == [(1, 1)]


def _name(hip, case, skew_in=0, skew_out=0):
    """made-up, aligned, disjoint addresses: nothing is dereferenced"""
    return mc.cabi_args(case).name(hip, (1 << 40) + skew_in, (1 << 41) + skew_out)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_name_picks_the_expected_form_and_honours_the_switch(built, case, monkeypatch):
    """pure host code: no device is initialised, no pointer is followed"""
    env = mc.FORM_ENV[case["op"]]
    monkeypatch.delenv(env, raising=False)
    hip = pkg.load_hip()
    natural = mc.expected_form(case)
    assert _name(hip, case) == natural
    for force in mc.FORCES[case["op"]]:
        monkeypatch.setenv(env, force)
        assert _name(hip, case) == mc.expected_form(case, force=force), force
    monkeypatch.setenv(env, "no such form")
    assert _name(hip, case) == natural  # only the forms' names mean anything
    monkeypatch.delenv(env)
    es = case["x"].itemsize
    for skew, align in ((4, 4), (es, es), (16, 16)):
        assert _name(hip, case, skew_in=skew) == mc.expected_form(case, align_in=align)
        assert _name(hip, case, skew_out=skew) == mc.expected_form(case, align_out=align)


def test_every_form_is_exercised():
    seen = {(mc.expected_form(c), c["dtype"]) for c in CASES}
    for form in ("transpose_flat", "transpose_rows_16", "transpose_rows_4", "transpose_tile_4", "transpose_tile_4_1",
                 "transpose_tile_1_4", "transpose_tile_1", "transpose_generic", "pad_vec", "pad_generic"):
        for dtype in ("int8", "f16"):
            assert (form, dtype) in seen, (form, dtype)
    # edge tiles both ways, several tiles, batch dims up to six
    assert any(c["op"] == "transpose" and len(mc.canonical(c["x"].shape, c["perm"])) == 8 for c in CASES)


def test_the_shapes_of_real_models_take_the_fast_forms(built, monkeypatch):
    monkeypatch.delenv("SHL_MI355X_TRANSPOSE_FORM", raising=False)
    monkeypatch.delenv("SHL_MI355X_PAD_FORM", raising=False)
    hip = pkg.load_hip()

    def tr(shape, perm, dtype="int8"):
        x = np.lib.stride_tricks.as_strided(np.zeros(1, np.int8 if dtype == "int8" else np.float16), shape, (0,) * len(shape))
        return _name(hip, dict(op="transpose", x=x, perm=perm, dtype=dtype, in_q=(0.0625, 0), out_q=(0.0625, 0)))
    for c, hw in ((256, 56), (512, 28), (1024, 14)):  # ResNet-50's maps, NCHW <-> NHWC
        assert tr((128, c, hw, hw), (0, 2, 3, 1)) == "transpose_tile_4" and tr((128, hw, hw, c), (0, 3, 1, 2)) == "transpose_tile_4"
    for dtype in ("int8", "f16"):  # one ragged side: 49-element planes against 2048 channels, 85 values against 400 pixels
        assert tr((128, 2048, 7, 7), (0, 2, 3, 1), dtype) == "transpose_tile_1_4"
        assert tr((128, 7, 7, 2048), (0, 3, 1, 2), dtype) == "transpose_tile_4_1"
        assert tr((128, 3, 85, 20, 20), (0, 1, 3, 4, 2), dtype) == "transpose_tile_4_1"
    assert tr((128, 197, 12, 64), (0, 2, 1, 3)) == "transpose_rows_16"  # an attention block's head merge
    for dtype in ("int8", "f16"):  # TensorFlow's SAME pad of MobileNetV1's stride-2 layers: NHWC, H and W only
        for c, hw in ((32, 112), (64, 112), (128, 56), (256, 28), (512, 14)):
            x = np.lib.stride_tricks.as_strided(np.zeros(1, np.int8 if dtype == "int8" else np.float16), (128, hw, hw, c), (0,) * 4)
            case = dict(op="pad", x=x, before=[0, 0, 0, 0], after=[0, 1, 1, 0], value=0.0, dtype=dtype, in_q=(0.0625, 0), out_q=(0.0625, 0))
            assert _name(hip, case) == "pad_vec"
    x = np.lib.stride_tricks.as_strided(np.zeros(1, np.int8), (128, 1, 1, 1024), (0,) * 4)
    assert _name(hip, dict(op="flatten", x=x, dtype="int8", in_q=(0.0625, 0), out_q=(0.0625, 0))) == "transpose_flat"


def test_pad_element_is_the_references_conversion(built):
    hip = pkg.load_hip()

    def element(dtype, value, q=(1.0, 0)):
        d = pkg.PadDesc()
        d.dtype, d.pad_value = dtype, value
        d.out_scale, d.out_zp = q
        return hip.shl_mi355x_pad_element(C.byref(d))
    for v in (0.0, -0.0, -1.5, 1000.0, -1000.0, 0.3, 2.5, 3.5, -2.5, 1e-3):
        for q in mc.RECORDS.values():
            if abs(v / q[1][0]) < 2 ** 20:
                want = int(mc.pool_cases.requantise(np.array([v], np.float32), "int8", q[1])[0])
                assert element(pkg.SHL_I8, v, q[1]) == want & 0xFF, (v, q[1])
    for v in (0.0, -0.0, -1.5, 65504.0, 65519.0, 65520.0, 70000.0, -70000.0, np.inf, -np.inf, 1e-7, 6e-8, 5.96e-8, 2.98e-8, 1.0009765625,
              1.00048828125, 0.1):
        want = int(mc.pool_cases.f32_to_f16_ref(np.array([v], np.float32))[0])
        assert element(pkg.SHL_F16, v) == want, v
    assert element(pkg.SHL_F16, -np.inf) == 0xFBFF
    assert element(pkg.SHL_F16, np.nan) in (0x7FFF, 0xFFFF)


def test_invalid_arguments_are_refused_before_touching_the_device(built):
    hip = pkg.load_hip()
    x = np.arange(96, dtype=np.int8)
    out = np.full(256, POISON, np.uint8)
    xin, o = x.ctypes.data, out.ctypes.data
    q = (0.0625, -5)
    tr = dict(op="transpose", x=x.reshape(2, 3, 16), perm=(1, 0, 2), dtype="int8", in_q=q, out_q=q)
    pad = dict(op="pad", x=x.reshape(1, 2, 3, 16), before=[0, 1, 1, 0], after=[0, 1, 1, 0], value=0.0, dtype="int8", in_q=q, out_q=q)
    flat = dict(op="reshape", x=x, dtype="int8", in_q=q, out_q=q)

    def refused(args, in_ptr, out_ptr, text):
        rc = args.run(hip, in_ptr, out_ptr)
        assert rc == EINVAL, (text, rc)
        assert text.encode() in hip.shl_mi355x_last_error(), (text, hip.shl_mi355x_last_error())
        assert args.name(hip, in_ptr, out_ptr) == ""
    for case in (tr, pad, flat):
        ok = mc.cabi_args(case)
        assert ok.name(hip, xin, o) != ""
        refused(ok, None, o, "NULL argument")
        refused(ok, xin, None, "NULL argument")
        refused(ok, xin, xin, "overlaps the input")
        refused(ok, xin, xin + 95, "overlaps the input")
        assert ok.name(hip, xin, xin + 96) != ""  # ... while an output that begins where the input ends is fine
        bad = mc.cabi_args(case)
        bad.desc.dtype = 2
        refused(bad, xin, o, "dtype")
    assert hip.shl_mi355x_transpose(xin, o, None, None) == EINVAL and hip.shl_mi355x_pad(xin, o, None, None) == EINVAL
    assert hip.shl_mi355x_move(xin, o, 96, None, None) == EINVAL
    for field, k, value, text in (("perm", 0, 0, "repeated"), ("perm", 2, 3, "out of range"), ("perm", 1, -1, "out of range"),
                                  ("dim", 0, -2, "negative dim")):
        bad = mc.cabi_args(tr)
        getattr(bad.desc, field)[k] = value
        refused(bad, xin, o, text)
    for rank in (0, -1, 9):
        bad = mc.cabi_args(tr)
        bad.desc.rank = rank
        refused(bad, xin, o, "rank")
    for field, k, text in (("before", 1, "negative pad"), ("after", 3, "negative pad"), ("dim", 2, "negative dim")):
        bad = mc.cabi_args(pad)
        getattr(bad.desc, field)[k] = -1
        refused(bad, xin, o, text)
    bad = mc.cabi_args(flat)
    bad.elems = -1
    refused(bad, xin, o, "element count")
    assert np.all(out == POISON) and np.array_equal(x, np.arange(96, dtype=np.int8))


REFUSED_LAYERS = [
    # (what, case key, overrides of mc.layer_run)
    ("permute_num != dim_count", "transpose.2x3x5x7_to_nhwc_i8_both", dict(permute_num=3)),
    ("permute_num larger than dim_count", "transpose.2x3x5x7_to_nhwc_i8_both", dict(permute_num=5)),
    ("a repeated permutation entry", "transpose.2x3x5x7_to_nhwc_i8_both", dict(perm=(0, 2, 2, 1))),
    ("a permutation entry out of range", "transpose.2x3x5x7_to_nhwc_i8_both", dict(perm=(0, 2, 4, 1))),
    ("a negative permutation entry", "transpose.2x3x5x7_to_nhwc_i8_both", dict(perm=(0, 2, -1, 1))),
    ("output dims that are not the permuted input dims", "transpose.2x3x5x7_to_nhwc_i8_both", dict(out_shape=(2, 5, 3, 7))),
    ("an output of another rank", "transpose.2x3x5x7_to_nhwc_i8_both", dict(out_shape=(2, 5, 21))),
    ("transpose: per-channel quantised input", "transpose.2x3x5x7_to_nhwc_i8_both", dict(in_scales=(0.5, 0.25))),
    ("transpose: an output of another dtype", "transpose.2x3x5x7_to_nhwc_i8_both", dict(out_dt=pkg.DTYPE_FLOAT32)),
    ("CSINN_PAD_EDGE", "pad.hw_11_nhwc_i8_both", dict(mode=pkg.PAD_EDGE)),
    ("CSINN_PAD_REFLECT", "pad.hw_11_nchw_f16", dict(mode=pkg.PAD_REFLECT)),
    ("pad_num 3", "pad.hw_11_nhwc_i8_both", dict(pad_num=3)),
    ("pad_num 5", "pad.hw_11_nhwc_i8_both", dict(pad_num=5)),
    ("a negative pad", "pad.hw_11_nhwc_i8_both", dict(before=[0, -1, 1, 0], out_shape=(1, 5, 7, 3))),
    ("a negative pad behind", "pad.hw_11_nhwc_i8_both", dict(after=[0, 1, -1, 0], out_shape=(1, 7, 5, 3))),
    ("output dims that are not input + before + after", "pad.hw_11_nhwc_i8_both", dict(out_shape=(1, 7, 6, 3))),
    ("an output with more channels", "pad.hw_11_nhwc_i8_both", dict(out_shape=(1, 7, 7, 4))),
    ("another layout", "pad.hw_11_nhwc_i8_both", dict(layout=pkg.LAYOUT_NC)),
    ("pad: per-channel quantised input", "pad.hw_11_nhwc_i8_both", dict(in_scales=(0.5,) * 3)),
    ("reshape into fewer elements", "reshape.2x1x1x24_i8_eq", dict(out_shape=(2, 23))),
    ("reshape into more elements", "reshape.2x1x1x24_i8_eq", dict(out_shape=(2, 25))),
    ("flatten into fewer elements", "flatten.2x1x1x24_i8_eq", dict(out_shape=(47,))),
    ("flatten into more elements", "flatten.2x1x1x24_f16", dict(out_shape=(7, 7))),
    ("reshape: an output of another dtype", "reshape.2x1x1x24_i8_eq", dict(out_dt=pkg.DTYPE_FLOAT32)),
]


@pytest.mark.parametrize("what,key,kw", REFUSED_LAYERS, ids=[r[0] for r in REFUSED_LAYERS])
def test_refused_layers_fail_in_the_callback_and_write_nothing(standalone, what, key, kw):
    """where the reference would read or write past a buffer or hit an assert; refused before anything is staged, so no
    device is needed"""
    fe, _, _ = standalone
    rc, out = mc.layer_run(fe, pkg.API_MI355X, BY_KEY[key], poison=POISON, **kw)
    assert rc != pkg.CSINN_TRUE, what
    assert np.all(out.view(np.uint8) == POISON), what


def test_pad_of_a_tensor_that_is_not_4d_is_refused(standalone):
    fe, _, _ = standalone
    case = dict(op="pad", name="3d", dtype="int8", layout="NHWC", in_q=mc.Q_SAME, out_q=mc.Q_SAME, x=np.zeros((2, 3, 16), np.int8),
                before=[0, 1, 0], after=[0, 1, 0], value=0.0, out_shape=(2, 5, 16))
    rc, out = mc.layer_run(fe, pkg.API_MI355X, case, poison=POISON)
    assert rc != pkg.CSINN_TRUE and np.all(out.view(np.uint8) == POISON)


def test_perf_callbacks_name_the_kernel_form(standalone, monkeypatch):
    """init accepts the layer from dims, dtypes and records alone; perf reports the form the rules choose for host tensors,
    which the staging path aligns"""
    fe, hip, opt = standalone
    for env in set(mc.FORM_ENV.values()):
        monkeypatch.delenv(env, raising=False)
    opt.shl_cb_map_mi355x.restype = C.POINTER(pkg.Callback)
    opt.shl_cb_map_mi355x.argtypes = [C.c_int, C.c_int]
    for op in (pkg.OP_TRANSPOSE, pkg.OP_RESHAPE, pkg.OP_FLATTEN, pkg.OP_PAD):
        for dt in (pkg.DTYPE_INT8, pkg.DTYPE_FLOAT16):
            cb = opt.shl_cb_map_mi355x(op, dt)
            assert cb and cb.contents.perf and cb.contents.exec and cb.contents.est and cb.contents.init
    seen = []

    def perf(cb, t_in, t_out, params):
        name = C.c_char_p()
        fn = C.CFUNCTYPE(C.c_int, TP, TP, C.c_void_p, C.POINTER(C.c_char_p))(cb.contents.perf)
        assert fn(t_in, t_out, params, C.byref(name)) == pkg.CSINN_TRUE
        seen.append(name.value.decode())
        raise StopIteration  # nothing is executed: no device is needed
    for case in CASES:
        with pytest.raises(StopIteration):
            mc.layer_run(fe, pkg.API_MI355X, case, perf=perf)
        assert seen[-1] == mc.expected_form(case), mc.case_id(case)
    monkeypatch.setenv("SHL_MI355X_TRANSPOSE_FORM", "generic")
    with pytest.raises(StopIteration):
        mc.layer_run(fe, pkg.API_MI355X, BY_KEY["transpose.64x64_f16"], perf=perf)
    assert seen[-1] == "transpose_generic"


FALL_THROUGH = r"""
import sys
sys.path.insert(0, %(tests)r)
import ctypes as C
import numpy as np
import cases, move_cases as mc
from cases import pkg
fe = cases.load_reference_frontend()          # genuine libshl_ref_x86.so
hip, opt = pkg.load_backend(fe)
fe.shl_cb_map_ref.restype = C.POINTER(pkg.Callback)
fe.shl_cb_map_ref.argtypes = [C.c_int, C.c_int]
opt.shl_cb_map_mi355x.restype = C.POINTER(pkg.Callback)
opt.shl_cb_map_mi355x.argtypes = [C.c_int, C.c_int]
by_key = {mc.golden_key(c): c for c in mc.all_cases()}
ops = {"transpose": pkg.OP_TRANSPOSE, "reshape": pkg.OP_RESHAPE, "flatten": pkg.OP_FLATTEN, "pad": pkg.OP_PAD}
bad = 0
def probe(key, want_ref, **kw):
    global bad
    case = by_key[key]
    seen = []
    def perf(cb, *args):
        seen.append(cb.contents.exec)
        raise StopIteration
    try:
        mc.layer_run(fe, pkg.API_MI355X, case, perf=perf, **kw)
    except StopIteration:
        pass
    dt = pkg.DTYPE_INT8 if case["dtype"] == "int8" else pkg.DTYPE_FLOAT16
    ref = fe.shl_cb_map_ref(ops[case["op"]], dt).contents.exec
    own = opt.shl_cb_map_mi355x(ops[case["op"]], dt).contents.exec
    ok = seen == [ref if want_ref else own] and ref != own
    print(key, kw, "reference" if want_ref else "backend", "ok" if ok else "WRONG")
    bad += int(not ok)
probe("transpose.2x3x5x7_to_nhwc_i8_both", False)
probe("transpose.2x3x5x7_to_nhwc_i8_both", True, permute_num=3)
probe("transpose.2x3x5x7_to_nhwc_i8_both", True, perm=(0, 2, 2, 1))
probe("transpose.2x3x5x7_to_nhwc_i8_both", True, out_shape=(2, 5, 3, 7))
probe("pad.hw_11_nhwc_i8_both", False)
probe("pad.hw_11_nhwc_i8_both", True, mode=pkg.PAD_EDGE)
probe("pad.hw_11_nhwc_i8_both", True, pad_num=3)
probe("pad.hw_11_nhwc_i8_both", True, out_shape=(1, 7, 6, 3))
probe("pad.hw_11_nhwc_i8_both", True, before=[0, -1, 1, 0], out_shape=(1, 5, 7, 3))
probe("reshape.2x1x1x24_i8_eq", False)
probe("reshape.2x1x1x24_i8_eq", True, out_shape=(2, 23))
probe("flatten.2x1x1x24_f16", False)
probe("flatten.2x1x1x24_f16", True, out_shape=(7, 7))
print("FALLTHROUGH_OK" if bad == 0 else "FALLTHROUGH_FAIL")
"""


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_a_refused_layer_is_handed_to_the_reference_at_init(built):
    """next to the genuine library init swaps the reference's exec into the layer's callback block; an accepted layer keeps
    the backend's.  Nothing is executed (the refused layers are ones the reference itself would run off a buffer with)."""
    code = FALL_THROUGH % dict(tests=HERE)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert "FALLTHROUGH_OK" in res.stdout, res.stdout + res.stderr


# ------------------------------------------------------------------------------------ the host code under sanitizers
DRIVER = r"""
// Stand-alone driver of the host code of csrc/transpose.hip, csrc/pad.hip and source/mi355x_opt/move.c: reads one problem per
// line, prints the kernel form (and the pad element).  Nothing is launched: the staging functions below are never reached.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <hip/hip_runtime.h>
extern "C" {
#include "mi355x_internal.h"
}
namespace shl {
bool requant_is_identity(float, int32_t) { return false; }
void set_error(const char *, ...) {}
int hip_fail(hipError_t, const char *) { return SHL_MI355X_EINVAL; }
}  // namespace shl
extern "C" {
void shl_debug_error(const char *, ...) {}
const char *shl_mi355x_last_error(void) { return ""; }
int csinn_tensor_size(struct csinn_tensor *t)
{
    int n = t->dim_count ? 1 : 0;
    for (int k = 0; k < t->dim_count; k++) n *= t->dim[k];
    return n;
}
int csinn_tensor_byte_size(struct csinn_tensor *t) { return csinn_tensor_size(t) * (t->dtype == CSINN_DTYPE_FLOAT16 ? 2 : 1); }
struct shl_mi355x_ctx *shl_mi355x_ctx_of(struct csinn_session *) { abort(); }
void *shl_mi355x_ctx_stream(struct shl_mi355x_ctx *) { abort(); }
const void *shl_mi355x_stage_in(struct shl_mi355x_ctx *, struct csinn_tensor *, int) { abort(); }
void *shl_mi355x_stage_out_begin(struct shl_mi355x_ctx *, struct csinn_tensor *, int) { abort(); }
int shl_mi355x_stage_out_end(struct shl_mi355x_ctx *, struct csinn_tensor *, void *) { abort(); }
}

static void tensor(struct csinn_tensor *t, struct csinn_quant_info *q, int dtype, int layout, int rank, const int *dims, float s, int zp)
{
    memset(t, 0, sizeof(*t)), memset(q, 0, sizeof(*q));
    t->dtype = (enum csinn_dtype_enum)dtype, t->layout = layout, t->dim_count = rank, t->quant_channel = 1, t->qinfo = q;
    for (int k = 0; k < rank; k++) t->dim[k] = dims[k];
    q->scale = s, q->zero_point = zp;
}

int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char op[16];
    // <op> <dtype: 0 int8, 1 binary16> <layout> <in scale> <in zp> <out scale> <out zp> <rank> <dims> <out rank> <out dims> ...
    while (fscanf(f, "%15s", op) == 1) {
        int dt, layout, zi, zo, rank, orank, dim[8], odim[8], n = 0, mode = 0;
        float si, so, value = 0.0f;
        if (fscanf(f, "%d %d %f %d %f %d %d", &dt, &layout, &si, &zi, &so, &zo, &rank) != 7) return 3;
        for (int k = 0; k < rank; k++) if (fscanf(f, "%d", &dim[k]) != 1) return 3;
        if (fscanf(f, "%d", &orank) != 1) return 3;
        for (int k = 0; k < orank; k++) if (fscanf(f, "%d", &odim[k]) != 1) return 3;
        struct csinn_tensor in, out;
        struct csinn_quant_info qi, qo;
        const int cdt = dt ? CSINN_DTYPE_FLOAT16 : CSINN_DTYPE_INT8;
        tensor(&in, &qi, cdt, layout, rank, dim, si, zi), tensor(&out, &qo, cdt, layout, orank, odim, so, zo);
        struct csinn_perf_info info;
        memset(&info, 0, sizeof(info));
        struct csinn_callback cb;
        memset(&cb, 0, sizeof(cb));
        const void *pi = (const void *)((uintptr_t)1 << 40), *po = (const void *)((uintptr_t)1 << 41);
        int rc = 0;
        const char *direct = "";
        unsigned element = 0;
        if (strcmp(op, "transpose") == 0) {
            if (fscanf(f, "%d", &n) != 1) return 3;
            int *perm = (int *)malloc(sizeof(int) * (n > 0 ? n : 1));  // exactly as long as it says: reads past it are caught
            for (int k = 0; k < n; k++) if (fscanf(f, "%d", &perm[k]) != 1) return 3;
            struct csinn_transpose_params p;
            memset(&p, 0, sizeof(p));
            p.base.cb = &cb, p.base.layout = layout, p.permute = perm, p.permute_num = n;
            shl_mi355x_transpose_init(&in, &out, &p);
            rc = shl_mi355x_transpose_perf(&in, &out, &p, &info);
            if (rc == CSINN_TRUE) {
                struct shl_mi355x_transpose_desc d;
                memset(&d, 0, sizeof(d));
                d.dtype = dt, d.rank = rank, d.in_scale = si, d.in_zp = zi, d.out_scale = so, d.out_zp = zo;
                for (int k = 0; k < rank; k++) d.dim[k] = dim[k], d.perm[k] = perm[k];
                direct = shl_mi355x_transpose_kernel_name(pi, po, &d);
            }
            free(perm);
        } else if (strcmp(op, "pad") == 0) {
            if (fscanf(f, "%d %d %f", &n, &mode, &value) != 3) return 3;
            int *before = (int *)malloc(sizeof(int) * (n > 0 ? n : 1)), *after = (int *)malloc(sizeof(int) * (n > 0 ? n : 1));
            for (int k = 0; k < n; k++) if (fscanf(f, "%d", &before[k]) != 1) return 3;
            for (int k = 0; k < n; k++) if (fscanf(f, "%d", &after[k]) != 1) return 3;
            struct csinn_pad_params p;
            memset(&p, 0, sizeof(p));
            p.base.cb = &cb, p.base.layout = layout, p.pad_before = before, p.pad_after = after, p.pad_num = n;
            p.pad_value = value, p.pad_mode = (enum csinn_pad_enum)mode;
            shl_mi355x_pad_init(&in, &out, &p);
            rc = shl_mi355x_pad_perf(&in, &out, &p, &info);
            if (rc == CSINN_TRUE) {
                struct shl_mi355x_pad_desc d;
                memset(&d, 0, sizeof(d));
                d.dtype = dt, d.pad_value = value, d.in_scale = si, d.in_zp = zi, d.out_scale = so, d.out_zp = zo;
                for (int k = 0; k < 4; k++) d.dim[k] = dim[k], d.before[k] = before[k], d.after[k] = after[k];
                direct = shl_mi355x_pad_kernel_name(pi, po, &d);
                element = shl_mi355x_pad_element(&d);
            }
            free(before), free(after);
        } else {
            struct shl_mi355x_move_desc d;
            memset(&d, 0, sizeof(d));
            d.dtype = dt, d.in_scale = si, d.in_zp = zi, d.out_scale = so, d.out_zp = zo;
            if (strcmp(op, "reshape") == 0) {
                struct csinn_reshape_params p;
                memset(&p, 0, sizeof(p));
                p.base.cb = &cb, p.base.layout = layout;
                shl_mi355x_reshape_init(&in, &out, &p);
                rc = shl_mi355x_reshape_perf(&in, &out, &p, &info);
            } else {
                struct csinn_flatten_params p;
                memset(&p, 0, sizeof(p));
                p.base.cb = &cb, p.base.layout = layout;
                shl_mi355x_flatten_init(&in, &out, &p);
                rc = shl_mi355x_flatten_perf(&in, &out, &p, &info);
            }
            if (rc == CSINN_TRUE) direct = shl_mi355x_move_kernel_name(pi, po, csinn_tensor_size(&in), &d);
        }
        printf("%s %d %s %s %u\n", op, rc, rc == CSINN_TRUE && info.kernel_name ? info.kernel_name : "-", *direct ? direct : "-", element);
    }
    fclose(f);
    return 0;
}
"""


def _line(case, **kw):
    x = case["x"]
    dt = 0 if case["dtype"] == "int8" else 1
    layout = kw.get("layout", pkg.LAYOUT_NHWC if case["layout"] == "NHWC" else pkg.LAYOUT_NCHW)
    oshape = kw.get("out_shape", case["out_shape"])
    words = [case["op"], dt, layout, repr(float(case["in_q"][0])), case["in_q"][1], repr(float(case["out_q"][0])), case["out_q"][1],
             x.ndim, *x.shape, len(oshape), *oshape]
    if case["op"] == "transpose":
        perm = list(kw.get("perm", case["perm"]))
        n = kw.get("permute_num", len(perm))
        words += [n, *(perm + [0] * n)[:n]]  # (the array is exactly as long as permute_num says)
    elif case["op"] == "pad":
        before, after = list(kw.get("before", case["before"])), list(kw.get("after", case["after"]))
        n = kw.get("pad_num", len(before))
        value = case["value"]
        words += [n, kw.get("mode", 0), "inf" if value == np.inf else "-inf" if value == -np.inf else repr(float(value)),
                  *(before + [0] * n)[:n], *(after + [0] * n)[:n]]
    return " ".join(str(w) for w in words)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc to compile with")
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on machines without a GPU")
def test_descriptor_code_runs_clean_under_address_and_undefined_sanitizers(built, tmp_path):
    """csrc/transpose.hip, csrc/pad.hip (host side: -Xarch_host) and source/mi355x_opt/move.c and layer.c compiled with
    -fsanitize=address,undefined into a program of their own, which takes every case's and every refused layer's descriptor
    apart -- init, perf, canonicalisation, form choice, pad element -- and must name the same forms the library does."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    root = cases.ROOT
    inc = os.path.join(root, "include")
    csrc = os.path.join(root, "csi-nn2_amd", "csrc")
    opt_dir = os.path.join(root, "csi-nn2_amd", "source", "mi355x_opt")
    san = "-fsanitize=address,undefined"
    (tmp_path / "driver.cpp").write_text(DRIVER)
    incs = ["-I" + inc, "-I" + os.path.join(inc, "csinn"), "-I" + csrc, "-I" + opt_dir]
    for name in ("move", "layer"):
        subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", san, "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-c",
                        os.path.join(opt_dir, name + ".c"), "-o", str(tmp_path / (name + ".o"))] + incs, check=True)
    hip_flags = ["--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-gpu-rdc", "-ffp-contract=off", "-Xarch_host", san,
                 "-Xarch_host", "-fno-sanitize-recover=undefined"]
    for name in ("transpose", "pad"):
        subprocess.run([hipcc] + hip_flags + incs + ["-c", os.path.join(csrc, name + ".hip"), "-o", str(tmp_path / (name + ".o"))],
                       check=True)
    subprocess.run([hipcc] + hip_flags + incs + ["-x", "hip", "-c", str(tmp_path / "driver.cpp"), "-o", str(tmp_path / "driver.o")],
                   check=True)
    exe = str(tmp_path / "move_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fno-gpu-rdc", san] + [str(tmp_path / (n + ".o")) for n in ("driver", "transpose", "pad", "move", "layer")]
                   + ["-o", exe], check=True)
    lines = [_line(c) for c in CASES]
    refused = [_line(BY_KEY[key], **kw) for _, key, kw in REFUSED_LAYERS if "in_scales" not in kw and "out_dt" not in kw]
    (tmp_path / "problems.txt").write_text("\n".join(lines + refused) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for force_t, force_p in ((None, None), ("generic", "generic"), ("tile", None), ("rows", None)):
        e = dict(env)
        e.pop("SHL_MI355X_TRANSPOSE_FORM", None), e.pop("SHL_MI355X_PAD_FORM", None)
        if force_t:
            e["SHL_MI355X_TRANSPOSE_FORM"] = force_t
        if force_p:
            e["SHL_MI355X_PAD_FORM"] = force_p
        res = subprocess.run([exe, str(tmp_path / "problems.txt")], capture_output=True, text=True, env=e, timeout=120)
        assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
        rows = [ln.split() for ln in res.stdout.splitlines()]
        assert len(rows) == len(lines) + len(refused)
        for case, row in zip(CASES, rows):
            force = force_p if case["op"] == "pad" else force_t
            want = mc.expected_form(case, force=force)
            assert row[:4] == [case["op"], str(pkg.CSINN_TRUE), want, want], (mc.case_id(case), force, row)
            if case["op"] == "pad":
                if any(case["before"]):  # the output's first element is padding: the genuine library's pad element
                    corner = int(GOLD[mc.golden_key(case)].reshape(-1)[0])
                    assert int(row[4]) == corner & (0xFF if case["dtype"] == "int8" else 0xFFFF), mc.case_id(case)
        for row in rows[len(lines):]:
            assert int(row[1]) != pkg.CSINN_TRUE and row[2] == "-", row


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
@pytest.mark.parametrize("dtype,layout", [("int8", "NHWC"), ("f16", "NCHW")])
@pytest.mark.parametrize("net", sorted(mc.NETS))
def test_oracle_chains_equal_the_genuine_graph_executor(net, dtype, layout):
    """the yardstick of tests/test_move_session.py: the networks through the genuine front-end, graph executor and C kernels
    (CSINN_REF) give the oracle chain's answer: int8 bit for bit, binary16 within the project's 1e-3"""
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)
    g = mc.NETS[net](dtype, layout)
    g.build(fe, pkg.API_REF)
    for k in (0, 1):
        x = g.input(k)
        got, want = g.run(fe, x), g.oracle(x)
        for name in g.outputs:
            what = "%s %s %s input %d, output %s" % (net, dtype, layout, k, name)
            if dtype == "int8":
                mc.assert_same(got[name], want[name], what)
            else:  # the C oracle's binary16 convolution sums in another order than the library's: the project's 1e-3
                g32, w32 = got[name].astype(np.float32), want[name].astype(np.float32)
                assert np.all(np.abs(g32 - w32) <= 1e-3 * np.maximum(np.abs(w32), 1e-3)), what
    g.close(fe)

"""The reductions without a GPU: the goldens from the genuine library against the numpy restatement (a plain sequential loop),
the crafted rows whose sum depends on its order, op ids and the params block's layout, the exported entry points, the front-end
and the stand-in executor's host path, canonicalisation and the form rule (pure host code), refusals before the device is
touched, and the descriptor code in a stand-alone program under the address and undefined-behaviour sanitizers."""
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
import reduce_cases as rc
from cases import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = rc.all_cases()
IDS = [rc.case_id(c) for c in CASES]
GOLD = rc.golden()
BY_KEY = {rc.golden_key(c): c for c in CASES}
POISON = 0x5A
EINVAL = -2
TP = C.POINTER(pkg.Tensor)
FORM_ENV = "SHL_MI355X_REDUCE_FORM"
OP_IDS = {"mean": 101, "sum": 173, "max": 96, "min": 103, "reduce_mean": 123, "reduce_sum": 126, "reduce_max": 122, "reduce_min": 124,
          "global_maxpool2d": 75}


def test_golden_covers_the_case_list():
    assert sorted(GOLD) == sorted(rc.golden_key(c) for c in CASES)
    for c in CASES:
        assert GOLD[rc.golden_key(c)].size == int(np.prod(rc.out_shape_of(c))), rc.case_id(c)
    path = os.path.join(HERE, "golden", "reduce_cases.npz")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "golden", "move_cases.npz")) // 2  # outputs only, and tiny


def _sizes(c):
    oe, _, ie, _ = rc.descriptor(c)["groups"]
    return int(np.prod(oe, dtype=np.int64)), int(np.prod(ie, dtype=np.int64))


def test_case_list_covers_what_it_must():
    assert {c["op"] for c in CASES} == set(rc.OPS)
    chunk_sizes = {"int8": (255, 256, 257, 515), "f16": (127, 128, 129, 259)}
    for dtype in ("int8", "f16"):
        assert rc.CHUNK[dtype] == chunk_sizes[dtype][1]
        for kind in ("sum", "mean", "max", "min"):
            mine = [c for c in CASES if c["dtype"] == dtype and rc.kind_of(c["op"]) == kind]
            for form in ("reduce_rows", "reduce_cols"):
                inner = {_sizes(c)[1] for c in mine if rc.expected_form(c) == form}
                outs = {_sizes(c)[0] for c in mine if rc.expected_form(c) == form}
                # (an inner size of 1 leaves no inner group and so cannot be `rows`; one output leaves no outer group)
                assert {2, 63, 64, 65, 255, 256, 257} | set(chunk_sizes[dtype]) <= inner, (dtype, kind, form)
                assert {3, 63, 64, 65, 257} <= outs, (dtype, kind, form)
            assert any(_sizes(c)[1] == 1 for c in mine) and any(_sizes(c)[0] == 1 for c in mine)
            assert any(c["name"].startswith("nchw_over_n_h") for c in mine)            # two inner groups that do not merge
            assert any(len(rc.canonical(*rc.descriptor(c)["groups"][:2])) == 3 for c in mine)   # three outer groups
            assert any(c["op"].startswith("reduce_") and c.get("axis") == -1 for c in mine)
            assert {c["axis"] for c in mine if c["name"].startswith("rank4_axis")} == {0, 1, 2, 3}
            assert any(rc.expected_form(c) == "reduce_generic" for c in mine)
        for layout in ("NCHW", "NHWC"):
            maps = {c["name"].split("_")[0] for c in CASES if c["op"] == "global_maxpool2d" and c["layout"] == layout and c["dtype"] == dtype}
            assert {"1x1", "7x7", "5x9"} <= maps
        assert any(_sizes(c) == (1, 1 << 16) for c in CASES if c["dtype"] == dtype)  # the long row
        assert any(c.get("order") and rc.kind_of(c["op"]) == k for c in CASES if c["dtype"] == dtype for k in ("sum", "mean"))
    assert max(c["x"].size for c in CASES) <= 1 << 16
    for c in CASES:
        if c.get("order") and c["dtype"] == "int8":
            assert c["in_q"][0] == float(np.float32(0.1)) and _sizes(c)[1] >= 4096 and (c["x"] > 0).any() and (c["x"] < 0).any()
    zps = {(c["in_q"][1], c["out_q"][1]) for c in CASES if c["dtype"] == "int8"}
    assert {-128, 127} <= {z[0] for z in zps} and {-128, 127} <= {z[1] for z in zps}
    assert any(c["out_q"][0] < 2.0 ** -40 for c in CASES if c["dtype"] == "int8")  # outside div_by_scale's range
    sat = [c for c in CASES if "saturates" in c["name"]]
    assert sat and any({-128, 127} <= set(GOLD[rc.golden_key(c)].ravel().tolist()) for c in sat)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_numpy_restatement_matches_the_reference_golden(case):
    rc.assert_same(rc.reduce_numpy(case), GOLD[rc.golden_key(case)].reshape(rc.out_shape_of(case)), rc.case_id(case))


ORDER_CASES = [c for c in CASES if c.get("order")]


@pytest.mark.parametrize("case", ORDER_CASES, ids=[rc.case_id(c) for c in ORDER_CASES])
def test_the_sum_in_reverse_order_gives_another_output(case):
    """what makes these cases a test of the ORDER: the same restatement walking the inner index backwards changes an output
    (a case where it does not would be replaced, not kept)"""
    forward, backward = rc.bits(rc.reduce_numpy(case)), rc.bits(rc.reduce_numpy(case, reverse=True))
    assert np.any(forward != backward), rc.case_id(case)
    if case["dtype"] == "int8":
        assert not np.all((forward == 127) | (forward == -128)), "the outputs must not all saturate"


def test_binary16_special_rows_give_what_the_documented_rules_say():
    """the goldens of the crafted max / min rows, spelled out: of +0 and -0 the later one stays; a NaN loses; from -FLT_MAX a row
    of NaNs or of -inf gives -65504, from the first element a row of NaNs gives the first NaN's sign"""
    row = lambda key: GOLD[key].ravel()
    mx, mn = row("max.special_rows_f16"), row("min.special_rows_f16")
    assert (mx[0], mx[1], mx[2]) == (0x8000, 0x0000, 0x8000) and (mn[0], mn[1]) == (0x8000, 0x0000)
    assert (mx[3], mx[5], mx[6]) == (0x4200, 0x4200, 0x4200) and (mn[3], mn[6]) == (0xC000, 0xC000)
    assert mx[7] == 0xFBFF and mx[11] == 0xFBFF and mn[7] == 0x7BFF and mn[12] == 0x7BFF  # all NaN / all -inf: -FLT_MAX rounds
    assert mx[13] == 0x7BFF and mn[13] == 0xFBFF                                            # inf saturates like 65504
    first = row("reduce_max.special_last_axis_f16")
    assert (first[7], first[8], first[9], first[10]) == (0x7FFF, 0xFFFF, 0xFFFF, 0x7FFF)  # all NaN: the first one's sign
    assert first[3] == 0x4200 and first[11] == 0xFBFF
    s = row("sum.order_rows_f16")
    assert s[3] == 0x7BFF and s[4] == 0xFFFF and (s[6], s[7]) == (0x7FFF, 0xFFFF) and s[8] == 0xFFFF  # inf; inf - inf; NaN signs
    assert 0 < (s[5] & 0x7FFF) < 0x0400  # the subnormal total


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_numpy_restatement_matches_the_live_reference_and_the_generator_is_reproducible():
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)  # errors only: the library warns about every binary16 saturation
    for case in CASES:
        got = rc.layer_run(fe, pkg.API_REF, case)
        rc.assert_same(rc.reduce_numpy(case), got, rc.case_id(case) + " vs live reference")
        rc.assert_same(got, GOLD[rc.golden_key(case)].reshape(got.shape), rc.case_id(case) + ": live reference vs golden")
    again = rc.all_cases()
    for a, b in zip(CASES, again):
        assert np.array_equal(rc.bits(a["x"]), rc.bits(b["x"])), "inputs are regenerated from seeds"


def _probe():
    spec = importlib.util.spec_from_file_location("make_reduce_golden", os.path.join(HERE, "golden", "make_reduce_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_op_ids_and_the_params_block_match_the_reference():
    want = json.load(open(os.path.join(HERE, "golden", "reduce_op_ids.json")))
    assert {k: v for k, v in want.items() if k.startswith("CSINN_OP_")} == {"CSINN_OP_" + k.upper(): v for k, v in OP_IDS.items()}
    assert want["sizeof csinn_reduce_params"] == 104
    inc = os.path.join(cases.ROOT, "include")
    assert _probe().measure([inc, os.path.join(inc, "csinn")]) == want  # this repository's headers, compiled
    text = open(os.path.join(inc, "csinn", "csinn_data_structure.h")).read()
    for op, value in OP_IDS.items():
        assert int(re.search(r"\bCSINN_OP_%s\s*=\s*(\d+)" % op.upper(), text).group(1)) == value
        assert getattr(pkg, "OP_" + op.upper()) == value
    assert C.sizeof(pkg.ReduceParams) == want["sizeof csinn_reduce_params"]
    for field, _ in pkg.ReduceParams._fields_[1:]:
        assert getattr(pkg.ReduceParams, field).offset == want["offsetof csinn_reduce_params." + field], field


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_libraries_export_the_entry_points(built):
    front = {"csinn_%s%s" % (op, s) for op in rc.OPS for s in ("", "_init")} | {"shl_gref_" + op for op in rc.OPS}
    assert front <= _exports(pkg.lib_path("libcsinn_nn2.so"))
    back = {"shl_mi355x_%s_%s" % (op, s) for op in rc.OPS for s in ("init", "exec", "perf")}
    assert back <= _exports(pkg.lib_path("libshl_mi355x_opt.so"))
    assert {"shl_mi355x_reduce", "shl_mi355x_reduce_kernel_name"} <= _exports(pkg.lib_path("libshl_mi355x.so"))
    assert C.sizeof(pkg.ReduceDesc) == 192 and pkg.ReduceDesc.out_extent.offset == 20 and pkg.ReduceDesc.inner_stride.offset == 116
    assert pkg.ReduceDesc.in_elems.offset == 152 and pkg.ReduceDesc.out_zp.offset == 172


# ------------------------------------------------------------------------------------ front-end and graph executor
FAKE_API = 6  # an unused slot of the dispatch tables
KEEP_ALIVE = []  # the C side keeps the callbacks' addresses


class Node(C.Structure):
    """struct shl_node (include/shl_gref.h)"""


Node._fields_ = [("type", C.c_int), ("in_", C.POINTER(C.POINTER(Node))), ("out", C.POINTER(C.POINTER(Node))),
                 ("subgraph_idx", C.c_int), ("in_num", C.c_int), ("out_num", C.c_int), ("name", C.c_char_p), ("data", C.c_void_p)]


class HostBackend:
    """the nine ops on the host, in numpy, registered in slot FAKE_API: what the graph executor's host path calls; records
    every call"""

    def __init__(self, fe, layout):
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
                case = dict(op=op, dtype="int8", in_q=rec(i), out_q=rec(o), x=x, out_shape=out.shape, layout=layout)
                if op in rc.STRIDE_OPS:  # the groups as the params block holds them
                    pc = C.cast(p, C.POINTER(pkg.ReduceParams)).contents
                    groups = ([pc.out_extents[k] for k in range(pc.n)], [pc.out_strides[k] for k in range(pc.n)],
                              [pc.inner_extents[k] for k in range(pc.m)], [pc.inner_strides[k] for k in range(pc.m)])
                    kept = [k for k in range(x.ndim) if x.shape[k] not in groups[2] or k < 2]
                    case["axes"] = tuple(k for k in range(x.ndim) if k not in kept)
                    assert rc.descriptor(case)["groups"] == groups
                elif op in rc.AXIS_OPS:
                    pc = C.cast(p, C.POINTER(pkg.ReduceParams)).contents
                    assert pc.axis_count == 1
                    case["axis"] = pc.axis[0]
                self.log.append(op)
                out[...] = rc.reduce_numpy(case).reshape(out.shape)
                return 1
            return C.CFUNCTYPE(C.c_int, TP, TP, C.c_void_p)(run)
        fns = {OP_IDS[name]: (make(name), getattr(fe, "shl_gref_" + name)) for name in rc.OPS}

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


def test_the_front_end_records_the_nine_ops_and_the_host_path_runs_them(built):
    """graph mode: each csinn_<op> lands in its shl_gref_* entry and appends one layer with one input and one output; the
    stand-in executor's host path then runs them.  One input [2, 3, 4, 5] (NCHW) feeds all nine: mean / sum / max / min over H
    and W, reduce_* over the channel axis, global_maxpool2d -- nine graph outputs"""
    fe = pkg.load_frontend("standalone")
    back = HostBackend(fe, "NCHW")
    keep = pkg.Keep()
    sess = fe.csinn_alloc_session()
    sc = sess.contents
    sc.base_api, sc.base_run_mode, sc.base_dtype = FAKE_API, pkg.RM_CPU_GRAPH, pkg.DTYPE_INT8
    sc.base_quant_type = pkg.QUANT_INT8_ASYM_W_SYM
    fe.csinn_session_init(sess)
    fe.csinn_set_input_number(1, sess)
    fe.csinn_set_output_number(len(rc.OPS), sess)
    shape = (2, 3, 4, 5)
    q_in = rc.Q_CONV[0]
    T = lambda shape, q, name: pkg.make_tensor(fe, keep, shape, pkg.DTYPE_INT8, pkg.LAYOUT_NCHW, scales=(q[0],), zps=(q[1],),
                                               name=name, sess=sess)
    t_in = T(shape, q_in, b"data")
    layers = []
    for op in rc.OPS:
        case = dict(op=op, dtype="int8", in_q=q_in, x=np.zeros(shape, np.int8), layout="NCHW", axes=(2, 3), axis=1)
        case["out_shape"] = rc._out_shape(case["x"], op, axes=(2, 3), axis=1, layout="NCHW")
        case["out_q"] = rc.out_record(rc.kind_of(op), 20 if op in rc.STRIDE_OPS or op == "global_maxpool2d" else 3, q_in, op)
        t_out = T(case["out_shape"], case["out_q"], op.encode())
        params = rc.op_params(fe, keep, FAKE_API, case, sess)
        assert getattr(fe, "csinn_%s_init" % op)(t_in, t_out, params) == pkg.CSINN_TRUE
        layers.append((op, case, t_out, params))
    fe.csinn_set_tensor_entry(t_in, sess)
    fe.csinn_set_input(0, t_in, sess)
    for op, case, t_out, params in layers:
        assert getattr(fe, "csinn_" + op)(t_in, t_out, params) == pkg.CSINN_TRUE
    assert back.log == []  # recorded, not run
    for op, case, t_out, params in layers:
        node = C.cast(t_out.contents.data, C.POINTER(Node)).contents
        layer = node.in_[0].contents
        assert (layer.type, layer.in_num, layer.out_num) == (OP_IDS[op], 1, 1)
        assert C.addressof(layer.in_[0].contents) == t_in.contents.data
    for i, (op, case, t_out, params) in enumerate(layers):
        fe.csinn_set_output(i, t_out, sess)
    assert fe.csinn_session_setup(sess) == pkg.CSINN_TRUE
    x = rc._data("host graph", "int8", shape)
    for _ in range(2):
        fe.csinn_update_input(0, pkg.make_tensor(fe, keep, x.shape, pkg.DTYPE_INT8, pkg.LAYOUT_NCHW, data=x, sess=sess), sess)
        assert fe.csinn_session_run(sess) == pkg.CSINN_TRUE
        for i, (op, case, t_out, params) in enumerate(layers):
            want = rc.reduce_numpy(dict(case, x=x))
            got = pkg.make_tensor(fe, keep, (1,), pkg.DTYPE_INT8, pkg.LAYOUT_NCHW, sess=sess)
            fe.csinn_get_output(i, got, sess)
            data = np.ctypeslib.as_array(C.cast(got.contents.data, C.POINTER(C.c_int8)), (want.size,)).copy()
            fe.shl_mem_free(got.contents.data)
            assert np.array_equal(data.reshape(want.shape), want), op
    assert sorted(back.log) == sorted(list(rc.OPS) * 2)
    fe.csinn_session_deinit(sess)
    fe.csinn_free_session(sess)


# ------------------------------------------------------------------------------------ canonicalisation, the form rule
def test_canonicalisation():
    g = pkg.reduce_groups
    canon = lambda shape, axes: (rc.canonical(*g(shape, axes)[:2]), rc.canonical(*g(shape, axes)[2:]))
    assert g((2, 3, 4, 5), (2, 3)) == ([2, 3], [60, 20], [4, 5], [5, 1])
    assert canon((2, 3, 4, 5), (2, 3)) == ([(6, 20)], [(20, 1)])                       # NCHW over H and W: both lists merge
    assert canon((2, 4, 5, 3), (1, 2)) == ([(2, 60), (3, 1)], [(20, 3)])               # NHWC over H and W
    assert canon((2, 3, 4, 5), (0, 2)) == ([(3, 20), (5, 1)], [(2, 60), (4, 5)])       # N and H: neither list merges
    assert canon((1, 4, 1, 6), (0, 3)) == ([(4, 6)], [(6, 1)])                         # unit dims dropped
    assert canon((3, 4, 5), (0, 1, 2)) == ([], [(60, 1)])                              # everything: one run
    assert canon((3, 4), ()) == ([(12, 1)], [])                                        # nothing: inner size 1
    assert canon((2, 3, 4, 5, 6), (1, 3)) == ([(2, 360), (4, 30), (6, 1)], [(3, 120), (5, 6)])
    assert rc.canonical([2, 3], [7, 2]) == [(2, 7), (3, 2)] and rc.canonical([2, 3], [6, 2]) == [(6, 2)] and rc.canonical([2, 3], [3, 1]) == [(6, 1)]


def _name(hip, case, skew_in=0, skew_out=0, **override):
    """made-up, aligned, disjoint addresses: nothing is dereferenced"""
    desc = rc.cabi_desc(case, **override)
    return hip.shl_mi355x_reduce_kernel_name((1 << 40) + skew_in, (1 << 41) + skew_out, C.byref(desc)).decode()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_name_picks_the_expected_form_and_honours_the_switch(built, case, monkeypatch):
    """pure host code: no device is initialised, no pointer is followed"""
    monkeypatch.delenv(FORM_ENV, raising=False)
    hip = pkg.load_hip()
    natural = rc.expected_form(case)
    assert _name(hip, case) == natural
    es = case["x"].itemsize
    for skew in (es, 2 * es, 4 * es):  # off the 16-byte grid: the same launch, element loads at the edges
        assert _name(hip, case, skew_in=skew) == natural and _name(hip, case, skew_out=skew) == natural
    monkeypatch.setenv(FORM_ENV, "generic")
    assert _name(hip, case) == "reduce_generic"
    monkeypatch.setenv(FORM_ENV, "no such form")
    assert _name(hip, case) == natural  # only the forms' names mean anything


def test_every_form_is_exercised_for_every_dtype_and_kind():
    seen = {(rc.expected_form(c), c["dtype"], rc.kind_of(c["op"])) for c in CASES}
    for form in ("reduce_rows", "reduce_cols", "reduce_generic"):
        for dtype in ("int8", "f16"):
            for kind in ("sum", "mean", "max", "min"):
                assert (form, dtype, kind) in seen, (form, dtype, kind)
    inits = {(rc.descriptor(c)["init"], rc.kind_of(c["op"]), rc.expected_form(c)) for c in CASES}
    for kind in ("max", "min"):
        for form in ("reduce_rows", "reduce_cols"):
            assert (pkg.REDUCE_INIT_FIRST, kind, form) in inits and (pkg.REDUCE_INIT_FLT_MAX, kind, form) in inits


def test_the_four_group_limit(built, monkeypatch):
    monkeypatch.delenv(FORM_ENV, raising=False)
    hip = pkg.load_hip()
    case = dict(dtype="int8", in_q=(0.0625, 0), out_q=(0.0625, 0), op="sum")

    def name(shape, axes):
        x = np.lib.stride_tricks.as_strided(np.zeros(1, np.int8), shape, (0,) * len(shape))
        return _name(hip, dict(case, x=x, axes=axes))
    assert name((2,) * 8, (1, 3, 5, 7)) == "reduce_rows"      # four groups a side, none merges
    assert name((2,) * 8, (0, 2, 4, 6)) == "reduce_cols"
    nine = rc.cabi_desc(dict(case, x=np.zeros((2,) * 8, np.int8), axes=(1, 3, 5, 7)))
    # a fifth group on one side that does not merge: five outer dims kept apart by reduced ones need nine dims -- handed as raw
    # groups instead
    d = rc.cabi_desc(dict(case, x=np.zeros(1024, np.int8), axes=(0,)),
                     groups=([2, 2, 2, 2, 2], [512, 128, 32, 8, 2], [2], [1]))
    assert hip.shl_mi355x_reduce_kernel_name(1 << 40, 1 << 41, C.byref(d)) == b""
    assert hip.shl_mi355x_reduce(1 << 40, 1 << 41, C.byref(d), None) == EINVAL and b"more than 4 groups" in hip.shl_mi355x_last_error()
    d = rc.cabi_desc(dict(case, x=np.zeros(1024, np.int8), axes=(0,)),
                     groups=([2], [1], [2, 2, 2, 2, 2], [512, 128, 32, 8, 2]))
    assert hip.shl_mi355x_reduce(1 << 40, 1 << 41, C.byref(d), None) == EINVAL and b"more than 4 groups" in hip.shl_mi355x_last_error()
    # eight raw groups a side are fine when they merge or are unit groups
    d = rc.cabi_desc(dict(case, x=np.zeros(256, np.int8), axes=(0,)),
                     groups=([2, 1, 2, 1, 2, 1, 2, 1], [128, 0, 64, 0, 32, 0, 16, 0], [2, 2, 2, 2], [8, 4, 2, 1]))
    assert hip.shl_mi355x_reduce_kernel_name(1 << 40, 1 << 41, C.byref(d)) == b"reduce_rows"
    assert nine.n_out == 4 and nine.n_inner == 4


def test_the_shapes_of_real_models_take_rows_or_cols(built, monkeypatch):
    monkeypatch.delenv(FORM_ENV, raising=False)
    hip = pkg.load_hip()

    def name(op, shape, dtype, **kw):
        x = np.lib.stride_tricks.as_strided(np.zeros(1, np.int8 if dtype == "int8" else np.float16), shape, (0,) * len(shape))
        return _name(hip, dict(op=op, x=x, dtype=dtype, in_q=(0.0625, 0), out_q=(0.0625, 0), **kw))
    for dtype in ("int8", "f16"):
        for n in (1, 128):
            assert name("mean", (n, 7, 7, 1280), dtype, axes=(1, 2)) == "reduce_cols"          # a TF MobileNetV2 tail, NHWC
            assert name("mean", (n, 1280, 7, 7), dtype, axes=(2, 3)) == "reduce_rows"          # the same, NCHW
            for op in ("max", "mean"):                                                         # CBAM's spatial attention
                assert name(op, (n, 56, 56, 64), dtype, axes=(3,)) == "reduce_rows"
                assert name(op, (n, 64, 56, 56), dtype, axes=(1,)) == "reduce_cols"
            assert name("global_maxpool2d", (n, 56, 56, 64), dtype, layout="NHWC") == "reduce_cols"
            assert name("global_maxpool2d", (n, 64, 56, 56), dtype, layout="NCHW") == "reduce_rows"
            assert name("reduce_max", (n, 1000), dtype, axis=1) == "reduce_rows"


def test_invalid_descriptors_are_refused_before_touching_the_device(built):
    hip = pkg.load_hip()
    x = np.arange(96, dtype=np.int8)
    out = np.full(256, POISON, np.uint8)
    xin, o = x.ctypes.data, out.ctypes.data
    case = dict(op="sum", x=x.reshape(2, 3, 16), axes=(1,), dtype="int8", in_q=(0.0625, -5), out_q=(0.0625, -5))

    def refused(desc, in_ptr, out_ptr, text):
        status = hip.shl_mi355x_reduce(in_ptr, out_ptr, C.byref(desc) if desc is not None else None, None)
        assert status == EINVAL, (text, status)
        assert text.encode() in hip.shl_mi355x_last_error(), (text, hip.shl_mi355x_last_error())
        assert hip.shl_mi355x_reduce_kernel_name(in_ptr, out_ptr, C.byref(desc) if desc is not None else None) == b""
    ok = rc.cabi_desc(case)
    assert hip.shl_mi355x_reduce_kernel_name(xin, o, C.byref(ok)) == b"reduce_cols"
    refused(ok, None, o, "NULL argument")
    refused(ok, xin, None, "NULL argument")
    refused(None, xin, o, "NULL argument")
    refused(ok, xin, xin, "overlaps the input")
    refused(ok, xin, xin + 95, "overlaps the input")
    assert hip.shl_mi355x_reduce_kernel_name(xin, xin + 96, C.byref(ok)) != b""  # an output that begins where the input ends is fine
    f16 = rc.cabi_desc(dict(case, dtype="f16", x=np.zeros((2, 3, 8), np.float16)))
    refused(f16, xin + 1, o, "not aligned")
    refused(f16, xin, o + 1, "not aligned")
    for field, value, text in (("dtype", 2, "dtype"), ("kind", 4, "kind"), ("kind", -1, "kind"), ("init", 2, "initial-value"),
                               ("n_out", 9, "group count"), ("n_out", -1, "group count"), ("n_inner", 9, "group count"),
                               ("in_elems", 0, "no elements"), ("in_elems", -5, "no elements"), ("in_elems", 1 << 31, "2^31"),
                               ("in_elems", 95, "past the input")):
        bad = rc.cabi_desc(case)
        setattr(bad, field, value)
        refused(bad, xin, o, text)
    for field, k, value, text in (("out_extent", 0, -1, "negative"), ("out_stride", 1, -1, "negative"), ("inner_extent", 0, 0, "below 1"),
                                  ("inner_extent", 0, -3, "below 1"), ("inner_stride", 0, -16, "negative"),
                                  ("inner_extent", 0, 4, "past the input"), ("out_stride", 0, 49, "past the input"),
                                  ("out_extent", 0, 0x7FFFFFFF, "2^31 or more outputs"), ("inner_extent", 0, 0x7FFFFFFF, "past the input"),
                                  ("inner_stride", 0, 0x7FFFFFFF, "past the input")):
        bad = rc.cabi_desc(case)
        getattr(bad, field)[k] = value
        refused(bad, xin, o, text)
    huge = rc.cabi_desc(case, groups=([2], [0], [0x7FFFFFFF, 2], [0, 0]))
    refused(huge, xin, o, "2^31 or more elements per output")
    none = rc.cabi_desc(case)
    none.out_extent[0] = 0  # no outputs: fine, nothing to do
    assert hip.shl_mi355x_reduce(xin, o, C.byref(none), None) == 0
    assert np.all(out == POISON) and np.array_equal(x, np.arange(96, dtype=np.int8))


REFUSED_LAYERS = [
    # (what, case key, overrides of rc.layer_run)
    ("an output tensor of another size", "mean.nchw_over_hw_i8", dict(out_shape=(2, 4))),
    ("an inner extent past the input", "mean.nchw_over_hw_i8", dict(groups=([2, 5], [245, 49], [8, 7], [7, 1]))),
    ("a negative stride", "max.nchw_over_hw_f16", dict(groups=([2, 5], [-245, 49], [7, 7], [7, 1]))),
    ("nine outer groups", "sum.nchw_over_hw_i8", dict(groups=([2, 5] + [1] * 7, [245, 49] + [0] * 7, [7, 7], [7, 1]))),
    ("axis_count 2", "reduce_max.rank4_axis3_i8", dict(axis_count=2, axis=[3, 2])),
    ("axis_count 0", "reduce_sum.rank4_axis3_i8", dict(axis_count=0)),
    ("an axis beyond the rank", "reduce_mean.rank4_axis3_f16", dict(axis=[4])),
    ("a negative axis other than -1", "reduce_min.rank4_axis3_i8", dict(axis=[-2])),
    ("reduce: an output tensor of another size", "reduce_max.rank4_axis3_i8", dict(out_shape=(2, 3, 5))),
    ("whole tensor into two outputs", "reduce_sum.whole_tensor_i8", dict(out_shape=(2,))),
    ("global_maxpool2d: other channels", "global_maxpool2d.7x7_nchw_i8", dict(out_shape=(2, 4, 1, 1))),
    ("global_maxpool2d: a 3-d output", "global_maxpool2d.7x7_nhwc_f16", dict(out_shape=(2, 1, 5))),
]


@pytest.mark.parametrize("what,key,kw", REFUSED_LAYERS, ids=[r[0] for r in REFUSED_LAYERS])
def test_refused_layers_fail_in_the_callback_and_write_nothing(standalone, what, key, kw):
    """where the reference would read past a buffer or hit an assert; refused before anything is staged, so no device is
    needed"""
    fe, _, _ = standalone
    status, out = rc.layer_run(fe, pkg.API_MI355X, BY_KEY[key], poison=POISON, **kw)
    assert status != pkg.CSINN_TRUE, what
    assert np.all(out.view(np.uint8) == POISON), what


def test_perf_callbacks_name_the_kernel_form(standalone, monkeypatch):
    """init accepts the layer from dims, dtypes and records alone; perf reports the form the rule chooses"""
    fe, hip, opt = standalone
    monkeypatch.delenv(FORM_ENV, raising=False)
    opt.shl_cb_map_mi355x.restype = C.POINTER(pkg.Callback)
    opt.shl_cb_map_mi355x.argtypes = [C.c_int, C.c_int]
    for op in OP_IDS.values():
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
            rc.layer_run(fe, pkg.API_MI355X, case, perf=perf)
        assert seen[-1] == rc.expected_form(case), rc.case_id(case)
    monkeypatch.setenv(FORM_ENV, "generic")
    with pytest.raises(StopIteration):
        rc.layer_run(fe, pkg.API_MI355X, BY_KEY["mean.nchw_over_hw_f16"], perf=perf)
    assert seen[-1] == "reduce_generic"


FALL_THROUGH = r"""
import sys
sys.path.insert(0, %(tests)r)
import ctypes as C
import numpy as np
import cases, reduce_cases as rc
from cases import pkg
fe = cases.load_reference_frontend()          # genuine libshl_ref_x86.so
hip, opt = pkg.load_backend(fe)
fe.shl_cb_map_ref.restype = C.POINTER(pkg.Callback)
fe.shl_cb_map_ref.argtypes = [C.c_int, C.c_int]
opt.shl_cb_map_mi355x.restype = C.POINTER(pkg.Callback)
opt.shl_cb_map_mi355x.argtypes = [C.c_int, C.c_int]
by_key = {rc.golden_key(c): c for c in rc.all_cases()}
bad = 0
def probe(key, want_ref, **kw):
    global bad
    case = by_key[key]
    seen = []
    def perf(cb, *args):
        seen.append(cb.contents.exec)
        raise StopIteration
    try:
        rc.layer_run(fe, pkg.API_MI355X, case, perf=perf, **kw)
    except StopIteration:
        pass
    dt = pkg.DTYPE_INT8 if case["dtype"] == "int8" else pkg.DTYPE_FLOAT16
    op = getattr(pkg, "OP_" + case["op"].upper())
    ref = fe.shl_cb_map_ref(op, dt).contents.exec
    own = opt.shl_cb_map_mi355x(op, dt).contents.exec
    ok = seen == [ref if want_ref else own] and ref != own
    print(key, kw, "reference" if want_ref else "backend", "ok" if ok else "WRONG")
    bad += int(not ok)
probe("mean.nchw_over_hw_i8", False)
probe("mean.nchw_over_hw_i8", True, out_shape=(2, 4))
probe("max.nchw_over_hw_f16", False)
probe("reduce_max.rank4_axis3_i8", False)
probe("reduce_max.rank4_axis3_i8", True, axis_count=2, axis=[3, 2])
probe("reduce_sum.whole_tensor_i8", False)
probe("reduce_sum.whole_tensor_i8", True, out_shape=(2,))
probe("global_maxpool2d.7x7_nchw_i8", False)
probe("global_maxpool2d.7x7_nchw_i8", True, out_shape=(2, 4, 1, 1))
print("FALLTHROUGH_OK" if bad == 0 else "FALLTHROUGH_FAIL")
"""


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_a_refused_layer_is_handed_to_the_reference_at_init(built):
    """next to the genuine library init swaps the reference's exec into the layer's callback block; an accepted layer keeps
    the backend's.  Nothing is executed."""
    code = FALL_THROUGH % dict(tests=HERE)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert "FALLTHROUGH_OK" in res.stdout, res.stdout + res.stderr


# ------------------------------------------------------------------------------------ the host code under sanitizers
DRIVER = r"""
// Stand-alone driver of csrc/reduce_canon.h, the host code of csrc/reduce.hip: reads one descriptor per line, prints whether it
// is refused, the form, and the rows form's plan.  Nothing is launched.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "reduce_canon.h"

int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    long long dtype, kind, init, n_out, n_inner, in_elems, v;
    unsigned long long pin, pout;
    // <dtype> <kind> <init> <in_elems> <in address> <out address> <n_out> <n_inner> then 4 x 8 values: out extents, out strides,
    // inner extents, inner strides
    while (fscanf(f, "%lld %lld %lld %lld %llu %llu %lld %lld", &dtype, &kind, &init, &in_elems, &pin, &pout, &n_out, &n_inner) == 8) {
        struct shl_mi355x_reduce_desc *d = new shl_mi355x_reduce_desc;  // on the heap: reads past it are caught
        memset(d, 0, sizeof(*d));
        d->dtype = (int32_t)dtype, d->kind = (int32_t)kind, d->init = (int32_t)init, d->in_elems = in_elems;
        d->n_out = (int32_t)n_out, d->n_inner = (int32_t)n_inner;
        d->in_scale = 0.1f, d->in_zp = 3, d->out_scale = 0.02f, d->out_zp = -7;
        int32_t *lists[4] = {d->out_extent, d->out_stride, d->inner_extent, d->inner_stride};
        for (int l = 0; l < 4; l++)
            for (int k = 0; k < 8; k++) {
                if (fscanf(f, "%lld", &v) != 1) return 3;
                lists[l][k] = (int32_t)v;
            }
        shl::RdCanon c;
        const char *why = shl::rd_canonicalise((const void *)(uintptr_t)pin, (const void *)(uintptr_t)pout, d, &c);
        if (why) {
            printf("refused\n");
        } else if (c.out_count == 0) {
            printf("empty\n");  // nothing to do: the entry point returns OK without a launch
        } else {
            const int form = shl::rd_form(&c);
            shl::RdRows r = {0, 0, 0, 0, 0};
            if (form == shl::RD_ROWS) shl::rd_rows_plan(&c, d->dtype == SHL_MI355X_F16 ? 2 : 1, &r);
            printf("%s %d %d %lld %lld %d %d %d %d %d %d\n", shl::rd_form_name(form), c.n_out, c.n_in, (long long)c.out_count,
                   (long long)c.inner_size, r.run, r.segs, r.np, r.rows, r.passes, (int)shl::reduce_fma_ok(d, &c));
        }
        delete d;
    }
    fclose(f);
    return 0;
}
"""


def _line(desc, pin=1 << 40, pout=1 << 41):
    words = [desc.dtype, desc.kind, desc.init, desc.in_elems, pin, pout, desc.n_out, desc.n_inner]
    for lst in (desc.out_extent, desc.out_stride, desc.inner_extent, desc.inner_stride):
        words += list(lst)
    return " ".join(str(int(w)) for w in words)


def _hostile():
    """descriptors nobody means: negative extents, products that overflow, strides past the input, counts at the limits.
    (line, what the program must print first)"""
    base = BY_KEY["mean.nchw_over_hw_i8"]
    out = []
    accepted = []
    big = 0x7FFFFFFF
    for groups in (([-1, 5], [245, 49], [7, 7], [7, 1]), ([2, 5], [245, 49], [-7, 7], [7, 1]), ([big, big], [1, 1], [7], [1]),
                   ([2], [1], [big, big, big], [1, 1, 1]), ([big] * 8, [big] * 8, [big] * 8, [big] * 8),
                   ([2, 5], [big, big], [7, 7], [7, 1]), ([2, 5], [245, 49], [7, 7], [big, big]),
                   ([2, 5], [-big - 1, 49], [7, 7], [7, 1])):
        out.append(_line(rc.cabi_desc(base, groups=groups)))
    # ... and two that look hostile and are not: unit groups whose strides never count, a broadcast of element 0
    accepted.append((_line(rc.cabi_desc(base, groups=([1] * 8, [big] * 8, [1] * 8, [big] * 8))), "reduce_generic"))
    accepted.append((_line(rc.cabi_desc(base, groups=([big], [0], [big], [0]))), "reduce_generic"))
    accepted.append((_line(rc.cabi_desc(base, groups=([0, 5], [245, 49], [7, 7], [7, 1]))), "empty"))
    accepted.append((_line(rc.cabi_desc(base, groups=([0, big], [big, big], [7, 7], [7, 1]))), "empty"))
    for field, value in (("n_out", 9), ("n_out", -1), ("n_inner", 1 << 20), ("in_elems", -1), ("in_elems", 1 << 40), ("kind", 99),
                         ("dtype", -3), ("init", 7)):
        d = rc.cabi_desc(base)
        setattr(d, field, value)
        out.append(_line(d))
    out.append(_line(rc.cabi_desc(base), pin=0))
    out.append(_line(rc.cabi_desc(base), pin=1 << 40, pout=(1 << 40) + 17))
    out.append(_line(rc.cabi_desc(base), pin=(1 << 64) - 64, pout=1 << 41))
    return [(ln, "refused") for ln in out] + accepted


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc to compile with")
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on machines without a GPU")
def test_descriptor_code_runs_clean_under_address_and_undefined_sanitizers(built, tmp_path, monkeypatch):
    """csrc/reduce_canon.h -- validation, canonicalisation, the form rule, the rows plan: all the host code of csrc/reduce.hip
    -- compiled (-Xarch_host -fsanitize=address,undefined) into a program of its own, which takes every case's descriptor and
    a list of hostile ones apart and must name the same forms the library does"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    inc = os.path.join(cases.ROOT, "include")
    csrc = os.path.join(cases.ROOT, "csi-nn2_amd", "csrc")
    san = "-fsanitize=address,undefined"
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "reduce_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-gpu-rdc", "-ffp-contract=off", "-Xarch_host", san,
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + inc, "-I" + csrc, "-x", "hip", "-c",
                    str(tmp_path / "driver.cpp"), "-o", str(tmp_path / "driver.o")], check=True)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fno-gpu-rdc", san, str(tmp_path / "driver.o"), "-o", exe], check=True)
    skews = (0, 1, 2, 4)
    lines = [_line(rc.cabi_desc(c), pin=(1 << 40) + s * c["x"].itemsize) for c in CASES for s in skews]
    hostile = _hostile()
    (tmp_path / "problems.txt").write_text("\n".join(lines + [h[0] for h in hostile]) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    hip = pkg.load_hip()
    for force in (None, "generic"):
        e = dict(env)
        e.pop(FORM_ENV, None)
        monkeypatch.delenv(FORM_ENV, raising=False)
        if force:
            e[FORM_ENV] = force
            monkeypatch.setenv(FORM_ENV, force)
        res = subprocess.run([exe, str(tmp_path / "problems.txt")], capture_output=True, text=True, env=e, timeout=120)
        assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
        rows = [ln.split() for ln in res.stdout.splitlines()]
        assert len(rows) == len(lines) + len(hostile)
        for i, case in enumerate(c for c in CASES for _ in skews):
            row = rows[i]
            want = rc.expected_form(case, force=force)
            assert row[0] == want == _name(hip, case, skew_in=skews[i % len(skews)] * case["x"].itemsize), (rc.case_id(case), force, row)
            outs, inner = _sizes(case)
            assert (int(row[3]), int(row[4])) == (outs, inner)
            if want == "reduce_rows":
                run, segs, np_, rows_, passes = (int(v) for v in row[5:10])
                span = 15 + run * case["x"].itemsize
                assert run * segs == inner and np_ in (1, 2, 4, 8, 16) and rows_ * (4 * np_ + 1) <= 256 * 17 and rows_ <= 256
                assert passes * np_ * 16 >= span and (passes - 1) * np_ * 16 < span
                assert np_ == 16 or np_ * 16 >= span  # a short row takes one window
            if "hw_division" in case["name"]:
                assert row[10] == "1"  # (the driver's own records: within range)
        for (_, want), row in zip(hostile, rows[len(lines):]):
            assert row[0] == want, (want, row)


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
@pytest.mark.parametrize("dtype,layout", [("int8", "NHWC"), ("f16", "NCHW")])
@pytest.mark.parametrize("net", sorted(rc.NETS))
def test_oracle_chains_equal_the_genuine_graph_executor(net, dtype, layout):
    """the yardstick of tests/test_reduce_session.py: the networks through the genuine front-end, graph executor and C kernels
    (CSINN_REF) give the oracle chain's answer: int8 bit for bit, binary16 within the project's 1e-3"""
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)
    g = rc.NETS[net](dtype, layout)
    g.build(fe, pkg.API_REF)
    for k in (0, 1):
        x = g.input(k)
        got, want = g.run(fe, x), g.oracle(x)
        for name in g.outputs:
            what = "%s %s %s input %d, output %s" % (net, dtype, layout, k, name)
            if dtype == "int8":
                rc.assert_same(got[name], want[name], what)
            else:  # the C oracle's binary16 convolution sums in another order than the library's: the project's 1e-3
                g32, w32 = got[name].astype(np.float32), want[name].astype(np.float32)
                assert np.all(np.abs(g32 - w32) <= 1e-3 * np.maximum(np.abs(w32), 1e-3)), what
    g.close(fe)

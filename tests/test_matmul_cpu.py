"""matmul without a GPU: the goldens from the genuine library against the numpy restatement of its chain (one fused
multiply-add per step), the int8 mfma form's formula against them (bit for bit where the plan-time proof holds, inside the gate
elsewhere), the proof in Python against the proof in C, op id and the params block's layout, the exported entry points, the
front-end and the stand-in executor's host path, the form rule, refusals before the device is touched, and the descriptor code
in a stand-alone program under the address and undefined-behaviour sanitizers."""
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
import matmul_cases as mc
from cases import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = mc.all_cases()
IDS = [mc.case_id(c) for c in CASES]
GOLD = mc.golden()
BY_KEY = {mc.golden_key(c): c for c in CASES}
I8 = [c for c in CASES if c["dtype"] == "int8"]
POISON = 0x5A
EINVAL = -2
TP = C.POINTER(pkg.Tensor)
FORM_ENV = "SHL_MI355X_MATMUL_FORM"


def golden_of(case):
    g = GOLD[mc.golden_key(case)].reshape(case["out_shape"])
    return g.view(np.float16) if case["dtype"] == "f16" else g


def test_golden_covers_the_case_list():
    assert sorted(GOLD) == sorted(mc.golden_key(c) for c in CASES)
    for c in CASES:
        g = GOLD[mc.golden_key(c)]
        assert g.size == int(np.prod(c["out_shape"])) and g.dtype == (np.uint16 if c["dtype"] == "f16" else np.int8)
    path = os.path.join(HERE, "golden")
    assert os.path.getsize(os.path.join(path, "matmul_cases.npz")) <= os.path.getsize(os.path.join(path, "move_cases.npz"))


def test_case_list_covers_what_it_must():
    for dtype in ("int8", "f16"):
        cs = [c for c in CASES if c["dtype"] == dtype]
        assert {c["m"] for c in cs} >= set(mc.MS) and {c["n"] for c in cs} >= set(mc.NS) and {c["k"] for c in cs} >= set(mc.KS)
        assert {c["batches"] for c in cs} >= set(mc.BATCHES)
        assert {(c["trans_a"], c["trans_b"]) for c in cs} == {(False, False), (False, True), (True, False), (True, True)}
        dense = [c for c in cs if c["batches"] > 1 and c["b"].ndim == 2]
        assert dense and all(not c["trans_a"] and not c["trans_b"] for c in dense)
        assert any(c["a"].ndim == 4 and c["b"].ndim == 2 for c in cs) and any(c["a"].ndim == 3 and c["b"].ndim == 4 for c in cs)
        # the alignment fallback: batches > 1 with odd M K and odd K N, under every transpose
        odd = {(c["trans_a"], c["trans_b"]) for c in cs if c["batches"] > 1 and c["b"].ndim > 2 and (c["m"] * c["k"]) % 2 and (c["k"] * c["n"]) % 2}
        assert len(odd) == 4
    for zp in mc.ZPS:
        for rec in ("a_q", "b_q", "out_q"):
            assert any(c[rec][1] == zp for c in I8), (rec, zp)
    proven = [c for c in I8 if mc.is_exact(c)]
    assert proven and all(c["regime"] == "pow2" for c in proven) and all(mc.is_exact(c) for c in I8 if c["regime"] == "pow2")
    assert any(c["regime"] == "conv" and c["k"] == 3 for c in I8) and any(c["regime"] == "conv" and c["k"] == 130 for c in I8)
    f16 = {c["regime"] for c in CASES if c["dtype"] == "f16"}
    assert f16 == {"exact", "nonneg", "special"}
    for c in CASES:
        if c["regime"] == "exact":  # multiples of 2^-4 in [-4, 4]
            for x in (c["a"], c["b"]):
                v = x.astype(np.float64) * 16
                assert np.all(v == np.rint(v)) and np.all(np.abs(v) <= 64)
        if c["regime"] == "nonneg":
            assert np.all(c["a"] >= 0) and np.all(c["b"] >= 0)
    special = [c for c in CASES if c["regime"] == "special"]
    bits = np.concatenate([mc.bits(golden_of(c)).ravel() for c in special])
    assert {0x7FFF, 0xFFFF, 0x7BFF, 0xFBFF} <= set(bits.tolist()), "NaNs of both signs and both saturations reach the outputs"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chain_restatement_matches_the_reference_golden(case):
    mc.assert_same(mc.chain_ref(case), golden_of(case), mc.case_id(case) + ": chain_ref vs reference golden")


def test_a_rounded_product_would_not_match():
    """the reference's build contracts `total += a * b`: with converter scales the two-rounding chain gives other outputs"""
    differing = 0
    for case in (BY_KEY["fma_witness_%d_i8" % seed] for seed in mc.FMA_WITNESSES):
        a3, b3 = mc._operands(case)
        fa = mc.pool_cases.dequantise(a3, "int8", case["a_q"])
        fb = mc.pool_cases.dequantise(b3, "int8", case["b_q"])
        acc = np.zeros((a3.shape[0], a3.shape[1], b3.shape[2]), np.float32)
        for k in range(a3.shape[2]):
            acc = acc + fa[:, :, k, None] * fb[:, k, None, :]
        two = mc.pool_cases.requantise(acc, "int8", case["out_q"]).reshape(case["out_shape"])
        differing += int(np.count_nonzero(two != golden_of(case)))
    assert differing >= len(mc.FMA_WITNESSES)


@pytest.mark.parametrize("case", I8, ids=[mc.case_id(c) for c in I8])
def test_exact_formula_against_the_reference_golden(case):
    """bit for bit where the proof holds; elsewhere the reference's own chain rounds, and the chosen inputs stay inside the
    gate: every difference 1 LSB, at most max(2, 2e-4 n) of them"""
    got, want = mc.exact_ref(case), golden_of(case)
    if mc.is_exact(case):
        mc.assert_same(got, want, mc.case_id(case) + ": exact_ref vs reference golden (the proof holds)")
    else:
        mc.assert_within_gate(got, want, mc.case_id(case) + ": exact_ref vs reference golden")


def test_the_proof_in_c_agrees_with_its_restatement(built):
    hip = pkg.load_hip()
    for case in CASES:
        d = mc.cabi_desc(case)
        assert bool(hip.shl_mi355x_matmul_is_exact(C.byref(d))) == mc.is_exact(case), mc.case_id(case)
    assert hip.shl_mi355x_matmul_is_exact(None) == 0
    base = BY_KEY["regime_pow2_k130_i8"]
    # around the bound: K Aa Ab ma mb against 2^24, with zero points 0 (Aa = Ab = 128) and scales 3 2^-6, 2^-4
    for k, sa, sb, za, zb in ((341, 0.046875, 0.0625, 0, 0), (342, 0.046875, 0.0625, 0, 0), (1024, 0.5, 0.25, 0, 0),
                              (1023, 0.5, 0.25, 0, 0), (257, 1.0, 1.0, -128, 127), (258, 1.0, 1.0, -128, 127), (1, 0.0473, 1.0, 0, 0),
                              (3, 1.0, 1.0, 5, 5), (3, 0.0, 1.0, 0, 0), (3, float("inf"), 1.0, 0, 0), (3, float("nan"), 1.0, 0, 0),
                              (3, 2.0 ** -130, 1.0, 0, 0), (3, 2.0 ** 70, 1.0, 0, 0), (3, -0.5, 0.25, 0, 0), (3, 1.0, 1.0, 200, 0)):
        case = dict(base, k=k, a_q=(sa, za), b_q=(sb, zb))
        d = mc.cabi_desc(base)
        d.k, d.a_scale, d.a_zp, d.b_scale, d.b_zp = k, sa, za, sb, zb
        assert bool(hip.shl_mi355x_matmul_is_exact(C.byref(d))) == mc.is_exact(case), (k, sa, sb, za, zb)
    assert mc.is_exact(dict(base, k=341, a_q=(0.046875, 0), b_q=(0.0625, 0))) and not mc.is_exact(dict(base, k=342, a_q=(0.046875, 0), b_q=(0.0625, 0)))
    assert mc.is_exact(dict(base, k=1023, a_q=(0.5, 0), b_q=(0.25, 0))) and not mc.is_exact(dict(base, k=1024, a_q=(0.5, 0), b_q=(0.25, 0)))


def _probe():
    spec = importlib.util.spec_from_file_location("make_matmul_golden", os.path.join(HERE, "golden", "make_matmul_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_op_id_and_the_params_block_match_the_reference():
    want = json.load(open(os.path.join(HERE, "golden", "matmul_op_ids.json")))
    assert want["CSINN_OP_MATMUL"] == 95 == pkg.OP_MATMUL and want["sizeof csinn_matmul_params"] == 48
    inc = os.path.join(cases.ROOT, "include")
    assert _probe().measure([inc, os.path.join(inc, "csinn")]) == want  # this repository's headers, compiled
    text = open(os.path.join(inc, "csinn", "csinn_data_structure.h")).read()
    assert int(re.search(r"\bCSINN_OP_MATMUL\s*=\s*(\d+)", text).group(1)) == 95
    assert C.sizeof(pkg.MatmulParams) == want["sizeof csinn_matmul_params"]
    for field, _ in pkg.MatmulParams._fields_[1:]:
        assert getattr(pkg.MatmulParams, field).offset == want["offsetof csinn_matmul_params." + field], field


@pytest.mark.skipif(not cases.have_reference(), reason="the reference's headers are not present")
def test_the_committed_probe_result_is_what_the_genuine_headers_give():
    mod = _probe()
    ref = os.path.join(mod.reference_checkout(), "include")
    if not os.path.isdir(ref):
        pytest.skip("no reference checkout")
    assert mod.measure([ref, ref + "/csinn"]) == json.load(open(os.path.join(HERE, "golden", "matmul_op_ids.json")))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_libraries_export_the_entry_points(built):
    assert {"csinn_matmul", "csinn_matmul_init", "shl_gref_matmul"} <= _exports(pkg.lib_path("libcsinn_nn2.so"))
    assert {"shl_mi355x_matmul_init", "shl_mi355x_matmul_exec", "shl_mi355x_matmul_perf"} <= _exports(pkg.lib_path("libshl_mi355x_opt.so"))
    assert {"shl_mi355x_matmul", "shl_mi355x_matmul_kernel_name", "shl_mi355x_matmul_is_exact"} <= _exports(pkg.lib_path("libshl_mi355x.so"))
    assert C.sizeof(pkg.MatmulDesc) == 136 and pkg.MatmulDesc.a_batch_stride.offset == 24 and pkg.MatmulDesc.a_elems.offset == 72
    assert pkg.MatmulDesc.a_scale.offset == 96 and pkg.MatmulDesc.out_zp.offset == 116


# ------------------------------------------------------------------------------------ front-end and graph executor
FAKE_API = 7  # an unused slot of the dispatch tables
KEEP_ALIVE = []  # the C side keeps the callbacks' addresses


class Node(C.Structure):
    """struct shl_node (include/shl_gref.h)"""


Node._fields_ = [("type", C.c_int), ("in_", C.POINTER(C.POINTER(Node))), ("out", C.POINTER(C.POINTER(Node))),
                 ("subgraph_idx", C.c_int), ("in_num", C.c_int), ("out_num", C.c_int), ("name", C.c_char_p), ("data", C.c_void_p)]


class HostBackend:
    """matmul on the host, in numpy (chain_ref), registered in slot FAKE_API: what the graph executor's host path calls"""

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

        def run(a, b, o, p):
            pc = C.cast(p, C.POINTER(pkg.MatmulParams)).contents
            out = view(o)
            case = dict(dtype="int8", a=view(a), b=view(b), a_q=rec(a), b_q=rec(b), out_q=rec(o), out_shape=out.shape,
                        trans_a=bool(pc.trans_a), trans_b=bool(pc.trans_b))
            self.log.append((case["trans_a"], case["trans_b"]))
            out[...] = mc.chain_ref(case)
            return 1
        self.run = C.CFUNCTYPE(C.c_int, TP, TP, TP, C.c_void_p)(run)

        def op_map(op, dtype):
            if op != pkg.OP_MATMUL:
                return None
            if op not in self.table:
                cb = pkg.Callback()
                cb.exec = C.cast(self.run, C.c_void_p).value
                cb.est = C.cast(fe.shl_gref_matmul, C.c_void_p).value
                self.table[op] = cb
            return C.addressof(self.table[op])
        self.map_fn = C.CFUNCTYPE(C.c_void_p, C.c_int, C.c_int)(op_map)
        self.rt_fn = C.CFUNCTYPE(C.c_void_p, C.c_int)(lambda op: fe.shl_gref_runtime_callback(op))
        KEEP_ALIVE.append(self)
        fe.shl_register_op_callback(FAKE_API, C.cast(self.map_fn, C.c_void_p))
        fe.shl_register_runtime_callback(FAKE_API, C.cast(self.rt_fn, C.c_void_p))


def test_the_front_end_records_matmul_and_the_host_path_runs_it(built):
    """graph mode: csinn_matmul lands in shl_gref_matmul and appends one layer with two inputs and one output -- a constant
    second operand becomes a const node --; the stand-in executor's host path then runs them.  x [2, 5, 7] feeds q = x W
    (W [7, 6] constant: the dense broadcast) and s = q q^T (two activations, trans_b)"""
    fe = pkg.load_frontend("standalone")
    back = HostBackend(fe)
    keep = pkg.Keep()
    sess = fe.csinn_alloc_session()
    sc = sess.contents
    sc.base_api, sc.base_run_mode, sc.base_dtype = FAKE_API, pkg.RM_CPU_GRAPH, pkg.DTYPE_INT8
    sc.base_quant_type = pkg.QUANT_INT8_ASYM_W_SYM
    fe.csinn_session_init(sess)
    fe.csinn_set_input_number(1, sess)
    fe.csinn_set_output_number(2, sess)
    rng = np.random.default_rng(3)
    w = rng.integers(-128, 128, (7, 6), dtype=np.int8)
    q_x, q_w, q_q, q_s = (2.0 ** -4, 3), (2.0 ** -6, 0), (2.0 ** -4, -7), (2.0 ** -2, 11)
    T = lambda shape, q, name, **kw: pkg.make_tensor(fe, keep, shape, pkg.DTYPE_INT8, pkg.LAYOUT_NCHW, scales=(q[0],), zps=(q[1],),
                                                     name=name, sess=sess, **kw)
    t_x, t_w = T((2, 5, 7), q_x, b"x"), T((7, 6), q_w, b"w", data=w, is_const=1)
    t_q, t_s = T((2, 5, 6), q_q, b"q"), T((2, 5, 5), q_s, b"s")
    p_q = pkg.matmul_params(fe, keep, FAKE_API, pkg.LAYOUT_NCHW, False, False, sess, b"q")
    p_s = pkg.matmul_params(fe, keep, FAKE_API, pkg.LAYOUT_NCHW, False, True, sess, b"s")
    assert fe.csinn_matmul_init(t_x, t_w, t_q, p_q) == pkg.CSINN_TRUE
    assert fe.csinn_matmul_init(t_q, t_q, t_s, p_s) == pkg.CSINN_TRUE
    fe.csinn_set_tensor_entry(t_x, sess)
    fe.csinn_set_input(0, t_x, sess)
    assert fe.csinn_matmul(t_x, t_w, t_q, p_q) == pkg.CSINN_TRUE
    assert fe.csinn_matmul(t_q, t_q, t_s, p_s) == pkg.CSINN_TRUE
    assert back.log == []  # recorded, not run
    layer_q = C.cast(t_q.contents.data, C.POINTER(Node)).contents.in_[0].contents
    layer_s = C.cast(t_s.contents.data, C.POINTER(Node)).contents.in_[0].contents
    assert (layer_q.type, layer_q.in_num, layer_q.out_num) == (pkg.OP_MATMUL, 2, 1) == (layer_s.type, layer_s.in_num, layer_s.out_num)
    assert C.addressof(layer_q.in_[0].contents) == t_x.contents.data
    assert C.addressof(layer_s.in_[0].contents) == t_q.contents.data == C.addressof(layer_s.in_[1].contents)
    fe.csinn_set_output(0, t_q, sess)
    fe.csinn_set_output(1, t_s, sess)
    assert fe.csinn_session_setup(sess) == pkg.CSINN_TRUE
    for rep in range(2):
        x = rng.integers(-128, 128, (2, 5, 7), dtype=np.int8)
        fe.csinn_update_input(0, pkg.make_tensor(fe, keep, x.shape, pkg.DTYPE_INT8, pkg.LAYOUT_NCHW, data=x, sess=sess), sess)
        assert fe.csinn_session_run(sess) == pkg.CSINN_TRUE
        want_q = mc.chain_ref(dict(dtype="int8", a=x, b=w, a_q=q_x, b_q=q_w, out_q=q_q, out_shape=(2, 5, 6), trans_a=False, trans_b=False))
        want_s = mc.chain_ref(dict(dtype="int8", a=want_q, b=want_q, a_q=q_q, b_q=q_q, out_q=q_s, out_shape=(2, 5, 5), trans_a=False, trans_b=True))
        for i, want in enumerate((want_q, want_s)):
            got = pkg.make_tensor(fe, keep, (1,), pkg.DTYPE_INT8, pkg.LAYOUT_NCHW, sess=sess)
            fe.csinn_get_output(i, got, sess)
            data = np.ctypeslib.as_array(C.cast(got.contents.data, C.POINTER(C.c_int8)), (want.size,)).copy()
            fe.shl_mem_free(got.contents.data)
            assert np.array_equal(data.reshape(want.shape), want), i
    assert back.log == [(False, False), (False, True)] * 2
    fe.csinn_session_deinit(sess)
    fe.csinn_free_session(sess)


# ------------------------------------------------------------------------------------ the form rule, refusals
def _name(hip, case, a=1 << 40, b=1 << 41, o=1 << 42):
    return hip.shl_mi355x_matmul_kernel_name(a, b, o, C.byref(mc.cabi_desc(case))).decode()


@pytest.mark.parametrize("force", [None, "chain", "mfma"])
def test_kernel_name_picks_the_expected_form_and_honours_the_switch(built, force, monkeypatch):
    hip = pkg.load_hip()
    if force is None:
        monkeypatch.delenv(FORM_ENV, raising=False)
    else:
        monkeypatch.setenv(FORM_ENV, force)
    seen = set()
    for case in CASES:
        want = mc.expected_form(case, force)
        for skew in (0, 1, 2):  # pointers off the 16-byte grid keep the form: only the width of the loads changes
            es = case["a"].itemsize
            assert _name(hip, case, a=(1 << 40) + skew * es, b=(1 << 41) + skew * es) == want, (mc.case_id(case), skew)
        seen.add((case["dtype"], want))
    if force != "chain":
        assert seen == {("int8", pkg.MATMUL_CHAIN), ("int8", pkg.MATMUL_MFMA), ("f16", pkg.MATMUL_CHAIN), ("f16", pkg.MATMUL_MFMA)} or force == "mfma"
    # what the mfma form refuses falls to the chain even when forced: no unit stride on an operand, K beyond the int8 bound
    base = BY_KEY["k64_t00_i8"]
    d = mc.cabi_desc(base)
    d.a_row_stride, d.a_k_stride, d.a_elems = 2 * d.k, 2, 2 * d.a_elems
    assert hip.shl_mi355x_matmul_kernel_name(1 << 40, 1 << 41, 1 << 42, C.byref(d)).decode() == pkg.MATMUL_CHAIN
    d = mc.cabi_desc(base)
    d.k = pkg.MATMUL_MFMA_MAX_K + 1
    d.a_row_stride, d.a_elems, d.b_elems = d.k, d.batches * d.m * d.k, d.batches * d.k * d.n
    d.a_batch_stride, d.b_batch_stride = d.m * d.k, d.k * d.n
    assert hip.shl_mi355x_matmul_kernel_name(1 << 40, 1 << 41, 1 << 42, C.byref(d)).decode() == pkg.MATMUL_CHAIN
    d.dtype = pkg.SHL_F16
    assert hip.shl_mi355x_matmul_kernel_name(1 << 40, 1 << 41, 1 << 42, C.byref(d)).decode() == mc.expected_form(dict(base, dtype="f16"), force)


def test_invalid_descriptors_are_refused_before_touching_the_device(built):
    hip = pkg.load_hip()
    case = BY_KEY["dense_2x33x65x31_i8"]
    a, b = case["a"], case["b"]
    out = np.full(4096, POISON, np.uint8)
    pa, pb, po = a.ctypes.data, b.ctypes.data, out.ctypes.data

    def refused(desc, x, y, o, text):
        ref = C.byref(desc) if desc is not None else None
        status = hip.shl_mi355x_matmul(x, y, o, ref, None)
        assert status == EINVAL, (text, status)
        assert text.encode() in hip.shl_mi355x_last_error(), (text, hip.shl_mi355x_last_error())
        assert hip.shl_mi355x_matmul_kernel_name(x, y, o, ref) == b""
    ok = mc.cabi_desc(case)
    assert hip.shl_mi355x_matmul_kernel_name(pa, pb, po, C.byref(ok)) == pkg.MATMUL_MFMA.encode()
    refused(ok, None, pb, po, "NULL argument")
    refused(ok, pa, None, po, "NULL argument")
    refused(ok, pa, pb, None, "NULL argument")
    refused(None, pa, pb, po, "NULL argument")
    refused(ok, pa, pb, pa, "overlaps an operand")
    refused(ok, pa, pb, pa + a.nbytes - 1, "overlaps an operand")
    refused(ok, pa, pb, pb + b.nbytes - 1, "overlaps an operand")
    room = np.zeros(a.nbytes + 4096, np.uint8)  # the first operand and, right behind it, the output: touching is fine
    assert hip.shl_mi355x_matmul_kernel_name(room.ctypes.data, pb, room.ctypes.data + a.nbytes, C.byref(ok)) != b""
    refused(ok, room.ctypes.data, pb, room.ctypes.data + a.nbytes - 1, "overlaps an operand")
    f16 = mc.cabi_desc(BY_KEY["dense_2x33x65x31_f16"])
    refused(f16, pa + 1, pb, po, "not aligned")
    refused(f16, pa, pb + 1, po, "not aligned")
    refused(f16, pa, pb, po + 1, "not aligned")
    for field, value, text in (("dtype", 2, "dtype"), ("m", 0, "below 1"), ("n", 0, "below 1"), ("k", 0, "below 1"), ("batches", 0, "below 1"),
                               ("m", -33, "below 1"), ("k", -1, "below 1"), ("a_elems", 0, "without elements"), ("b_elems", -4, "without elements"),
                               ("out_elems", 0, "without elements"), ("a_elems", 1 << 31, "2^31"), ("b_elems", 1 << 31, "2^31"),
                               ("out_elems", 1 << 31, "2^31"), ("a_batch_stride", -1, "negative stride"), ("a_row_stride", -65, "negative stride"),
                               ("a_k_stride", -1, "negative stride"), ("b_batch_stride", -1, "negative stride"),
                               ("b_col_stride", -1, "negative stride"), ("b_k_stride", -31, "negative stride"),
                               ("out_elems", 2 * 33 * 31 + 1, "batches x m x n"), ("out_elems", 33 * 31, "batches x m x n"),
                               ("m", 0x7FFFFFFF, "batches x m x n"), ("a_elems", a.size - 1, "past the first operand"),
                               ("b_elems", b.size - 1, "past the second operand"), ("a_k_stride", 2, "past the first operand"),
                               ("b_batch_stride", 1, "past the second operand"), ("a_row_stride", 1 << 40, "past the first operand"),
                               ("b_k_stride", 1 << 62, "past the second operand"), ("k", 66, "past the first operand")):
        bad = mc.cabi_desc(case)
        setattr(bad, field, value)
        refused(bad, pa, pb, po, text)
    assert np.all(out == POISON)


REFUSED_LAYERS = [
    # (what, case key or a case, overrides of mc.layer_run)
    ("an output tensor of another size", "dense_2x33x65x31_i8", dict(out_shape=(2, 33, 30))),
    ("an output tensor without the batches", "dense_2x33x65x31_f16", dict(out_shape=(33, 31))),
    ("the broadcast with trans_b", "dense_3x64x64x64_i8", dict(trans_b=True)),
    ("the broadcast with trans_a", "dense_3x64x64x64_f16", dict(trans_a=True)),
    ("mat1 has more batches than mat0", dict(BY_KEY["dense_2x33x65x31_i8"], a=BY_KEY["dense_2x33x65x31_i8"]["a"][0],
                                             b=np.zeros((2, 65, 31), np.int8), out_shape=(2, 33, 31)), {}),
    ("batches 2 and 3", dict(BY_KEY["dense_2x33x65x31_i8"], b=np.zeros((3, 65, 31), np.int8)), {}),
    ("the operands disagree on K", dict(BY_KEY["dense_2x33x65x31_i8"], b=np.zeros((64, 31), np.int8)), {}),
    ("a 1-d operand", dict(BY_KEY["dense_2x33x65x31_i8"], b=np.zeros((65,), np.int8), out_shape=(2, 33, 1)), {}),
]


@pytest.mark.parametrize("what,key,kw", REFUSED_LAYERS, ids=[r[0] for r in REFUSED_LAYERS])
def test_refused_layers_fail_in_the_callback_and_write_nothing(standalone, what, key, kw):
    """where the reference would return CSINN_FALSE after converting three tensors, or read past a buffer; refused before
    anything is staged, so no device is needed"""
    fe, _, _ = standalone
    case = BY_KEY[key] if isinstance(key, str) else key
    status, out = mc.layer_run(fe, pkg.API_MI355X, case, poison=POISON, **kw)
    assert status != pkg.CSINN_TRUE, what
    assert np.all(out.view(np.uint8) == POISON), what


def test_perf_callback_names_the_kernel_form(standalone, monkeypatch):
    """init accepts the layer from dims, dtypes and records alone; perf reports the form the rule chooses"""
    fe, hip, opt = standalone
    monkeypatch.delenv(FORM_ENV, raising=False)
    opt.shl_cb_map_mi355x.restype = C.POINTER(pkg.Callback)
    opt.shl_cb_map_mi355x.argtypes = [C.c_int, C.c_int]
    for dt in (pkg.DTYPE_INT8, pkg.DTYPE_FLOAT16):
        cb = opt.shl_cb_map_mi355x(pkg.OP_MATMUL, dt)
        assert cb and cb.contents.perf and cb.contents.exec and cb.contents.est and cb.contents.init
    seen = []

    def perf(cb, t_a, t_b, t_o, params):
        name = C.c_char_p()
        fn = C.CFUNCTYPE(C.c_int, TP, TP, TP, C.c_void_p, C.POINTER(C.c_char_p))(cb.contents.perf)
        assert fn(t_a, t_b, t_o, params, C.byref(name)) == pkg.CSINN_TRUE
        seen.append(name.value.decode())
        raise StopIteration  # nothing is executed: no device is needed
    for case in CASES:
        with pytest.raises(StopIteration):
            mc.layer_run(fe, pkg.API_MI355X, case, perf=perf)
        assert seen[-1] == mc.expected_form(case), mc.case_id(case)
    monkeypatch.setenv(FORM_ENV, "chain")
    with pytest.raises(StopIteration):
        mc.layer_run(fe, pkg.API_MI355X, BY_KEY["dense_3x64x64x64_f16"], perf=perf)
    assert seen[-1] == pkg.MATMUL_CHAIN


FALL_THROUGH = r"""
import sys
sys.path.insert(0, %(tests)r)
import ctypes as C
import numpy as np
import cases, matmul_cases as mc
from cases import pkg
fe = cases.load_reference_frontend()          # genuine libshl_ref_x86.so
hip, opt = pkg.load_backend(fe)
fe.shl_cb_map_ref.restype = C.POINTER(pkg.Callback)
fe.shl_cb_map_ref.argtypes = [C.c_int, C.c_int]
opt.shl_cb_map_mi355x.restype = C.POINTER(pkg.Callback)
opt.shl_cb_map_mi355x.argtypes = [C.c_int, C.c_int]
by_key = {mc.golden_key(c): c for c in mc.all_cases()}
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
    ref = fe.shl_cb_map_ref(pkg.OP_MATMUL, dt).contents.exec
    own = opt.shl_cb_map_mi355x(pkg.OP_MATMUL, dt).contents.exec
    ok = seen == [ref if want_ref else own] and ref != own
    print(key, kw, "reference" if want_ref else "backend", "ok" if ok else "WRONG")
    bad += int(not ok)
probe("dense_2x33x65x31_i8", False)
probe("dense_2x33x65x31_i8", True, out_shape=(2, 33, 30))
probe("dense_3x64x64x64_f16", False)
probe("dense_3x64x64x64_f16", True, trans_b=True)
probe("m65_t11_i8", False)
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
// Stand-alone driver of csrc/matmul_canon.h, the host code of csrc/matmul.hip: reads one descriptor per line, prints whether it
// is refused, else the form, the plan and the proof.  Nothing is launched.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "matmul_canon.h"

int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    long long v[14], za, zb;
    unsigned long long pa, pb, po;
    float sa, sb;
    // <dtype> <batches> <m> <n> <k> <6 strides> <3 element counts> <3 addresses> <a scale> <a zp> <b scale> <b zp>
    for (;;) {
        int got = 0;
        for (int i = 0; i < 14; i++) got += fscanf(f, "%lld", &v[i]) == 1;
        if (got != 14) break;
        if (fscanf(f, "%llu %llu %llu %a %lld %a %lld", &pa, &pb, &po, &sa, &za, &sb, &zb) != 7) return 3;
        struct shl_mi355x_matmul_desc *d = new shl_mi355x_matmul_desc;  // on the heap: reads past it are caught
        memset(d, 0, sizeof(*d));
        d->dtype = (int32_t)v[0], d->batches = (int32_t)v[1], d->m = (int32_t)v[2], d->n = (int32_t)v[3], d->k = (int32_t)v[4];
        d->a_batch_stride = v[5], d->a_row_stride = v[6], d->a_k_stride = v[7];
        d->b_batch_stride = v[8], d->b_col_stride = v[9], d->b_k_stride = v[10];
        d->a_elems = v[11], d->b_elems = v[12], d->out_elems = v[13];
        d->a_scale = sa, d->a_zp = (int32_t)za, d->b_scale = sb, d->b_zp = (int32_t)zb, d->out_scale = 0.02f, d->out_zp = -7;
        const void *a = (const void *)(uintptr_t)pa, *b = (const void *)(uintptr_t)pb, *o = (const void *)(uintptr_t)po;
        const char *why = shl::mm_validate(a, b, o, d);
        if (why) {
            printf("refused %d\n", (int)shl::mm_is_exact(d));
        } else {
            shl::MmPlan p;
            shl::mm_plan(a, b, d, &p);
            printf("%s %d %d %d %d %d %d %d\n", shl::mm_form_name(shl::mm_form(d, &p)), p.a_kcontig, p.b_kcontig, p.a_vec, p.b_vec,
                   p.mfma_fits, (int)shl::mm_is_exact(d), (int)shl::mm_fma_ok(d));
        }
        delete d;
    }
    fclose(f);
    return 0;
}
"""


def _line(desc, pa=1 << 40, pb=1 << 41, po=1 << 42):
    words = [desc.dtype, desc.batches, desc.m, desc.n, desc.k, desc.a_batch_stride, desc.a_row_stride, desc.a_k_stride,
             desc.b_batch_stride, desc.b_col_stride, desc.b_k_stride, desc.a_elems, desc.b_elems, desc.out_elems, pa, pb, po]
    return " ".join(str(int(w)) for w in words) + " %s %d %s %d" % (float(desc.a_scale).hex(), desc.a_zp, float(desc.b_scale).hex(), desc.b_zp)


def _hostile():
    """descriptors nobody means: zero and negative dims, 2^31 elements, products that overflow, strides past the operands,
    overlapping buffers.  (line, what the program must print first)"""
    base = BY_KEY["dense_2x33x65x31_i8"]
    big = 0x7FFFFFFF
    out = []
    for fields in (dict(m=0), dict(n=-1), dict(k=0), dict(batches=-2), dict(m=big, n=big, k=big, batches=big),
                   dict(a_elems=1 << 31), dict(b_elems=1 << 31), dict(out_elems=1 << 31), dict(a_elems=(1 << 63) - 1),
                   dict(out_elems=-1), dict(a_row_stride=-1), dict(a_batch_stride=(1 << 63) - 1), dict(b_k_stride=(1 << 63) - 1),
                   dict(a_k_stride=1 << 62, a_row_stride=1 << 62, a_batch_stride=1 << 62), dict(b_col_stride=big, b_k_stride=big),
                   dict(dtype=-3), dict(out_elems=2 * 33 * 31 - 1), dict(batches=big, m=big, out_elems=1)):
        d = mc.cabi_desc(base)
        for k, v in fields.items():
            setattr(d, k, v)
        out.append(_line(d))
    d = mc.cabi_desc(base)
    out.append(_line(d, pa=0))
    out.append(_line(d, po=(1 << 40) + 17))                 # inside the first operand
    out.append(_line(d, po=(1 << 41) - 5))                  # its tail reaches into the second
    out.append(_line(d, pa=(1 << 64) - 64))                 # wraps around the address space
    accepted = []
    one = mc.cabi_desc(base)                                # extents of 1 whose strides never count
    one.batches, one.m, one.out_elems = 1, 1, 31
    one.a_batch_stride, one.a_row_stride = (1 << 63) - 1, (1 << 63) - 1
    accepted.append((_line(one), None))                     # (K = 65: the mfma form, unless the chain is forced)
    return [(ln, "refused") for ln in out] + accepted


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc to compile with")
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on machines without a GPU")
def test_descriptor_code_runs_clean_under_address_and_undefined_sanitizers(built, tmp_path, monkeypatch):
    """csrc/matmul_canon.h -- validation, the plan, the form rule, the proof: all the host code of csrc/matmul.hip -- compiled
    (-Xarch_host -fsanitize=address,undefined) into a program of its own, which takes every case's descriptor and a list of
    hostile ones apart and must name the same forms the library does and give the proof's verdict the restatement gives"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    inc = os.path.join(cases.ROOT, "include")
    csrc = os.path.join(cases.ROOT, "csi-nn2_amd", "csrc")
    san = "-fsanitize=address,undefined"
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "matmul_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-gpu-rdc", "-ffp-contract=off", "-Xarch_host", san,
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + inc, "-I" + csrc, "-x", "hip", "-c",
                    str(tmp_path / "driver.cpp"), "-o", str(tmp_path / "driver.o")], check=True)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fno-gpu-rdc", san, str(tmp_path / "driver.o"), "-o", exe], check=True)
    skews = (0, 1, 2, 8)
    lines = [_line(mc.cabi_desc(c), pa=(1 << 40) + s * c["a"].itemsize, pb=(1 << 41) + s * c["a"].itemsize) for c in CASES for s in skews]
    hostile = _hostile()
    (tmp_path / "problems.txt").write_text("\n".join(lines + [h[0] for h in hostile]) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    hip = pkg.load_hip()
    for force in (None, "chain", "mfma"):
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
            row, s = rows[i], skews[i % len(skews)] * case["a"].itemsize
            want = mc.expected_form(case, force=force)
            assert row[0] == want == _name(hip, case, a=(1 << 40) + s, b=(1 << 41) + s), (mc.case_id(case), force, row)
            a_kc, b_kc, a_vec, b_vec, fits, exact = (int(v) for v in row[1:7])
            assert fits == 1 and exact == int(mc.is_exact(case))
            assert a_kc == int(not case["trans_a"] or case["k"] == 1 or case["m"] == 1)  # (a k stride of 1 either way)
            assert b_kc == int(case["trans_b"] or case["k"] == 1 or case["n"] == 1)
            if s % 16:
                assert a_vec == 0 and b_vec == 0  # a pointer off the grid: no 16-byte loads
        for (_, want), row in zip(hostile, rows[len(lines):]):
            assert row[0] == (want or (pkg.MATMUL_CHAIN if force == "chain" else pkg.MATMUL_MFMA)), (want, row)

"""Split and shuffle_channel, the part that needs no GPU: the numpy restatements of the reference against the genuine
library's golden outputs and, where it is built, the live library; the op ids and the params blocks; the exported symbols;
the stand-alone front-end and graph executor (a layer with several outputs); the kernel-form rules; refusals."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import split_shuffle_cases as ssc
from cases import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ssc.all_cases()
IDS = ["%s-%s" % (c["op"], c["name"]) for c in CASES]
GOLD = ssc.golden()
POISON = 0x5A
EINVAL = -2


def test_golden_covers_the_case_list():
    assert sorted(GOLD) == sorted(k for c in CASES for k in ssc.golden_keys(c))
    path = os.path.join(HERE, "golden", "split_shuffle_cases.npz")
    largest = max(os.path.getsize(os.path.join(HERE, "golden", f)) for f in os.listdir(os.path.join(HERE, "golden"))
                  if f.endswith(".npz") and f != "split_shuffle_cases.npz")
    assert os.path.getsize(path) < largest


def test_case_list_covers_what_it_must():
    split = {c["name"]: c for c in CASES if c["op"] == "split"}
    shuf = {c["name"]: c for c in CASES if c["op"] == "shuffle"}
    assert {c["n"] for c in split.values()} >= {1, 2, 8, 9, 17}
    assert {c["axis"] for c in split.values()} >= {-3, -1, 0, 1, 2, 3} and {c["x"].ndim for c in split.values()} >= {1, 2, 4}
    assert any(c["index"] is None for c in split.values()) and any(c["index"] is not None for c in split.values())
    assert split["null_index_10_into_3_i8"]["lens"] == [4, 4, 2] and split["null_index_7_into_4_f16"]["lens"] == [2, 2, 2, 1]
    for layout in ("NHWC", "NCHW"):
        assert {c["axis"] for c in split.values() if c["layout"] == layout and c["x"].ndim == 4} >= {0, 1, 2, 3}
    assert {c["group"] for c in shuf.values()} >= {1, 2, 3, 4, 8, 16}
    assert any(c["group"] == c["x"].shape[3] for c in shuf.values() if c["layout"] == "NHWC")
    assert {c["x"].shape[0] for c in shuf.values()} >= {1, 2}
    for name in ("exhaustive_f16_nhwc", "exhaustive_f16_nchw"):
        assert np.array_equal(shuf[name]["x"].view(np.uint16).ravel(), np.arange(65536, dtype=np.uint16))
    assert sorted(split["exhaustive_f16"]["x"].view(np.uint16).ravel().tolist())[-1] == 65535
    assert len(set(split["exhaustive_f16"]["x"].view(np.uint16).ravel().tolist())) == 65536
    # every (input record, output record) pair of the int8 cases is walked exhaustively, by both ops
    for cs, prefix in ((split, "exhaustive_i8_"), (shuf, "exhaustive_i8_")):
        walked, used = set(), set()
        for c in cs.values():
            if c["dtype"] != "int8":
                continue
            pairs = {(c["in_q"], q) for q in (c["out_qs"] if c["op"] == "split" else [c["out_q"]])}
            used |= pairs
            if c["name"].startswith(prefix):
                assert sorted(c["x"].ravel().tolist())[::c["x"].size // 256] == list(range(-128, 128))
                walked |= pairs
        assert used <= walked, used - walked


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_numpy_restatement_matches_the_reference_golden(case):
    for key, got in zip(ssc.golden_keys(case), ssc.outputs_numpy(case)):
        ssc.assert_same(got, GOLD[key], key + " vs golden")


def test_binary16_round_trip_changes_only_infinities_and_nans():
    h = np.arange(65536, dtype=np.uint32)
    mag, sign = h & 0x7FFF, h & 0x8000
    want = np.where(mag == 0x7C00, 0x7BFF | sign, np.where(mag > 0x7C00, 0x7FFF | sign, h))
    got = np.concatenate([GOLD["split.exhaustive_f16#0"].ravel(), GOLD["split.exhaustive_f16#2"].ravel()]).astype(np.uint32)
    assert np.array_equal(got, want)
    # shuffle_channel of all patterns, group 2 over 8 channels: the same function of the permuted input
    src = h.reshape(-1, 2, 4).transpose(0, 2, 1).ravel()
    assert np.array_equal(GOLD["shuffle.exhaustive_f16_nhwc#0"].ravel().astype(np.uint32), want[src])


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_numpy_restatement_matches_the_live_reference():
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)  # errors only: the library warns about every binary16 saturation
    for case in CASES:
        got = ssc.layer_run(fe, pkg.API_REF, case)
        for key, g, w in zip(ssc.golden_keys(case), got, ssc.outputs_numpy(case)):
            ssc.assert_same(w, g, key + " vs live reference")
            ssc.assert_same(g, GOLD[key], key + ": live reference vs golden")


def _probe():
    spec = importlib.util.spec_from_file_location("make_split_shuffle_golden",
                                                  os.path.join(HERE, "golden", "make_split_shuffle_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_op_ids_and_params_blocks_match_the_reference():
    want = json.load(open(os.path.join(HERE, "golden", "split_shuffle_op_ids.json")))
    assert want == {"CSINN_OP_SPLIT": 166, "CSINN_OP_SHUFFLE_CHANNEL": 153, "sizeof csinn_split_params": 56,
                    "offsetof csinn_split_params.split_index": 40, "offsetof csinn_split_params.output_num": 48,
                    "offsetof csinn_split_params.axis": 52, "sizeof csinn_shuffle_channel_params": 48,
                    "offsetof csinn_shuffle_channel_params.group": 40}
    inc = os.path.join(cases.ROOT, "include")
    assert _probe().measure([inc, os.path.join(inc, "csinn")]) == want  # this repository's headers, compiled
    text = open(os.path.join(inc, "csinn", "csinn_data_structure.h")).read()
    assert int(re.search(r"\bCSINN_OP_SPLIT\s*=\s*(\d+)", text).group(1)) == 166
    assert int(re.search(r"\bCSINN_OP_SHUFFLE_CHANNEL\s*=\s*(\d+)", text).group(1)) == 153
    assert (pkg.OP_SPLIT, pkg.OP_SHUFFLE_CHANNEL) == (166, 153)
    assert C.sizeof(pkg.SplitParams) == 56 and C.sizeof(pkg.ShuffleChannelParams) == 48
    assert (pkg.SplitParams.split_index.offset, pkg.SplitParams.output_num.offset, pkg.SplitParams.axis.offset) == (40, 48, 52)
    assert pkg.ShuffleChannelParams.group.offset == 40


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_libraries_export_the_entry_points(built):
    assert {"csinn_split_init", "csinn_split", "csinn_shuffle_channel_init", "csinn_shuffle_channel", "shl_gref_split",
            "shl_gref_shuffle_channel"} <= _exports(pkg.lib_path("libcsinn_nn2.so"))
    assert {"shl_mi355x_split_exec", "shl_mi355x_split_perf", "shl_mi355x_shuffle_channel_exec",
            "shl_mi355x_shuffle_channel_perf"} <= _exports(pkg.lib_path("libshl_mi355x_opt.so"))
    assert {"shl_mi355x_split", "shl_mi355x_split_kernel_name", "shl_mi355x_shuffle_channel",
            "shl_mi355x_shuffle_channel_kernel_name"} <= _exports(pkg.lib_path("libshl_mi355x.so"))
    assert C.sizeof(pkg.SplitDesc) == 40 and pkg.SplitDesc.outer.offset == 8 and pkg.SplitDesc.in_scale.offset == 16
    assert C.sizeof(pkg.ShuffleDesc) == 64 and pkg.ShuffleDesc.outer.offset == 8 and pkg.ShuffleDesc.in_scale.offset == 32


# ------------------------------------------------------------------------------------ front-end and graph executor
FAKE_API = 6  # an unused slot of the dispatch tables
TP = C.POINTER(pkg.Tensor)


class Node(C.Structure):
    """struct shl_node (include/shl_gref.h)"""


Node._fields_ = [("type", C.c_int), ("in_", C.POINTER(C.POINTER(Node))), ("out", C.POINTER(C.POINTER(Node))),
                 ("subgraph_idx", C.c_int), ("in_num", C.c_int), ("out_num", C.c_int), ("name", C.c_char_p), ("data", C.c_void_p)]


class HostBackend:
    """split and shuffle_channel on the host, in numpy, registered in slot FAKE_API: what the graph executor's host path
    calls; records every call"""

    def __init__(self, fe):
        self.fe, self.log, self.keep, self.table = fe, [], [], {}
        fe.shl_gref_runtime_callback.restype = C.c_void_p
        fe.shl_gref_runtime_callback.argtypes = [C.c_int]

        def view(t, dtype=np.int8):
            tc = t.contents
            shape = tuple(tc.dim[i] for i in range(tc.dim_count))
            return np.ctypeslib.as_array(C.cast(tc.data, C.POINTER(C.c_int8)), shape)

        def rec(t):
            return (t.contents.qinfo.contents.scale, t.contents.qinfo.contents.zero_point)

        def split(i, outs, p):
            pc = C.cast(p, C.POINTER(pkg.SplitParams)).contents
            n = pc.output_num
            self.log.append(("split", n))
            x = view(i)
            lens = ssc.chunk_lens(x.shape[pc.axis], n, [pc.split_index[k] for k in range(n - 1)] if pc.split_index else None)
            got = ssc.split_numpy(dict(x=x, axis=pc.axis, dtype="int8", lens=lens, in_q=rec(i), out_qs=[rec(outs[k]) for k in range(n)]))
            for k in range(n):
                view(outs[k])[...] = got[k]
            return 1

        def shuffle(i, o, p):
            pc = C.cast(p, C.POINTER(pkg.ShuffleChannelParams)).contents
            self.log.append(("shuffle", pc.group))
            view(o)[...] = ssc.shuffle_numpy(dict(x=view(i), group=pc.group, dtype="int8", layout="NHWC", in_q=rec(i), out_q=rec(o)))
            return 1
        fns = {pkg.OP_SPLIT: (C.CFUNCTYPE(C.c_int, TP, C.POINTER(TP), C.c_void_p)(split), fe.shl_gref_split),
               pkg.OP_SHUFFLE_CHANNEL: (C.CFUNCTYPE(C.c_int, TP, TP, C.c_void_p)(shuffle), fe.shl_gref_shuffle_channel)}

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
        self.keep.append(fns)
        fe.shl_register_op_callback(FAKE_API, C.cast(self.map_fn, C.c_void_p))
        fe.shl_register_runtime_callback(FAKE_API, C.cast(self.rt_fn, C.c_void_p))


def test_the_front_end_records_a_split_as_one_layer_and_the_host_path_runs_it(built):
    """graph mode: csinn_split lands in shl_gref_split, which appends ONE layer with output_num output nodes; the stand-in
    executor's host path then allocates every output, hands the callback the array and releases what nobody reads.
    data -> split(3: 4, 4, 2 of 10 channels) -> [0] graph output; [1] read by nobody; [2] -> shuffle_channel(2) -> output"""
    fe = pkg.load_frontend("standalone")
    s = fe.csinn_alloc_session()
    fe.csinn_free_session(s)
    back = HostBackend(fe)
    keep = pkg.Keep()
    sess = fe.csinn_alloc_session()
    sc = sess.contents
    sc.base_api, sc.base_run_mode, sc.base_dtype = FAKE_API, pkg.RM_CPU_GRAPH, pkg.DTYPE_INT8
    sc.base_quant_type = pkg.QUANT_INT8_ASYM_W_SYM
    fe.csinn_session_init(sess)
    fe.csinn_set_input_number(1, sess)
    fe.csinn_set_output_number(2, sess)
    recs = [ssc.Q_SAME, ssc.Q_CONV[0], ssc.Q_A]
    T = lambda shape, q, name: pkg.make_tensor(fe, keep, shape, pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, scales=(q[0],), zps=(q[1],),
                                               name=name, sess=sess)
    t_in = T((1, 2, 3, 10), ssc.Q_SAME, b"data")
    parts = [T((1, 2, 3, c), q, b"part%d" % i) for i, (c, q) in enumerate(zip((4, 4, 2), recs))]
    t_sh = T((1, 2, 3, 2), ssc.Q_B, b"shuffled")
    p_split = pkg.split_params(fe, keep, FAKE_API, pkg.LAYOUT_NHWC, 3, 3, None, sess)
    p_shuf = pkg.shuffle_channel_params(fe, keep, FAKE_API, pkg.LAYOUT_NHWC, 2, sess)
    outs = pkg.tensor_array(keep, parts)
    assert fe.csinn_split_init(t_in, outs, p_split) == pkg.CSINN_TRUE
    assert fe.csinn_shuffle_channel_init(parts[2], t_sh, p_shuf) == pkg.CSINN_TRUE
    fe.csinn_set_tensor_entry(t_in, sess)
    fe.csinn_set_input(0, t_in, sess)
    assert fe.csinn_split(t_in, outs, p_split) == pkg.CSINN_TRUE
    assert fe.csinn_shuffle_channel(parts[2], t_sh, p_shuf) == pkg.CSINN_TRUE
    assert back.log == []  # recorded, not run
    nodes = [C.cast(t.contents.data, C.POINTER(Node)).contents for t in parts]
    layer = nodes[0].in_[0].contents
    assert (layer.type, layer.in_num, layer.out_num) == (pkg.OP_SPLIT, 1, 3)
    for i in range(3):
        assert C.addressof(layer.out[i].contents) == parts[i].contents.data
        assert C.addressof(nodes[i].in_[0].contents) == C.addressof(layer)
    assert C.addressof(layer.in_[0].contents) == t_in.contents.data
    fe.csinn_set_output(0, parts[0], sess)
    fe.csinn_set_output(1, t_sh, sess)
    assert fe.csinn_session_setup(sess) == pkg.CSINN_TRUE
    x = ssc._data(ssc._rng("host graph"), "int8", (1, 2, 3, 10))
    for _ in range(2):
        fe.csinn_update_input(0, pkg.make_tensor(fe, keep, x.shape, pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, data=x, sess=sess), sess)
        assert fe.csinn_session_run(sess) == pkg.CSINN_TRUE
        want = ssc.split_numpy(dict(x=x, axis=3, dtype="int8", lens=[4, 4, 2], in_q=ssc.Q_SAME, out_qs=recs))
        want_sh = ssc.shuffle_numpy(dict(x=want[2], group=2, dtype="int8", layout="NHWC", in_q=ssc.Q_A, out_q=ssc.Q_B))
        for i, w in enumerate((want[0], want_sh)):
            got = pkg.make_tensor(fe, keep, (1,), pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, sess=sess)
            fe.csinn_get_output(i, got, sess)
            data = np.ctypeslib.as_array(C.cast(got.contents.data, C.POINTER(C.c_int8)), (w.size,)).copy()
            fe.shl_mem_free(got.contents.data)
            assert np.array_equal(data.reshape(w.shape), w), "graph output %d" % i
    assert back.log == [("split", 3), ("shuffle", 2)] * 2
    fe.csinn_session_deinit(sess)
    fe.csinn_free_session(sess)


# ------------------------------------------------------------------------------------ kernel-form rules
def _fake_ptrs(case, skew_in=0, skew_out=None):
    """made-up, aligned, disjoint addresses: nothing is dereferenced"""
    n = case["n"] if case["op"] == "split" else 1
    return (1 << 40) + skew_in, [((i + 1) << 32) + (skew_out[i] if skew_out else 0) for i in range(n)]


def _name(hip, case, **kw):
    in_ptr, outs = _fake_ptrs(case, **kw)
    return ssc.cabi_args(case, outs).name(hip, in_ptr)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_name_picks_the_expected_form_and_honours_the_switch(built, case, monkeypatch):
    """pure host code: no device is initialised, no pointer is followed"""
    env = ssc.FORM_ENV[case["op"]]
    monkeypatch.delenv(env, raising=False)
    hip = pkg.load_hip()
    assert _name(hip, case) == ssc.expected_form(case)
    for force in ssc.other_forms(case):
        monkeypatch.setenv(env, force)
        assert _name(hip, case) == ssc.forced_form(case, force), force
    monkeypatch.setenv(env, "no such form")
    assert _name(hip, case) == ssc.expected_form(case)  # only the forms' names mean anything
    monkeypatch.delenv(env)
    # one element off the 16-byte grid, the input and separately each output: the literal form
    es = case["x"].itemsize
    n = case["n"] if case["op"] == "split" else 1
    assert _name(hip, case, skew_in=es) == ssc.expected_form(case, aligned=False)
    for i in range(min(n, 3)):
        assert _name(hip, case, skew_out=[es if j == i else 0 for j in range(n)]) == ssc.expected_form(case, aligned=False)


def test_every_form_is_exercised():
    seen = {(ssc.expected_form(c), c["dtype"]) for c in CASES}
    for form in ("split_vec", "split_generic", "shuffle_plane_16", "shuffle_plane_4", "shuffle_pixel_16", "shuffle_pixel_4",
                 "shuffle_generic"):
        for dtype in ("int8", "f16"):
            assert (form, dtype) in seen, (form, dtype)
    launches = {(ssc.expected_form(c), min((c["n"] + 7) // 8, 3)) for c in CASES if c["op"] == "split"}
    assert launches >= {(f, k) for f in ("split_vec", "split_generic") for k in (1, 2, 3)}


def test_shufflenet_v2_widths_take_the_pixel_form(built, monkeypatch):
    """116 / 232 / 464 int8 channels, two groups, NHWC: 116 and 232 are multiples of 4 bytes and not of 16, 464 is 29 x 16"""
    monkeypatch.delenv("SHL_MI355X_SHUFFLE_FORM", raising=False)
    hip = pkg.load_hip()
    for c, hw in ((116, 28), (232, 14), (464, 7)):
        for n in (1, 128):
            d = pkg.ShuffleDesc()
            d.dtype, d.group, d.outer, d.c, d.inner = pkg.SHL_I8, 2, n * hw * hw, c, 1
            d.in_scale = d.out_scale = 0.0625
            want = b"shuffle_pixel_16" if c % 16 == 0 else b"shuffle_pixel_4"
            assert hip.shl_mi355x_shuffle_channel_kernel_name(1 << 40, 1 << 41, C.byref(d)) == want


def test_invalid_arguments_are_refused_before_touching_the_device(built):
    hip = pkg.load_hip()
    x = np.arange(96, dtype=np.int8)
    outs = [np.full(64, POISON, np.uint8) for _ in range(2)]
    case = dict(op="split", x=x.reshape(3, 32), axis=1, dtype="int8", lens=[16, 16], n=2, in_q=(0.0625, -5), out_qs=[(0.0625, -5)] * 2)
    ptrs = [o.ctypes.data for o in outs]
    xin = x.ctypes.data

    def refused(args, in_ptr, text, call=None):
        rc = call() if call else args.run(hip, in_ptr)
        assert rc == EINVAL, (text, rc)
        assert text.encode() in hip.shl_mi355x_last_error(), (text, hip.shl_mi355x_last_error())
        if call is None:
            assert args.name(hip, in_ptr) == ""
    ok = ssc.SplitArgs(case, ptrs)
    assert ok.name(hip, xin) != ""
    refused(ok, None, "NULL argument")
    refused(ssc.SplitArgs(case, [ptrs[0], None]), xin, "NULL output")
    refused(ok, xin, "NULL argument", call=lambda: hip.shl_mi355x_split(xin, None, ok.len, ok.scale, ok.zp, C.byref(ok.desc), None))
    refused(ok, xin, "NULL argument", call=lambda: hip.shl_mi355x_split(xin, ok.ptrs, None, ok.scale, ok.zp, C.byref(ok.desc), None))
    refused(ok, xin, "NULL argument", call=lambda: hip.shl_mi355x_split(xin, ok.ptrs, ok.len, None, ok.zp, C.byref(ok.desc), None))
    refused(ok, xin, "NULL argument", call=lambda: hip.shl_mi355x_split(xin, ok.ptrs, ok.len, ok.scale, ok.zp, None, None))
    for field, value, text in (("n_outputs", 0, "n_outputs < 1"), ("dtype", 2, "dtype"), ("outer", -1, "negative outer")):
        bad = ssc.SplitArgs(case, ptrs)
        setattr(bad.desc, field, value)
        refused(bad, xin, text)
    for length in (0, -16):  # a chunk of length <= 0: dim 5 into 4 gives 2, 2, 2, -1
        bad = ssc.SplitArgs(case, ptrs)
        bad.len[1] = length
        refused(bad, xin, "length <= 0")
    # an output aliasing the input -- the same address, an overlap by the input's last byte -- and two outputs overlapping
    refused(ssc.SplitArgs(case, [ptrs[0], xin]), xin, "overlaps the input")
    refused(ssc.SplitArgs(case, [ptrs[0], xin + 95]), xin, "overlaps the input")
    refused(ssc.SplitArgs(case, [ptrs[0], ptrs[0] + 47]), xin, "two outputs overlap")
    assert ssc.SplitArgs(case, [ptrs[0], xin + 96]).name(hip, xin) != ""  # ... while one that begins where the input ends is fine
    # shuffle_channel
    scase = dict(op="shuffle", x=x.reshape(1, 2, 3, 16), dtype="int8", layout="NHWC", group=4, in_q=(0.0625, -5), out_q=(0.0625, -5))
    o = outs[0].ctypes.data
    sok = ssc.ShuffleArgs(scase, [o])
    assert sok.name(hip, xin) != ""
    refused(sok, None, "NULL argument")
    refused(ssc.ShuffleArgs(scase, [None]), xin, "NULL argument")
    refused(sok, xin, "NULL argument", call=lambda: hip.shl_mi355x_shuffle_channel(xin, o, None, None))
    for field, value, text in (("group", 0, "group < 1"), ("group", -2, "group < 1"), ("group", 3, "no multiple of group"),
                               ("group", 32, "no multiple of group"), ("dtype", 2, "dtype"), ("outer", -1, "outer < 0"),
                               ("c", 0, "c < 1"), ("inner", 0, "inner < 1")):
        bad = ssc.ShuffleArgs(scase, [o])
        setattr(bad.desc, field, value)
        refused(bad, xin, text)
    refused(ssc.ShuffleArgs(scase, [xin]), xin, "overlaps the input")
    refused(ssc.ShuffleArgs(scase, [xin + 95]), xin, "overlaps the input")
    assert all(np.all(v == POISON) for v in outs) and np.array_equal(x, np.arange(96, dtype=np.int8))


REFUSED_LAYERS = [
    # (what, case name, overrides of ssc.layer_run)
    ("per-channel quantised input", "null_index_10_into_3_i8", dict(in_scales=(0.5,) * 3)),
    ("an output of another dtype", "null_index_10_into_3_i8", dict(out_dt=pkg.DTYPE_FLOAT32)),
    ("output dims that do not match the rule", "null_index_10_into_3_i8", dict(out_shapes=[(2, 4, 3), (2, 3, 3), (2, 3, 3)])),
    ("a non-axis dim differs", "null_index_10_into_3_i8", dict(out_shapes=[(2, 4, 3), (2, 4, 3), (2, 2, 4)])),
    ("a last chunk of length <= 0: 10 into 6 gives 2 x 5 and 0", "null_index_10_into_3_i8",
     dict(out_shapes=[(2, 2, 3)] * 5 + [(2, 0, 3)])),
    ("a last chunk of length -1: 5 into 4", "count1_null_index_i8", dict(out_shapes=[(2, 2, 3)] * 3 + [(2, 1, 3)], count=4)),
    ("split_index not ascending", "given_index_ragged_i8", dict(index=[3, 3, 9])),
    ("split_index descending", "given_index_ragged_i8", dict(index=[4, 3, 9])),
    ("split_index out of range", "given_index_ragged_i8", dict(index=[3, 4, 10])),
    ("split_index negative", "given_index_ragged_i8", dict(index=[-1, 4, 9])),
    ("output_num 0", "null_index_10_into_3_i8", dict(count=0)),
    ("output_num -1", "null_index_10_into_3_i8", dict(count=-1)),
    ("axis out of range", "null_index_10_into_3_i8", dict(axis=3)),
    ("axis below -dim_count", "null_index_10_into_3_i8", dict(axis=-4)),
    ("C % group != 0", "nhwc_i8_c16_g2", dict(group=3)),
    ("group 0", "nhwc_i8_c16_g2", dict(group=0)),
    ("group -2", "nhwc_i8_c16_g2", dict(group=-2)),
    ("shuffle: per-channel quantised input", "nhwc_i8_c16_g2", dict(in_scales=(0.5,) * 16)),
    ("shuffle: an output of another dtype", "nhwc_i8_c16_g2", dict(out_dt=pkg.DTYPE_FLOAT32)),
    ("shuffle: output dims differ", "nhwc_i8_c16_g2", dict(out_shapes=[(1, 5, 3, 16)])),
]


@pytest.mark.parametrize("what,name,kw", REFUSED_LAYERS, ids=[r[0] for r in REFUSED_LAYERS])
def test_refused_layers_fail_in_the_callback_and_write_nothing(standalone, what, name, kw):
    """where the reference would read or write past a buffer; refused before anything is staged, so no device is needed"""
    fe, _, _ = standalone
    case = next(c for c in CASES if c["name"] == name)
    rc, outs = ssc.layer_run(fe, pkg.API_MI355X, case, poison=POISON, **kw)
    assert rc != pkg.CSINN_TRUE, what
    for o in outs:
        assert np.all(o.view(np.uint8) == POISON), what


def test_shuffle_of_a_tensor_that_is_not_4d_is_refused(standalone):
    fe, _, _ = standalone
    case = dict(op="shuffle", name="3d", dtype="int8", layout="NHWC", group=2, in_q=ssc.Q_SAME, out_q=ssc.Q_SAME,
                x=np.zeros((2, 3, 16), np.int8))
    rc, outs = ssc.layer_run(fe, pkg.API_MI355X, case, poison=POISON)
    assert rc != pkg.CSINN_TRUE and np.all(outs[0].view(np.uint8) == POISON)


def test_one_output_with_a_split_index_does_not_read_in_front_of_it(standalone):
    """the reference reads split_index[-1] (split.c:42-44); here output_num == 1 is the whole tensor whatever precedes the
    array: the perf callback accepts the layer and names a form"""
    fe, _, opt = standalone
    case = next(c for c in CASES if c["name"] == "count1_null_index_i8")
    names = []

    def perf(cb, t_in, outs, params):
        fn = C.CFUNCTYPE(C.c_int, TP, C.POINTER(TP), C.c_void_p, C.POINTER(C.c_char_p))(cb.contents.perf)
        name = C.c_char_p()
        assert fn(t_in, outs, params, C.byref(name)) == pkg.CSINN_TRUE
        names.append(name.value)
    guarded = (C.c_int32 * 3)(1 << 30, 7, 1 << 30)  # split_index points at the middle one
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, pkg.API_MI355X, keep)
    x = case["x"]
    t_in = pkg.make_tensor(fe, keep, x.shape, pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, data=x, scales=(case["in_q"][0],), zps=(case["in_q"][1],), sess=sess)
    t_out = pkg.make_tensor(fe, keep, x.shape, pkg.DTYPE_INT8, pkg.LAYOUT_NHWC, data=np.zeros_like(x), scales=(case["out_qs"][0][0],),
                            zps=(case["out_qs"][0][1],), sess=sess)
    params = pkg.split_params(fe, keep, pkg.API_MI355X, pkg.LAYOUT_NHWC, 1, 1, None, sess)
    pc = C.cast(params, C.POINTER(pkg.SplitParams)).contents
    pc.split_index = C.cast(C.addressof(guarded) + 4, C.POINTER(C.c_int32))
    outs = pkg.tensor_array(keep, [t_out])
    assert fe.csinn_split_init(t_in, outs, params) == pkg.CSINN_TRUE
    perf(pc.base.cb, t_in, outs, params)
    assert names == [b"split_generic"]


def test_perf_callbacks_name_the_kernel_form(standalone, monkeypatch):
    """split's perf callback has the array-of-outputs signature; both report the form the rules choose for host tensors,
    which the staging path aligns"""
    fe, hip, opt = standalone
    for env in ssc.FORM_ENV.values():
        monkeypatch.delenv(env, raising=False)
    opt.shl_cb_map_mi355x.restype = C.POINTER(pkg.Callback)
    opt.shl_cb_map_mi355x.argtypes = [C.c_int, C.c_int]
    for op in (pkg.OP_SPLIT, pkg.OP_SHUFFLE_CHANNEL):
        for dt in (pkg.DTYPE_INT8, pkg.DTYPE_FLOAT16):
            cb = opt.shl_cb_map_mi355x(op, dt)
            assert cb and cb.contents.perf and cb.contents.exec and cb.contents.est and cb.contents.init
    seen = []

    def perf(cb, t_in, outs, params):
        sig = [TP, C.POINTER(TP) if isinstance(outs, C.Array) else TP, C.c_void_p, C.POINTER(C.c_char_p)]
        name = C.c_char_p()
        assert C.CFUNCTYPE(C.c_int, *sig)(cb.contents.perf)(t_in, outs, params, C.byref(name)) == pkg.CSINN_TRUE
        seen.append(name.value.decode())
        raise StopIteration  # nothing is executed: no device is needed
    for name in ("form_i8_nhwc_16_32_48", "form_i8_nhwc_16_20", "form_f16_nhwc_8_24", "form_f16_nhwc_8_12", "nhwc_i8_c116_g2",
                 "nhwc_i8_c6_g2", "nchw_f16_2x4", "nchw_i8_2x2", "nhwc_f16_c8_g2"):
        case = next(c for c in CASES if c["name"] == name)
        with pytest.raises(StopIteration):
            ssc.layer_run(fe, pkg.API_MI355X, case, perf=perf)
        assert seen[-1] == ssc.expected_form(case), name
    assert set(seen) >= {"split_vec", "split_generic", "shuffle_pixel_4", "shuffle_pixel_16", "shuffle_plane_16", "shuffle_plane_4",
                         "shuffle_generic"}
    monkeypatch.setenv("SHL_MI355X_SHUFFLE_FORM", "generic")
    with pytest.raises(StopIteration):
        ssc.layer_run(fe, pkg.API_MI355X, case, perf=perf)
    assert seen[-1] == "shuffle_generic"


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
@pytest.mark.parametrize("dtype,layout", [("int8", "NHWC"), ("f16", "NCHW")])
@pytest.mark.parametrize("net", ["shufflenet", "c2f", "c2f_export"])
def test_oracle_chains_equal_the_genuine_graph_executor(net, dtype, layout):
    """the yardstick of tests/test_split_shuffle_session.py: both networks through the genuine front-end, graph executor and
    C kernels (CSINN_REF) give the oracle chain's answer: int8 bit for bit, binary16 within the project's 1e-3"""
    fe = cases.load_reference_frontend(local=True)
    fe.shl_debug_set_level(1)
    g = ssc.shufflenet(dtype, layout) if net == "shufflenet" else ssc.c2f(dtype, layout, export=net.endswith("export"))
    g.build(fe, pkg.API_REF)
    for k in (0, 1):
        x = g.input(k)
        got, want = g.run(fe, x), g.oracle(x)
        for name in g.outputs:
            what = "%s %s %s input %d, output %s" % (net, dtype, layout, k, name)
            if dtype == "int8":
                ssc.assert_same(got[name], want[name], what)
            else:  # the C oracle's binary16 convolution sums in another order than the library's: the project's 1e-3
                g32, w32 = got[name].astype(np.float32), want[name].astype(np.float32)
                assert np.all(np.abs(g32 - w32) <= 1e-3 * np.maximum(np.abs(w32), 1e-3)), what
    g.close(fe)

"""Shared helpers for split (CSINN_OP_SPLIT) and shuffle_channel (CSINN_OP_SHUFFLE_CHANNEL).

  split_cases() / shuffle_cases()   deterministic single-op problems, seeded by crc32(name): the smallest shapes at which each
                                    kernel form, the 8-outputs-per-launch chunking, every axis and every group count can
                                    still go wrong
  split_numpy / shuffle_numpy       plain numpy restatements of the reference (source/reference/split.c:21-92,
                                    shuffle_channel.c): dequantise with the input's record, move, requantise with the
                                    output's -- every split output with its own
  split_run / shuffle_run           csinn_<op>_init + csinn_<op> through a front-end (layer mode)
  SplitArgs / ShuffleArgs           what the C ABI takes, from a case and device addresses
  GraphNet, shufflenet(), c2f()     small networks through the csinn session API (graph mode) with an oracle replay:
                                    convolutions through the C oracle (cases.oracle_run), the rest through the numpy
                                    restatements
The genuine library's outputs for the cases live in tests/golden/split_shuffle_cases.npz (make_split_shuffle_golden.py).
"""
import ctypes as C
import os
import zlib

import numpy as np

import cases
import concat_cases
import pool_cases
import tail
from cases import pkg
from pool_cases import Q_CONV, Q_F16, Q_POW2, Q_SAME, Q_SAT, _q, assert_same, bits  # noqa: F401

Q_A, Q_B = _q(0.0311, 3), _q(0.0127, -20)   # two more converter-style records
Q_OUT_SAT = Q_SAT[1]                        # 2^-6, zero point 100: most values leave the int8 range
# every (input record, output records) set the int8 cases below use: the exhaustive cases walk all 256 values through each
RECORD_SETS = {
    "same": (Q_SAME, [Q_SAME, Q_CONV[0], Q_A]),                     # one raw copy, two requantised
    "conv": (Q_CONV[1], [Q_CONV[0], Q_A, Q_B, Q_CONV[1], Q_SAME]),  # all differing but one
    "pow2": (Q_POW2[1], [Q_POW2[0], Q_POW2[1]]),
    "pow2_up": (Q_POW2[0], [Q_POW2[1]]),
    "sat": (Q_SAME, [Q_OUT_SAT, Q_CONV[0]]),
    # the middle output's scale, 2^41, lies outside the [2^-40, 2^40] that requant_move.h:move_fma_ok admits: one launch
    # mixes outputs whose division may go through div_by_scale with one whose may not
    "fma_mixed": (Q_CONV[1], [Q_CONV[0], _q(2.0 ** 41, 0), Q_A]),
}


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _data(rng, dtype, shape, narrow=False):
    """narrow: sixteen distinct values only, so that the large cases' golden outputs compress"""
    if dtype == "int8":
        return rng.integers(-8, 8, shape, dtype=np.int8) if narrow else rng.integers(-128, 128, shape, dtype=np.int8)
    return (3.0 * rng.standard_normal(shape)).astype(np.float16)


def chunk_lens(dim, n, index=None):
    """the axis lengths of the n outputs (source/reference/split.c:38-61); index: the n - 1 boundaries"""
    if index is not None:
        edges = [0] + list(index[:n - 1]) + [dim]
        return [edges[i + 1] - edges[i] for i in range(n)]
    avg = (dim + n - 1) // n
    return [avg] * (n - 1) + [dim - avg * (n - 1)]


def _index_of(lens):
    return list(np.cumsum(lens)[:-1])


# ------------------------------------------------------------------------------------ cases
def split_cases():
    out = []

    def add(name, dtype, shape, axis, n=None, lens=None, in_q=None, out_qs=None, x=None, layout="NHWC", narrow=False):
        """lens given: split_index carries their boundaries; else split_index is NULL and n says how many outputs"""
        ax = axis if axis >= 0 else len(shape) + axis
        n = len(lens) if lens is not None else n
        # (one output: the reference reads split_index[-1] when it is given one, split.c:42-44, so it gets none)
        index = _index_of(lens) if lens is not None and n > 1 else None
        lens = chunk_lens(shape[ax], n, index)
        assert all(v > 0 for v in lens) and sum(lens) == shape[ax], name
        if dtype == "f16" or in_q is None:
            in_q, out_qs = (Q_F16[0], [Q_F16[0]] * n) if dtype == "f16" else (Q_SAME, [Q_SAME] * n)
        assert len(out_qs) == n, name
        if x is None:
            x = _data(_rng(name), dtype, shape, narrow)
        shapes = [tuple(shape[:ax]) + (v,) + tuple(shape[ax + 1:]) for v in lens]
        out.append(dict(op="split", name=name, dtype=dtype, layout=layout, axis=axis, n=n, index=index, lens=lens,
                        in_q=in_q, out_qs=list(out_qs), x=np.ascontiguousarray(x), out_shapes=shapes))

    recs = [Q_SAME, Q_CONV[0], Q_A]
    cyc = lambda n, k=0: [recs[(i + k) % 3] for i in range(n)]
    # ---- axes: every axis of a 4-d tensor, in both layouts; 2-d, 1-d, negative axes -------------------------------------
    for layout in ("NHWC", "NCHW"):
        add("axis0_%s_i8" % layout, "int8", (4, 3, 4, 4), 0, n=2, in_q=Q_SAME, out_qs=[Q_SAME, Q_CONV[0]], layout=layout)
        add("axis1_%s_f16" % layout, "f16", (2, 6, 2, 4), 1, lens=(2, 4), layout=layout)
        add("axis2_%s_i8" % layout, "int8", (2, 3, 6, 5), 2, n=3, in_q=Q_POW2[1], out_qs=[Q_POW2[0], Q_POW2[1], Q_POW2[0]],
            layout=layout)
        add("axis3_%s_i8" % layout, "int8", (1, 3, 5, 96), 3, lens=(16, 32, 48), in_q=Q_CONV[1], out_qs=[Q_CONV[0], Q_A, Q_B],
            layout=layout)
        add("axis3_%s_f16" % layout, "f16", (1, 3, 5, 32), 3, lens=(8, 24), layout=layout)
    add("axis_minus1_i8", "int8", (1, 3, 5, 32), -1, n=2)                                   # pure copy
    add("axis_minus3_f16", "f16", (2, 6, 2, 2), -3, n=3)
    add("axis_minus1_f16_2d", "f16", (3, 20), -1, lens=(8, 12))
    add("two_d_i8", "int8", (3, 48), 1, lens=(16, 32), in_q=Q_CONV[1], out_qs=[Q_CONV[0], Q_CONV[1]])
    add("two_d_i8_outer1", "int8", (1, 12), 1, lens=(5, 7), in_q=Q_CONV[1], out_qs=[Q_A, Q_B])
    add("one_d_i8", "int8", (64,), 0, lens=(16, 48), in_q=Q_SAME, out_qs=[Q_SAME, Q_CONV[0]])
    add("one_d_f16_null_index", "f16", (10,), 0, n=4)                                        # 3, 3, 3, 1
    # ---- split_index NULL: even and ragged tails ---------------------------------------------------------------------
    add("null_index_10_into_3_i8", "int8", (2, 10, 3), 1, n=3, in_q=Q_CONV[1], out_qs=cyc(3))   # 4, 4, 2
    add("null_index_7_into_4_f16", "f16", (2, 7), 1, n=4)                                       # 2, 2, 2, 1
    add("null_index_even_i8", "int8", (1, 2, 2, 64), 3, n=4, in_q=Q_SAME, out_qs=cyc(4))        # 16 each: the vector form
    add("given_index_ragged_i8", "int8", (2, 10, 3), 1, lens=(3, 1, 5, 1), in_q=Q_CONV[1], out_qs=cyc(4, 1))
    # ---- output counts: 9 and 17 cross the 8-per-launch chunking --------------------------------------------------------
    for n in (1, 2, 8, 9, 17):
        lens = [16 * (1 + i % 3) for i in range(n)]
        add("count%d_i8_vec" % n, "int8", (1, 2, 2, sum(lens)), 3, lens=lens, in_q=Q_SAME, out_qs=cyc(n))
        lens = [2 * (1 + i % 2) for i in range(n)]
        add("count%d_f16_vec" % n, "f16", (2, sum(lens), 2, 2), 1, lens=lens, layout="NCHW")
        lens = [1 + i % 4 for i in range(n)]
        add("count%d_i8_generic" % n, "int8", (1, 2, 2, sum(lens)), 3, lens=lens, in_q=Q_CONV[1], out_qs=cyc(n, 1))
        lens = [1 + i % 3 for i in range(n)]
        add("count%d_f16_generic" % n, "f16", (2, sum(lens), 3), 1, lens=lens)
    add("count1_null_index_i8", "int8", (2, 5, 3), 1, n=1, in_q=Q_CONV[1], out_qs=[Q_A])      # the whole tensor, requantised
    # ---- form boundaries: a length, an offset, or both off the 16-byte grid ------------------------------------------
    for cs in ((16, 16), (16, 32, 48), (16, 20), (20, 16), (3, 5)):
        add("form_i8_nhwc_" + "_".join(map(str, cs)), "int8", (1, 2, 3, sum(cs)), 3, lens=cs, in_q=Q_SAME, out_qs=cyc(len(cs)))
    for cs in ((8, 8), (8, 24), (8, 12)):
        add("form_f16_nhwc_" + "_".join(map(str, cs)), "f16", (1, 2, 3, sum(cs)), 3, lens=cs)
    add("nchw_channels_divisible_i8", "int8", (2, 6, 4, 4), 1, lens=(3, 1, 2), in_q=Q_SAME, out_qs=[Q_SAME, Q_CONV[0], Q_SAME],
        layout="NCHW")                                                                       # 48, 16, 32 bytes
    add("nchw_channels_indivisible_i8", "int8", (2, 8, 3, 3), 1, lens=(3, 5), in_q=Q_CONV[1], out_qs=[Q_CONV[0], Q_A],
        layout="NCHW")
    # ---- int8 records ------------------------------------------------------------------------------------------------
    three = dict(shape=(1, 3, 3, 64), axis=3, lens=(16, 16, 32))
    add("records_pure_copy", "int8", in_q=Q_SAME, out_qs=[Q_SAME] * 3, **three)
    add("records_one_differs", "int8", in_q=Q_SAME, out_qs=[Q_SAME, Q_CONV[0], Q_SAME], **three)
    add("records_all_differ", "int8", in_q=Q_CONV[1], out_qs=[Q_CONV[0], Q_A, Q_B], **three)
    add("records_saturating", "int8", in_q=Q_SAME, out_qs=[Q_SAME, Q_OUT_SAT, Q_CONV[0]], **three)
    add("records_all_differ_generic", "int8", (1, 3, 3, 24), 3, lens=(5, 16, 3), in_q=Q_CONV[1], out_qs=[Q_CONV[0], Q_A, Q_B])
    fma_mixed = dict(in_q=RECORD_SETS["fma_mixed"][0], out_qs=RECORD_SETS["fma_mixed"][1])  # one wave spans all three outputs
    add("records_fma_mixed_vec", "int8", (1, 2, 2, 64), 3, lens=(16, 32, 16), **fma_mixed)
    add("records_fma_mixed_generic", "int8", (1, 2, 2, 24), 3, lens=(5, 16, 3), **fma_mixed)
    every = np.arange(-128, 128, dtype=np.int16).astype(np.int8)
    for key, (in_q, outs) in RECORD_SETS.items():
        add("exhaustive_i8_" + key, "int8", (1, 256 * len(outs)), 1, lens=[256] * len(outs), in_q=in_q, out_qs=outs,
            x=np.tile(every, len(outs)).reshape(1, -1))
    # ---- binary16, exhaustive: all 65 536 bit patterns; the vector form by the rules, the literal form forced ----------
    patterns = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    beside = _data(_rng("f16 beside"), "f16", (8,))
    add("exhaustive_f16", "f16", (1, 65536 + 8), 1, lens=(32768, 8, 32768),
        x=np.concatenate([patterns[:32768], beside, patterns[32768:]]).reshape(1, -1))
    # ---- several workgroups per row ---------------------------------------------------------------------------------
    add("large_2x28x28x256_i8_nhwc", "int8", (2, 28, 28, 256), 3, n=4, in_q=Q_SAME, out_qs=[Q_SAME, Q_CONV[0], Q_A, Q_SAME],
        narrow=True)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def shuffle_cases():
    out = []

    def add(name, dtype, layout, shape, group, in_q=None, out_q=None, x=None, narrow=False):
        if dtype == "f16" or in_q is None:
            in_q, out_q = (Q_F16[0], Q_F16[0]) if dtype == "f16" else (Q_SAME, Q_SAME)
        c = shape[3] if layout == "NHWC" else shape[1]
        assert c % group == 0, name
        if x is None:
            x = _data(_rng(name), dtype, shape, narrow)
        out.append(dict(op="shuffle", name=name, dtype=dtype, layout=layout, group=group, in_q=in_q, out_q=out_q,
                        x=np.ascontiguousarray(x)))

    conv = (Q_CONV[1], Q_CONV[0])
    # ---- NHWC int8: both store widths of the pixel form, and the literal form ------------------------------------------
    for c, g in ((16, 2), (32, 2), (32, 4), (48, 3), (116, 2), (24, 3), (6, 2), (16, 1), (32, 8), (16, 16)):
        add("nhwc_i8_c%d_g%d" % (c, g), "int8", "NHWC", (1, 3, 5, c), g, *conv)
    # ---- NHWC binary16 -----------------------------------------------------------------------------------------------
    for c, g in ((8, 2), (24, 3), (6, 3), (3, 3)):
        add("nhwc_f16_c%d_g%d" % (c, g), "f16", "NHWC", (1, 3, 5, c), g)
    # ---- pixel counts: one, and one more than two workgroups' runs (one pass of 256 lanes: 4096 bytes of 16-byte pieces,
    # 256 pixels of 16 int8 channels, 128 of 16 binary16 ones); pixels longer than a pass, walked in several ------------
    add("nhwc_i8_one_pixel", "int8", "NHWC", (1, 1, 1, 16), 2, *conv)
    add("nhwc_i8_513_pixels", "int8", "NHWC", (1, 19, 27, 16), 4)
    add("nhwc_f16_257_pixels", "f16", "NHWC", (1, 1, 257, 16), 2)
    add("nhwc_i8_long_pixel_by4", "int8", "NHWC", (1, 1, 3, 1028), 2, *conv, narrow=True)     # 1028 bytes: 257 dwords
    add("nhwc_i8_long_pixel_by16", "int8", "NHWC", (1, 1, 2, 4112), 4, narrow=True)           # 4112 bytes: 257 pieces
    # ---- NCHW planes ------------------------------------------------------------------------------------------------
    add("nchw_i8_4x4", "int8", "NCHW", (2, 6, 4, 4), 3, *conv)       # 16-byte planes
    add("nchw_i8_2x2", "int8", "NCHW", (2, 4, 2, 2), 2, *conv)       # 4-byte planes
    add("nchw_i8_3x3", "int8", "NCHW", (2, 6, 3, 3), 2, *conv)       # the literal form
    add("nchw_f16_3x3", "f16", "NCHW", (2, 4, 3, 3), 4)
    add("nchw_f16_2x4", "f16", "NCHW", (2, 8, 2, 4), 2)              # 16-byte planes
    add("nchw_f16_1x2", "f16", "NCHW", (1, 6, 1, 2), 3)              # 4-byte planes
    add("nchw_i8_8x8_g1", "int8", "NCHW", (1, 4, 8, 8), 1)
    add("nchw_i8_1x1", "int8", "NCHW", (3, 16, 1, 1), 8, *conv)      # no plane to speak of: the pixel form
    # ---- int8 records ------------------------------------------------------------------------------------------------
    for key, (in_q, out_q) in (("pure_copy", (Q_SAME, Q_SAME)), ("differ", conv), ("pow2", Q_POW2), ("saturating", Q_SAT)):
        add("records_%s_nhwc" % key, "int8", "NHWC", (2, 3, 3, 32), 4, in_q, out_q)
        add("records_%s_nchw" % key, "int8", "NCHW", (2, 8, 4, 4), 4, in_q, out_q)
    every = np.arange(-128, 128, dtype=np.int16).astype(np.int8)
    for key, (in_q, outs) in RECORD_SETS.items():
        for i, out_q in enumerate(outs):
            add("exhaustive_i8_%s_%d" % (key, i), "int8", "NHWC", (1, 4, 4, 16), 4, in_q, out_q, x=every.reshape(1, 4, 4, 16))
    # ---- binary16, exhaustive: the pixel and the plane form by the rules, the literal form forced on both ---------------
    patterns = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    add("exhaustive_f16_nhwc", "f16", "NHWC", (1, 64, 128, 8), 2, x=patterns.reshape(1, 64, 128, 8))
    add("exhaustive_f16_nchw", "f16", "NCHW", (1, 8, 64, 128), 4, x=patterns.reshape(1, 8, 64, 128))
    # ---- several workgroups -------------------------------------------------------------------------------------------
    add("large_2x28x28x116_i8_nhwc", "int8", "NHWC", (2, 28, 28, 116), 2, *conv, narrow=True)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


# ------------------------------------------------------------------------------------ numpy restatements
def split_numpy(case):
    """every output of the split, each requantised with its own record"""
    x = case["x"]
    ax = case["axis"] if case["axis"] >= 0 else x.ndim + case["axis"]
    with np.errstate(all="ignore"):
        f = pool_cases.dequantise(x, case["dtype"], case["in_q"])
        outs, at = [], 0
        for length, q in zip(case["lens"], case["out_qs"]):
            piece = np.take(f, range(at, at + length), axis=ax)
            outs.append(np.ascontiguousarray(pool_cases.requantise(piece, case["dtype"], q)))
            at += length
    return outs


def shuffle_numpy(case):
    x, g = case["x"], case["group"]
    with np.errstate(all="ignore"):
        f = pool_cases.dequantise(x, case["dtype"], case["in_q"])
        if case["layout"] == "NHWC":
            n, h, w, c = f.shape
            f = f.reshape(n, h, w, g, c // g).transpose(0, 1, 2, 4, 3).reshape(n, h, w, c)
        else:
            n, c, h, w = f.shape
            f = f.reshape(n, g, c // g, h, w).transpose(0, 2, 1, 3, 4).reshape(n, c, h, w)
        out = pool_cases.requantise(np.ascontiguousarray(f), case["dtype"], case["out_q"])
    return np.ascontiguousarray(out)


def outputs_numpy(case):
    return split_numpy(case) if case["op"] == "split" else [shuffle_numpy(case)]


def all_cases():
    return split_cases() + shuffle_cases()


def golden_keys(case):
    n = case["n"] if case["op"] == "split" else 1
    return ["%s.%s#%d" % (case["op"], case["name"], i) for i in range(n)]


def golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_shuffle_cases.npz")
    blob = np.load(path)
    return {k: blob[k] for k in blob.files}


def _layout(case):
    return pkg.LAYOUT_NHWC if case["layout"] == "NHWC" else pkg.LAYOUT_NCHW


def _np_dtype(case):
    return np.int8 if case["dtype"] == "int8" else np.float16


# ------------------------------------------------------------------------------------ through csinn_*
def layer_run(fe, api, case, device=None, poison=None, out_shapes=None, axis=None, count=None, index=False, group=None,
              in_scales=None, out_dt=None, perf=None):
    """layer mode through csinn_split / csinn_shuffle_channel (+ _init).  device: a cases.HipDevice -- every tensor then is a
    DMABUF tensor in HBM.  Returns the list of outputs, or (status, outputs) when `poison` (a byte the outputs are
    pre-filled with) is given.  out_shapes / axis / count / index / group / in_scales / out_dt override what the case says
    (refusal tests).  perf: a callable (callback block, input, outputs, params) run between init and exec."""
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, api, keep)
    int8 = case["dtype"] == "int8"
    dt = pkg.DTYPE_INT8 if int8 else pkg.DTYPE_FLOAT16
    layout = _layout(case)
    split = case["op"] == "split"
    x = case["x"]
    shapes = out_shapes or (case["out_shapes"] if split else [x.shape])
    out_qs = case["out_qs"] if split else [case["out_q"]]
    out_qs = list(out_qs) + [out_qs[-1]] * (len(shapes) - len(out_qs))
    allocs = []

    def place(arr):
        if device is None:
            return None
        p = device.alloc(arr.nbytes)
        device.upload(p, arr)
        allocs.append(p)
        return p
    s, z = case["in_q"]
    t_in = pkg.make_tensor(fe, keep, x.shape, dt, layout, data=x, scales=in_scales or (s,), zps=(z,), name=b"in", sess=sess,
                           device_ptr=place(x))
    outs, t_outs, ptrs = [], [], []
    for i, shape in enumerate(shapes):
        o = np.zeros(shape, dtype=x.dtype)
        o.view(np.uint8)[...] = poison if poison is not None else 0
        ptrs.append(place(o))
        outs.append(o)
        t_outs.append(pkg.make_tensor(fe, keep, shape, out_dt or dt, layout, data=o, scales=(out_qs[i][0],), zps=(out_qs[i][1],),
                                      name=b"out%d" % i, sess=sess, device_ptr=ptrs[-1]))
    if split:
        idx = case["index"] if index is False else index
        params = pkg.split_params(fe, keep, api, layout, len(shapes) if count is None else count,
                                  case["axis"] if axis is None else axis, idx, sess)
        args = (t_in, pkg.tensor_array(keep, t_outs), params)
        stem = "csinn_split"
    else:
        params = pkg.shuffle_channel_params(fe, keep, api, layout, case["group"] if group is None else group, sess)
        args = (t_in, t_outs[0], params)
        stem = "csinn_shuffle_channel"
    rc = getattr(fe, stem + "_init")(*args)
    if rc == pkg.CSINN_TRUE and perf is not None:
        perf(C.cast(params, C.POINTER(pkg.ParamsBase)).contents.cb, *args)
    if rc == pkg.CSINN_TRUE:
        rc = getattr(fe, stem)(*args)
    if device is not None:
        outs = [device.download(p, o.shape, o.dtype) for p, o in zip(ptrs, outs)]
        for p in allocs:
            device.free(p)
    if poison is not None:
        return rc, outs
    if rc != pkg.CSINN_TRUE:
        raise pkg.MI355XError("%s returned %d" % (stem, rc))
    return outs


class SplitArgs:
    """the arrays shl_mi355x_split takes, from a case and the addresses of its outputs"""

    def __init__(self, case, out_ptrs):
        n = len(out_ptrs)
        x = case["x"]
        ax = case["axis"] if case["axis"] >= 0 else x.ndim + case["axis"]
        inner = int(np.prod(x.shape[ax + 1:], dtype=np.int64))
        self.ptrs = (C.c_void_p * n)(*out_ptrs)
        self.len = (C.c_int64 * n)(*[v * inner for v in case["lens"]])
        self.scale = (C.c_float * n)(*[q[0] for q in case["out_qs"]])
        self.zp = (C.c_int32 * n)(*[q[1] for q in case["out_qs"]])
        d = pkg.SplitDesc()
        d.dtype = pkg.SHL_I8 if case["dtype"] == "int8" else pkg.SHL_F16
        d.n_outputs = n
        d.outer = int(np.prod(x.shape[:ax], dtype=np.int64))
        d.in_scale, d.in_zp = case["in_q"]
        self.desc = d

    def name(self, hip, in_ptr):
        return hip.shl_mi355x_split_kernel_name(in_ptr, self.ptrs, self.len, self.scale, self.zp, C.byref(self.desc)).decode()

    def run(self, hip, in_ptr, stream=None):
        return hip.shl_mi355x_split(in_ptr, self.ptrs, self.len, self.scale, self.zp, C.byref(self.desc), stream)


class ShuffleArgs:
    """the descriptor shl_mi355x_shuffle_channel takes, from a case and the address of its output"""

    def __init__(self, case, out_ptrs):
        self.out = out_ptrs[0]
        x = case["x"]
        d = pkg.ShuffleDesc()
        d.dtype = pkg.SHL_I8 if case["dtype"] == "int8" else pkg.SHL_F16
        d.group = case["group"]
        if case["layout"] == "NHWC":
            d.outer, d.c, d.inner = x.shape[0] * x.shape[1] * x.shape[2], x.shape[3], 1
        else:
            d.outer, d.c, d.inner = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
        d.in_scale, d.in_zp = case["in_q"]
        d.out_scale, d.out_zp = case["out_q"]
        self.desc = d

    def name(self, hip, in_ptr):
        return hip.shl_mi355x_shuffle_channel_kernel_name(in_ptr, self.out, C.byref(self.desc)).decode()

    def run(self, hip, in_ptr, stream=None):
        return hip.shl_mi355x_shuffle_channel(in_ptr, self.out, C.byref(self.desc), stream)


def cabi_args(case, out_ptrs):
    return (SplitArgs if case["op"] == "split" else ShuffleArgs)(case, out_ptrs)


FORM_ENV = {"split": "SHL_MI355X_SPLIT_FORM", "shuffle": "SHL_MI355X_SHUFFLE_FORM"}


def expected_form(case, aligned=True):
    """the form the documented rules give a case whose buffers are 16-byte aligned (aligned=False: one of them is not, by one
    element)"""
    es = 1 if case["dtype"] == "int8" else 2
    x = case["x"]
    if case["op"] == "split":
        ax = case["axis"] if case["axis"] >= 0 else x.ndim + case["axis"]
        inner = int(np.prod(x.shape[ax + 1:], dtype=np.int64))
        return "split_vec" if aligned and all(v * inner * es % 16 == 0 for v in case["lens"]) else "split_generic"
    if case["layout"] == "NHWC" or x.shape[2] * x.shape[3] == 1:
        unit, kind = (x.shape[3] if case["layout"] == "NHWC" else x.shape[1]) * es, "pixel"
    else:
        unit, kind = x.shape[2] * x.shape[3] * es, "plane"
    if not aligned or (kind == "pixel" and unit > 8192):  # (one element is 1 or 2 bytes: off the 4-byte grid too)
        return "shuffle_generic"
    if unit % 16 == 0:
        return "shuffle_%s_16" % kind
    if unit % 4 == 0:
        return "shuffle_%s_4" % kind
    return "shuffle_generic"


def other_forms(case):
    """the values of the force switch that make sense for a case, besides leaving it unset"""
    if case["op"] == "split":
        return ["generic", "vec"]
    return ["generic", "plane", "pixel"]


def forced_form(case, force):
    """the form a forced call takes: the forced one where the arguments admit it, else generic"""
    natural = expected_form(case)
    if force == "generic":
        return natural.split("_")[0] + "_generic"
    return natural if ("_" + force) in natural else natural.split("_")[0] + "_generic"


# ------------------------------------------------------------------------------------ networks that divide a tensor
class GraphNet:
    """A small network given as a list of layers over named tensors, run two ways: through the csinn session API in graph
    mode, and as an oracle chain -- convolutions through the C oracle (cases.oracle_run), everything else through the numpy
    restatements.  cut=True builds THE SAME GRAPH WITHOUT ITS SPLIT AND SHUFFLE LAYERS: each one's input becomes a graph
    output and its outputs graph inputs, so that the fusion planner's counts can be compared (that graph is built, never
    run).

    layers: (kind, name, inputs, outputs, info) with kind conv (info: act 0 | 1 fused, k, stride, depthwise, k_log2), relu,
    split, concat, shuffle (info: group), gap, softmax.  tensors: name -> (channels, height, record)."""

    def __init__(self, dtype, layout, seed, in_name, tensors, layers, outputs, cut=False):
        self.dtype, self.layout, self.cut = dtype, layout, cut
        self.in_name, self.tensors, self.layers, self.outputs = in_name, tensors, layers, list(outputs)
        int8 = dtype == "int8"
        rng = np.random.default_rng(seed)
        self.cv = {}
        for kind, name, ins, outs, info in layers:
            if kind != "conv":
                continue
            cin, hin, q_prev = self.tensors[ins[0]]
            cout, _, out_q = self.tensors[outs[0]]
            k = info.get("k", 1)
            case = cases.make_case(int(rng.integers(1 << 30)), layout=layout, dtype=dtype, n=1, h=hin, w=hin, c=cin, co=cout,
                                   k=(k, k), stride=(info.get("stride", 1),) * 2, pad=(k // 2,) * 4, act=info.get("act", 0),
                                   depthwise=info.get("depthwise", False))
            if int8:
                case["in_scale"], case["in_zp"] = q_prev
                case["k_scale"] = np.array([2.0 ** info.get("k_log2", -7)], dtype=np.float32)
                case["b_scale"] = (np.float32(case["in_scale"]) * case["k_scale"]).astype(np.float32)
                case["bias"] = rng.integers(-2000, 2001, (case["co"],), dtype=np.int32)
                case["out_scale"], case["out_zp"] = out_q
            self.cv[name] = case

    def rec(self, name):
        return self.tensors[name][2] if self.dtype == "int8" else _q(1.0, 0)

    def shape(self, name):
        c, h, _ = self.tensors[name]
        return (1, h, h, c) if self.layout == "NHWC" else (1, c, h, h)

    @property
    def c_axis(self):
        return 3 if self.layout == "NHWC" else 1

    def input(self, k):
        rng = np.random.default_rng(900 + k)
        shape = self.shape(self.in_name)
        return rng.integers(-100, 100, shape, dtype=np.int8) if self.dtype == "int8" else rng.standard_normal(shape).astype(np.float16)

    # -- the oracle chain: every named tensor
    def oracle(self, x):
        env = {self.in_name: x}
        form = "ref" if self.dtype == "int8" else "f16"
        for kind, name, ins, outs, info in self.layers:
            a = env[ins[0]]
            if kind == "conv":
                case = dict(self.cv[name])
                case["input"] = np.ascontiguousarray(a)
                env[outs[0]] = cases.oracle_run(case, form)
            elif kind == "split":
                lens = [self.tensors[o][0] for o in outs]
                got = split_numpy(dict(x=a, axis=self.c_axis, dtype=self.dtype, lens=lens, in_q=self.rec(ins[0]),
                                       out_qs=[self.rec(o) for o in outs]))
                env.update(zip(outs, got))
            elif kind == "shuffle":
                env[outs[0]] = shuffle_numpy(dict(x=a, group=info["group"], dtype=self.dtype, layout=self.layout,
                                                  in_q=self.rec(ins[0]), out_q=self.rec(outs[0])))
            elif kind == "concat":
                xs = [env[i] for i in ins]
                env[outs[0]] = concat_cases.concat_numpy(dict(dtype=self.dtype, axis=self.c_axis, xs=xs, in_qs=[self.rec(i) for i in ins],
                                                              out_q=self.rec(outs[0]), out_shape=xs[0].shape))
            else:
                what = {"relu": "relu", "gap": "pool", "softmax": "softmax"}[kind]
                env[outs[0]] = tail.siso_oracle(dict(kind=what, x=a, dtype=self.dtype, layout=self.layout, axis=self.c_axis,
                                                     in_q=self.rec(ins[0]), out_q=self.rec(outs[0])))
        return env

    def build(self, fe, api):
        keep = pkg.Keep()
        sess = fe.csinn_alloc_session()
        sc = sess.contents
        int8 = self.dtype == "int8"
        dt = pkg.DTYPE_INT8 if int8 else pkg.DTYPE_FLOAT16
        sc.base_api, sc.base_run_mode, sc.base_dtype = api, pkg.RM_CPU_GRAPH, dt
        sc.base_quant_type = pkg.QUANT_INT8_ASYM_W_SYM if int8 else pkg.QUANT_FLOAT16
        sc.debug_level = 0
        fe.csinn_session_init(sess)
        nhwc = self.layout == "NHWC"
        act_l = pkg.LAYOUT_NHWC if nhwc else pkg.LAYOUT_NCHW

        def T(dims, rec, name, data=None, const=0, layout=act_l, dtype=dt, scales=None):
            return pkg.make_tensor(fe, keep, dims, dtype, layout, data=data, is_const=const, name=name, sess=sess,
                                   scales=scales if scales is not None else (rec[0],), zps=(rec[1] if rec else 0,))
        env = {self.in_name: T(self.shape(self.in_name), self.rec(self.in_name), self.in_name.encode())}
        ops, inputs, outputs = [], [env[self.in_name]], []
        for kind, name, ins, outs, info in self.layers:
            for o in outs:
                env[o] = T(self.shape(o), self.rec(o), o.encode())
            nm = name.encode()
            if kind in ("split", "shuffle") and self.cut:
                outputs.append(env[ins[0]])
                inputs.extend(env[o] for o in outs)
            elif kind == "conv":
                case = self.cv[name]
                if case["depthwise"]:
                    w_l = pkg.LAYOUT_1HWO if nhwc else pkg.LAYOUT_O1HW
                else:
                    w_l = pkg.LAYOUT_OHWI if nhwc else pkg.LAYOUT_OIHW
                t_w = T(case["w_shape"], None, nm + b"_w", case["kernel"], 1, w_l, scales=tuple(case["k_scale"]))
                t_b = T((case["co"],), None, nm + b"_b", case["bias"], 1, pkg.LAYOUT_O, pkg.DTYPE_INT32 if int8 else dt,
                        scales=tuple(case["b_scale"]))
                p = pkg.conv_params(fe, keep, api, act_l, case["stride"], case["pad"], case["dilation"], case["group"], 0, sess, nm)
                ops.append(("csinn_conv2d_relu" if case["act"] else "csinn_conv2d", (env[ins[0]], env[outs[0]], t_w, t_b, p)))
            elif kind == "split":
                # (the boundaries are given, as a converter gives them: the genuine graph executor saves the model at
                # setup and copies output_num entries of split_index, NULL or not)
                index = _index_of([self.tensors[o][0] for o in outs])
                p = pkg.split_params(fe, keep, api, act_l, len(outs), self.c_axis, index, sess, nm)
                ops.append(("csinn_split", (env[ins[0]], pkg.tensor_array(keep, [env[o] for o in outs]), p)))
            elif kind == "shuffle":
                p = pkg.shuffle_channel_params(fe, keep, api, act_l, info["group"], sess, nm)
                ops.append(("csinn_shuffle_channel", (env[ins[0]], env[outs[0]], p)))
            elif kind == "concat":
                p = pkg.concat_params(fe, keep, api, act_l, len(ins), self.c_axis, sess, nm)
                ops.append(("csinn_concat", (pkg.tensor_array(keep, [env[i] for i in ins]), env[outs[0]], p)))
            else:
                what = {"relu": "relu", "gap": "pool", "softmax": "softmax"}[kind]
                stem = {"relu": "csinn_relu", "gap": "csinn_global_avgpool2d", "softmax": "csinn_softmax"}[kind]
                ops.append((stem, (env[ins[0]], env[outs[0]], pkg.siso_params(fe, keep, api, what, act_l, self.c_axis, sess, nm))))
        outputs.extend(env[o] for o in self.outputs)
        fe.csinn_set_input_number(len(inputs), sess)
        fe.csinn_set_output_number(len(outputs), sess)
        for stem, args in ops:
            assert getattr(fe, stem + "_init")(*args) == pkg.CSINN_TRUE, stem
        for i, t in enumerate(inputs):
            fe.csinn_set_tensor_entry(t, sess)
            fe.csinn_set_input(i, t, sess)
        for stem, args in ops:
            assert getattr(fe, stem)(*args) == pkg.CSINN_TRUE, stem
        for i, t in enumerate(outputs):
            fe.csinn_set_output(i, t, sess)
        rc = fe.csinn_session_setup(sess)
        assert rc == pkg.CSINN_TRUE or getattr(fe, "kind", "") == "reference"
        self._keep, self._sess, self.layer_count = keep, sess, len(ops)
        return sess

    def run(self, fe, x):
        """one run on host buffers; returns {graph output name: array}"""
        keep, sess = self._keep, self._sess
        int8 = self.dtype == "int8"
        dt = pkg.DTYPE_INT8 if int8 else pkg.DTYPE_FLOAT16
        act_l = pkg.LAYOUT_NHWC if self.layout == "NHWC" else pkg.LAYOUT_NCHW
        q = self.rec(self.in_name)
        feed = pkg.make_tensor(fe, keep, x.shape, dt, act_l, data=x, sess=sess, scales=(q[0],), zps=(q[1],))
        fe.csinn_update_input(0, feed, sess)
        assert fe.csinn_session_run(sess) == pkg.CSINN_TRUE
        res = {}
        for i, name in enumerate(self.outputs):
            got = pkg.make_tensor(fe, keep, (1,), dt, act_l, sess=sess)
            fe.csinn_get_output(i, got, sess)
            shape = self.shape(name)
            ctype = C.c_int8 if int8 else C.c_uint16
            data = np.ctypeslib.as_array(C.cast(got.contents.data, C.POINTER(ctype)), (int(np.prod(shape)),)).copy()
            fe.shl_mem_free(got.contents.data)  # graph outputs belong to the caller after a run
            res[name] = data.reshape(shape) if int8 else data.view(np.float16).reshape(shape)
        return res

    close = tail.MiniNet.close


def shufflenet(dtype="int8", layout="NHWC", cut=False, classes=24):
    """16x16x16 -> stem conv3x3 s2 (16 @8x8) -> one basic ShuffleNetV2 unit: split(2); the right half through pw + relu (a
    relu LAYER, which a session folds) -> dw3x3 -> pw+relu; concat; shuffle_channel(2) -> one down-sampling unit: both
    branches read the same tensor, a depthwise 3x3 stride 2 in each; concat (32 @4x4); shuffle_channel(2) ->
    global_avgpool -> 1x1 classifier -> softmax"""
    q = lambda s, z: _q(2.0 ** s, z)
    t = {"data": (16, 16, q(-4, -5)), "stem": (16, 8, q(-3, -100)),
         "left": (8, 8, q(-3, -100)), "right": (8, 8, q(-4, -90)),             # the left half is a copy, the right is requantised
         "r1c": (8, 8, q(-3, -100)), "r1": (8, 8, q(-3, -100)), "r2": (8, 8, q(-3, -10)), "r3": (8, 8, q(-4, -110)),
         "cat1": (16, 8, q(-3, -100)), "shuf1": (16, 8, q(-3, -100)),
         "l1": (16, 4, q(-3, -20)), "l2": (16, 4, q(-3, -120)),
         "d1": (16, 8, q(-3, -100)), "d2": (16, 4, q(-3, 5)), "d3": (16, 4, q(-4, -128)),
         "cat2": (32, 4, q(-3, -120)), "shuf2": (32, 4, q(-4, -110)),         # the second shuffle requantises
         "gap": (32, 1, q(-5, -128)), "fc": (classes, 1, q(-4, -11)), "prob": (classes, 1, _q(1.0 / 256, -128))}
    L = [("conv", "stem", ["data"], ["stem"], dict(k=3, stride=2, act=1)),
         ("split", "split1", ["stem"], ["left", "right"], {}),
         ("conv", "r1", ["right"], ["r1c"], dict(act=0)),
         ("relu", "r1_relu", ["r1c"], ["r1"], {}),
         ("conv", "r2", ["r1"], ["r2"], dict(k=3, depthwise=True, k_log2=-5)),
         ("conv", "r3", ["r2"], ["r3"], dict(act=1)),
         ("concat", "cat1", ["left", "r3"], ["cat1"], {}),
         ("shuffle", "shuf1", ["cat1"], ["shuf1"], dict(group=2)),
         ("conv", "l1", ["shuf1"], ["l1"], dict(k=3, stride=2, depthwise=True, k_log2=-5)),
         ("conv", "l2", ["l1"], ["l2"], dict(act=1)),
         ("conv", "d1", ["shuf1"], ["d1"], dict(act=1)),
         ("conv", "d2", ["d1"], ["d2"], dict(k=3, stride=2, depthwise=True, k_log2=-5)),
         ("conv", "d3", ["d2"], ["d3"], dict(act=1)),
         ("concat", "cat2", ["l2", "d3"], ["cat2"], {}),
         ("shuffle", "shuf2", ["cat2"], ["shuf2"], dict(group=2)),
         ("gap", "gap", ["shuf2"], ["gap"], {}),
         ("conv", "fc", ["gap"], ["fc"], dict(k_log2=-9)),
         ("softmax", "softmax", ["fc"], ["prob"], {})]
    return GraphNet(dtype, layout, 41, "data", t, L, ["prob"], cut=cut)


def c2f(dtype="int8", layout="NHWC", cut=False, export=False):
    """8x8x16 -> conv1x1 (32) + a relu LAYER -> split(2) -> the second half feeds a conv3x3+relu AND the final concat of three
    (so that split output has two consumers) -> conv1x1+relu (32).  export=True: the second half is a graph output too"""
    q = lambda s, z: _q(2.0 ** s, z)
    t = {"data": (16, 8, q(-4, -5)), "cv1c": (32, 8, q(-3, -100)), "cv1": (32, 8, q(-3, -100)),
         "a": (16, 8, q(-3, -100)), "b": (16, 8, q(-4, -80)), "m": (16, 8, q(-3, -110)),
         "cat": (48, 8, q(-3, -100)), "out": (32, 8, q(-3, -90))}
    L = [("conv", "cv1", ["data"], ["cv1c"], dict(act=0)),
         ("relu", "cv1_relu", ["cv1c"], ["cv1"], {}),
         ("split", "split", ["cv1"], ["a", "b"], {}),
         ("conv", "m", ["b"], ["m"], dict(k=3, act=1)),
         ("concat", "cat", ["a", "b", "m"], ["cat"], {}),
         ("conv", "cv2", ["cat"], ["out"], dict(act=1))]
    return GraphNet(dtype, layout, 43, "data", t, L, ["out", "b"] if export else ["out"], cut=cut)

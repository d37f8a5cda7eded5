"""Shared helpers for concat (CSINN_OP_CONCAT).

  concat_cases()                deterministic single-op problems: the smallest shapes at which each kernel form (16 bytes
                                per thread, one element per thread), the 8-inputs-per-launch chunking and every axis can
                                still go wrong
  concat_numpy(case)            plain numpy restatement of the reference (source/reference/concat.c:21-76): every input
                                dequantised with its own record, slabs copied, the result requantised with the output's
  concat_run(fe, api, case)     csinn_concat_init + csinn_concat through a front-end (layer mode)
  BranchNet                     conv -> Fire module -> concat -> maxpool -> Inception block of four branches -> concat ->
                                global_avgpool -> classifier -> softmax through the csinn session API (graph mode), with an
                                oracle replay
The genuine library's outputs for concat_cases() live in tests/golden/concat_cases.npz (make_concat_golden.py).
"""
import ctypes as C
import os
import zlib

import numpy as np

import cases
import pool_cases
import tail
from cases import pkg
from pool_cases import Q_CONV, Q_F16, Q_POW2, Q_SAME, Q_SAT, _q, assert_same, bits  # noqa: F401

OP = pkg.OP_CONCAT                         # the op under test (26 in the reference's enum)
Q_A, Q_B = _q(0.0311, 3), _q(0.0127, -20)   # two more converter-style input records
Q_OUT_SAT = Q_SAT[1]                        # 2^-6, zero point 100: most values leave the int8 range
# every (input record, output record) pair the cases below use: the exhaustive cases walk all 256 values through each
RECORD_PAIRS = {
    "same": ([Q_SAME, Q_CONV[0], Q_A], Q_SAME),                     # one raw copy, two requantised
    "conv": ([Q_CONV[0], Q_A, Q_B, Q_CONV[1], Q_SAME], Q_CONV[1]),  # all differing but one
    "pow2": ([Q_POW2[0], Q_POW2[1]], Q_POW2[1]),
    "sat": ([Q_SAME, Q_CONV[0]], Q_OUT_SAT),
    # (128 + |zp|) s = 2^61 for the 2^54 record, past the 2^60 that requant_move.h:move_fma_ok admits: one launch mixes
    # inputs whose division may go through div_by_scale with one whose may not
    "fma_mixed": ([Q_CONV[0], _q(2.0 ** 54, 0), Q_A], Q_SAME),
}


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _data(rng, dtype, shape):
    if dtype == "int8":
        return rng.integers(-128, 128, shape, dtype=np.int8)
    return (3.0 * rng.standard_normal(shape)).astype(np.float16)


def _with_axis(shape, axis, n):
    s = list(shape)
    s[axis] = n
    return tuple(s)


def concat_cases():
    out = []

    def add(name, dtype, shapes, axis, in_qs=None, out_q=None, xs=None, alias=None):
        """shapes: one per input; alias[i]: which DISTINCT tensor input i is (the same tensor may be given twice)"""
        n = len(shapes)
        alias = list(alias) if alias is not None else list(range(n))
        if dtype == "f16" or in_qs is None:
            in_qs, out_q = ([Q_F16[0]] * n, Q_F16[0]) if dtype == "f16" else ([Q_SAME] * n, Q_SAME)
        assert len(in_qs) == n
        rng = _rng(name)
        if xs is None:
            uniq = {}
            for i in range(n):
                if alias[i] not in uniq:
                    uniq[alias[i]] = _data(rng, dtype, shapes[i])
            xs = [uniq[alias[i]] for i in range(n)]
        ax = axis if axis >= 0 else len(shapes[0]) + axis
        out_shape = _with_axis(shapes[0], ax, sum(s[ax] for s in shapes))
        for i in range(n):
            assert xs[i].shape == tuple(shapes[i]) and _with_axis(shapes[i], ax, 0) == _with_axis(out_shape, ax, 0), name
            assert in_qs[i] == in_qs[alias.index(alias[i])], name  # one tensor, one record
        out.append(dict(name=name, dtype=dtype, axis=axis, shapes=[tuple(s) for s in shapes], in_qs=list(in_qs),
                        out_q=out_q, xs=[np.ascontiguousarray(x) for x in xs], alias=alias, out_shape=out_shape))

    def chans(base, axis, cs):
        return [_with_axis(base, axis, c) for c in cs]

    mixed = ([Q_SAME, Q_CONV[0], Q_SAME], Q_SAME)             # raw and requantised inputs in one launch
    differ = ([Q_CONV[0], Q_A, Q_B], Q_CONV[1])               # all differing, converter scales
    # ---- axes ------------------------------------------------------------------------------------------------
    nhwc = (1, 3, 5, 0)
    add("axis3_nhwc_i8_16_32_48", "int8", chans(nhwc, 3, (16, 32, 48)), 3, *differ)          # vector form, outer 15
    add("axis3_nhwc_f16_8_24", "f16", chans(nhwc, 3, (8, 24)), 3)
    add("axis1_nchw_i8_divisible", "int8", chans((2, 0, 4, 4), 1, (3, 1, 2)), 1, *mixed)     # C H W = 48, 16, 32 bytes
    add("axis1_nchw_i8_indivisible", "int8", chans((2, 0, 3, 3), 1, (3, 5)), 1, [Q_CONV[0], Q_A], Q_CONV[1])
    add("axis1_nchw_f16_divisible", "f16", chans((2, 0, 2, 2), 1, (2, 4, 6)), 1)             # 16, 32, 48 bytes
    add("axis1_nchw_f16_indivisible", "f16", chans((2, 0, 3, 3), 1, (2, 1)), 1)              # 36, 18 bytes
    add("axis0_outer1_i8", "int8", chans((0, 3, 4, 4), 0, (2, 1)), 0, [Q_SAME, Q_CONV[0]], Q_SAME)
    add("axis0_outer1_f16", "f16", chans((0, 3, 3, 3), 0, (2, 1, 3)), 0)                     # 108, 54, 162 bytes: generic
    add("axis2_i8", "int8", chans((2, 3, 0, 5), 2, (4, 2)), 2, [Q_POW2[0], Q_POW2[1]], Q_POW2[1])
    add("axis2_f16_vec", "f16", chans((2, 3, 0, 8), 2, (1, 3)), 2)
    add("axis_minus1_i8", "int8", chans(nhwc, 3, (16, 16)), -1, [Q_SAME, Q_SAME], Q_SAME)    # pure copy
    add("axis_minus1_f16_2d", "f16", [(3, 8), (3, 12)], -1)
    add("two_d_i8", "int8", [(3, 16), (3, 32)], 1, [Q_CONV[0], Q_CONV[1]], Q_CONV[1])
    add("two_d_i8_outer1", "int8", [(1, 5), (1, 7)], 1, [Q_A, Q_B], Q_CONV[1])
    add("one_d_i8", "int8", [(16,), (48,)], 0, [Q_SAME, Q_CONV[0]], Q_SAME)
    # ---- input counts: 9 and 17 cross the 8-per-launch chunking ---------------------------------------------
    recs = [Q_SAME, Q_CONV[0], Q_A]
    for n in (1, 2, 4, 8, 9, 17):
        add("count%d_i8_vec" % n, "int8", chans((1, 2, 2, 0), 3, [16 * (1 + i % 3) for i in range(n)]), 3,
            [recs[i % 3] for i in range(n)], Q_SAME)
        add("count%d_f16_vec" % n, "f16", chans((2, 0, 2, 2), 1, [2 * (1 + i % 2) for i in range(n)]), 1)
    for n in (1, 8, 9, 17):
        add("count%d_i8_generic" % n, "int8", chans((1, 2, 2, 0), 3, [1 + i % 4 for i in range(n)]), 3,
            [recs[(i + 1) % 3] for i in range(n)], Q_CONV[1])
        add("count%d_f16_generic" % n, "f16", chans((2, 0, 3), 1, [1 + i % 3 for i in range(n)]), 1)
    # ---- the same tensor given twice ----------------------------------------------------------------------
    add("same_tensor_twice_i8", "int8", chans((1, 2, 2, 0), 3, (16, 32, 16)), 3, [Q_CONV[0], Q_SAME, Q_CONV[0]], Q_SAME,
        alias=[0, 1, 0])
    add("same_tensor_twice_f16", "f16", chans((1, 2, 2, 0), 3, (3, 3)), 3, alias=[0, 0])
    # ---- form boundaries: a length, an offset, or both off the 16-byte grid --------------------------------------
    for cs in ((16, 16), (16, 32, 48), (16, 20), (20, 16), (3, 5)):
        add("form_i8_nhwc_" + "_".join(map(str, cs)), "int8", chans((1, 2, 3, 0), 3, cs), 3,
            [recs[i % 3] for i in range(len(cs))], Q_SAME)
    for cs in ((8, 8), (8, 24), (8, 12)):
        add("form_f16_nhwc_" + "_".join(map(str, cs)), "f16", chans((1, 2, 3, 0), 3, cs), 3)
    # ---- int8 records --------------------------------------------------------------------------------------
    three = chans((1, 3, 3, 0), 3, (16, 16, 32))
    add("records_pure_copy", "int8", three, 3, [Q_SAME] * 3, Q_SAME)
    add("records_one_differs", "int8", three, 3, *mixed)
    add("records_all_differ", "int8", three, 3, *differ)
    add("records_saturating", "int8", three, 3, [Q_SAME, Q_CONV[0], Q_SAME], Q_OUT_SAT)
    add("records_all_differ_generic", "int8", chans((1, 3, 3, 0), 3, (5, 16, 3)), 3, *differ)
    fma_mixed = RECORD_PAIRS["fma_mixed"]                     # one wave spans all three inputs
    add("records_fma_mixed_vec", "int8", chans((1, 2, 2, 0), 3, (16, 32, 16)), 3, *fma_mixed)
    add("records_fma_mixed_generic", "int8", chans((1, 2, 2, 0), 3, (5, 16, 3)), 3, *fma_mixed)
    nine = [recs[i % 3] for i in range(9)]
    nine[3] = fma_mixed[0][1]                               # (input 8, an ordinary record, is the second launch)
    add("count9_fma_mixed_vec", "int8", chans((1, 2, 2, 0), 3, [16] * 9), 3, nine, Q_SAME)
    every = np.arange(-128, 128, dtype=np.int16).astype(np.int8).reshape(1, 256)
    for key, (ins, outq) in RECORD_PAIRS.items():
        add("exhaustive_i8_" + key, "int8", [(1, 256)] * len(ins), 1, ins, outq, xs=[every] * len(ins),
            alias=list(range(len(ins))))
    # ---- binary16, exhaustive: all 65 536 bit patterns beside an ordinary input -----------------------------------
    patterns = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).reshape(1, 65536)
    for form, c in (("vec", 8), ("generic", 12)):
        add("exhaustive_f16_" + form, "f16", [(1, 65536), (1, c)], 1,
            xs=[patterns, _data(_rng("f16 beside " + form), "f16", (1, c))])
    # ---- more than one wave and workgroup per row and per input -------------------------------------------------
    add("large_2x28x28x256_i8_nhwc", "int8", chans((2, 28, 28, 0), 3, (64, 64, 96, 32)), 3,
        [Q_SAME, Q_CONV[0], Q_A, Q_SAME], Q_SAME)
    add("large_2x40x28x28_f16_nchw", "f16", chans((2, 0, 28, 28), 1, (16, 24)), 1)
    # ---- a zero-length input between two ordinary ones: the device path skips it, as the reference's float loop does.
    # The genuine library ran it without error when the golden file was generated, so it IS in the golden file.
    add("zero_length_middle_i8", "int8", chans((1, 2, 2, 0), 3, (16, 0, 16)), 3, [Q_SAME, Q_CONV[0], Q_A], Q_SAME)
    add("zero_length_middle_f16", "f16", chans((2, 0, 3), 1, (2, 0, 1)), 1)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


# ------------------------------------------------------------------------------------ numpy restatement
def concat_numpy(case):
    ax = case["axis"] if case["axis"] >= 0 else len(case["out_shape"]) + case["axis"]
    with np.errstate(all="ignore"):
        fs = [pool_cases.dequantise(x, case["dtype"], q) for x, q in zip(case["xs"], case["in_qs"])]
        out = pool_cases.requantise(np.concatenate(fs, axis=ax), case["dtype"], case["out_q"])
    return np.ascontiguousarray(out)


def golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "concat_cases.npz")
    blob = np.load(path)
    return {k: blob[k] for k in blob.files}


# ------------------------------------------------------------------------------------ through csinn_*
def concat_run(fe, api, case, device=None, on_device=None, poison=None, layout=None, out_shape=None, axis=None,
               count=None):
    """layer mode through csinn_concat (+ _init).  device: a cases.HipDevice; on_device(i) says whether input i (or the
    output, i == -1) is a DMABUF tensor in HBM (default: all of them when `device` is given).  Returns the output, or
    (status, output buffer) when `poison` (a byte the output is pre-filled with) is given."""
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, api, keep)
    int8 = case["dtype"] == "int8"
    dt = pkg.DTYPE_INT8 if int8 else pkg.DTYPE_FLOAT16
    layout = layout if layout is not None else pkg.LAYOUT_NHWC
    on_device = on_device or (lambda i: device is not None)
    out = np.zeros(out_shape or case["out_shape"], dtype=case["xs"][0].dtype)
    if poison is not None:
        out.view(np.uint8)[...] = poison
    allocs, made = [], {}
    for i, x in enumerate(case["xs"]):
        k = case["alias"][i]
        if k in made:
            continue
        ptr = None
        if device is not None and on_device(i):
            ptr = device.alloc(x.nbytes)
            device.upload(ptr, x)
            allocs.append(ptr)
        s, z = case["in_qs"][i]
        made[k] = pkg.make_tensor(fe, keep, x.shape, dt, layout, data=x, scales=(s,), zps=(z,), name=b"in%d" % i,
                                  sess=sess, device_ptr=ptr)
    dev_out = None
    if device is not None and on_device(-1):
        dev_out = device.alloc(out.nbytes)
        device.upload(dev_out, out)
    t_out = pkg.make_tensor(fe, keep, out.shape, dt, layout, data=out, scales=(case["out_q"][0],), zps=(case["out_q"][1],),
                            name=b"out", sess=sess, device_ptr=dev_out)
    ins = pkg.tensor_array(keep, [made[k] for k in case["alias"]])
    params = pkg.concat_params(fe, keep, api, layout, len(case["xs"]) if count is None else count,
                               case["axis"] if axis is None else axis, sess)
    rc = fe.csinn_concat_init(ins, t_out, params)
    if rc == pkg.CSINN_TRUE:
        rc = fe.csinn_concat(ins, t_out, params)
    if dev_out is not None:
        out = device.download(dev_out, out.shape, out.dtype)
        device.free(dev_out)
    for p in allocs:
        device.free(p)
    if poison is not None:
        return rc, out
    if rc != pkg.CSINN_TRUE:
        raise pkg.MI355XError("csinn_concat returned %d" % rc)
    return out


class CabiArgs:
    """the arrays shl_mi355x_concat takes, from a case and the addresses of its inputs"""

    def __init__(self, case, ptrs):
        n = len(ptrs)
        ax = case["axis"] if case["axis"] >= 0 else len(case["out_shape"]) + case["axis"]
        inner = int(np.prod(case["out_shape"][ax + 1:], dtype=np.int64))
        self.ptrs = (C.c_void_p * n)(*ptrs)
        self.len = (C.c_int64 * n)(*[s[ax] * inner for s in case["shapes"]])
        self.scale = (C.c_float * n)(*[q[0] for q in case["in_qs"]])
        self.zp = (C.c_int32 * n)(*[q[1] for q in case["in_qs"]])
        d = pkg.ConcatDesc()
        d.dtype = pkg.SHL_I8 if case["dtype"] == "int8" else pkg.SHL_F16
        d.n_inputs = n
        d.outer = int(np.prod(case["out_shape"][:ax], dtype=np.int64))
        d.out_scale, d.out_zp = case["out_q"]
        self.desc = d

    def name(self, hip, out_ptr):
        return hip.shl_mi355x_concat_kernel_name(self.ptrs, self.len, self.scale, self.zp, out_ptr, C.byref(self.desc)).decode()

    def run(self, hip, out_ptr, stream=None):
        return hip.shl_mi355x_concat(self.ptrs, self.len, self.scale, self.zp, out_ptr, C.byref(self.desc), stream)


# ------------------------------------------------------------------------------------ a model that branches
class BranchNet:
    """data -> conv3x3+relu (16 -> 32 @16x16) -> Fire module (1x1 squeeze to 16 -> 1x1 and 3x3 expand to 32 each, with relu
    -> concat [+ a constant tensor]) -> maxpool 3x3 s2 pad 1 -> Inception block (1x1; 1x1 -> 3x3; 1x1 -> depthwise 3x3 ->
    1x1; avgpool 3x3 s1 p1 -> 1x1) -> concat -> global_avgpool2d -> 1x1 classifier -> softmax, int8 NHWC or fp16 NCHW,
    through the csinn session API in graph mode.

    concats=False builds THE SAME GRAPH WITHOUT ITS CONCATS: every concat input becomes a graph output and every concat
    output a graph input, so that the fusion planner's counts can be compared (that graph is built, never run)."""

    def __init__(self, dtype="int8", layout="NHWC", seed=31, const_input=False, concats=True, hw=16, classes=24):
        self.dtype, self.layout, self.hw, self.classes = dtype, layout, hw, classes
        self.const_c = 16 if const_input else 0
        self.concats = concats
        int8 = dtype == "int8"
        rng = np.random.default_rng(seed)
        q1 = lambda s, z: _q(s, z) if int8 else _q(1.0, 0)
        self.q1 = q1
        self.q_in = q1(2.0 ** -4, -5)

        def conv(cin, cout, k, act, hin, q_prev, out_q, k_log2=-7, depthwise=False):
            case = cases.make_case(int(rng.integers(1 << 30)), layout=layout, dtype=dtype, n=1, h=hin, w=hin, c=cin, co=cout,
                                   k=(k, k), pad=(k // 2,) * 4, act=act, depthwise=depthwise)
            if int8:
                case["in_scale"], case["in_zp"] = q_prev
                case["k_scale"] = np.array([2.0 ** k_log2], dtype=np.float32)
                case["b_scale"] = (np.float32(case["in_scale"]) * case["k_scale"]).astype(np.float32)
                case["bias"] = rng.integers(-2000, 2001, (case["co"],), dtype=np.int32)
                case["out_scale"], case["out_zp"] = out_q
            return case

        h, h2 = hw, pool_cases.out_dim(hw, 3, 2, 1, 1, 0)
        self.h2 = h2
        q = self.q = {}
        q["c0"], q["sq"] = q1(2.0 ** -3, -100), q1(2.0 ** -3, -90)
        # e1: a convolution and a relu LAYER with one record, which is what lets a session fold the relu into the convolution
        q["e1c"], q["e1"], q["e3"] = q1(2.0 ** -3, -100), q1(2.0 ** -3, -100), q1(2.0 ** -4, -90)
        q["k"] = q1(2.0 ** -5, 11)            # the constant concat input
        q["cat1"] = q["e1"]                   # the first input is copied, the others are requantised
        q["mp"] = q1(2.0 ** -3, -100)
        q["b1"], q["b2a"], q["b2"] = q1(2.0 ** -3, -110), q1(2.0 ** -3, -100), q1(2.0 ** -4, -100)
        q["b3a"], q["b3d"], q["b3"] = q1(2.0 ** -3, -100), q1(2.0 ** -3, -10), q1(2.0 ** -3, -120)
        q["b4p"], q["b4"] = q1(2.0 ** -3, -100), q1(2.0 ** -4, -128)
        q["cat2"] = q["b1"]
        q["gap"] = q1(2.0 ** -5, -128)
        c1 = 64 + self.const_c
        self.c_cat1, self.c_cat2 = c1, 16 + 32 + 16 + 16
        cv = self.cv = {}
        cv["c0"] = conv(16, 32, 3, 1, h, self.q_in, q["c0"])
        cv["sq"] = conv(32, 16, 1, 1, h, q["c0"], q["sq"])
        cv["e1"] = conv(16, 32, 1, 0, h, q["sq"], q["e1c"])     # followed by a relu LAYER (folded into it in a session)
        cv["e3"] = conv(16, 32, 3, 1, h, q["sq"], q["e3"])
        cv["b1"] = conv(c1, 16, 1, 1, h2, q["mp"], q["b1"])
        cv["b2a"] = conv(c1, 16, 1, 1, h2, q["mp"], q["b2a"])
        cv["b2"] = conv(16, 32, 3, 1, h2, q["b2a"], q["b2"])
        cv["b3a"] = conv(c1, 16, 1, 1, h2, q["mp"], q["b3a"])
        cv["b3d"] = conv(16, 16, 3, 0, h2, q["b3a"], q["b3d"], k_log2=-5, depthwise=True)
        cv["b3"] = conv(16, 16, 1, 1, h2, q["b3d"], q["b3"])
        cv["b4"] = conv(c1, 16, 1, 1, h2, q["b4p"], q["b4"])
        cv["fc"] = conv(self.c_cat2, classes, 1, 0, 1, q["gap"], q1(2.0 ** -4, -11), k_log2=-9)
        q["fc"] = q1(cv["fc"]["out_scale"], cv["fc"]["out_zp"])
        self.q_out = _q(1.0 / 256, -128) if int8 else _q(1.0, 0)
        if const_input:
            self.konst = _data(np.random.default_rng(seed + 1), dtype, self._shape(self.const_c, h))

    def _shape(self, c, h):
        return (1, h, h, c) if self.layout == "NHWC" else (1, c, h, h)

    @property
    def c_axis(self):
        return 3 if self.layout == "NHWC" else 1

    def input(self, k):
        rng = np.random.default_rng(900 + k)
        shape = self._shape(16, self.hw)
        return rng.integers(-100, 100, shape, dtype=np.int8) if self.dtype == "int8" else rng.standard_normal(shape).astype(np.float16)

    # -- oracle chain: convolutions through cases.oracle_run, pools and concat through the numpy restatements
    def oracle(self, x):
        form = "ref" if self.dtype == "int8" else "f16"
        q, cv = self.q, self.cv
        so = lambda **kw: tail.siso_oracle(dict(dtype=self.dtype, layout=self.layout, axis=1, **kw))

        def run_conv(name, cur):
            case = dict(cv[name])
            case["input"] = np.ascontiguousarray(cur)
            return cases.oracle_run(case, form)

        def pool(kind, cur, kernel, stride, in_q, out_q):
            h = cur.shape[1] if self.layout == "NHWC" else cur.shape[2]
            ho = pool_cases.out_dim(h, kernel, stride, 1, 1, 0)
            return pool_cases.pool_numpy(dict(kind=kind, dtype=self.dtype, layout=self.layout, x=cur, kernel=(kernel,) * 2,
                                              stride=(stride,) * 2, pad=(1,) * 4, cip=0, ho=ho, wo=ho, in_q=in_q, out_q=out_q))

        def cat(xs, in_qs, out_q):
            return concat_numpy(dict(dtype=self.dtype, axis=self.c_axis, xs=xs, in_qs=in_qs, out_q=out_q,
                                     out_shape=xs[0].shape))
        y0 = run_conv("c0", x)
        sq = run_conv("sq", y0)
        e1 = so(kind="relu", x=run_conv("e1", sq), in_q=q["e1c"], out_q=q["e1"])
        e3 = run_conv("e3", sq)
        parts, recs = [e1, e3], [q["e1"], q["e3"]]
        if self.const_c:
            parts, recs = parts + [self.konst], recs + [q["k"]]
        c1 = cat(parts, recs, q["cat1"])
        mp = pool("max", c1, 3, 2, q["cat1"], q["mp"])
        b1 = run_conv("b1", mp)
        b2 = run_conv("b2", run_conv("b2a", mp))
        b3 = run_conv("b3", run_conv("b3d", run_conv("b3a", mp)))
        b4 = run_conv("b4", pool("avg", mp, 3, 1, q["mp"], q["b4p"]))
        c2 = cat([b1, b2, b3, b4], [q["b1"], q["b2"], q["b3"], q["b4"]], q["cat2"])
        g = so(kind="pool", x=c2, in_q=q["cat2"], out_q=q["gap"])
        logits = run_conv("fc", g)
        return tail.siso_oracle(dict(kind="softmax", x=logits, dtype=self.dtype, layout=self.layout, axis=self.c_axis,
                                     in_q=q["fc"], out_q=self.q_out))

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
        n_in, n_out = (1, 1) if self.concats else (3, 7)
        fe.csinn_set_input_number(n_in, sess)
        fe.csinn_set_output_number(n_out, sess)
        nhwc = self.layout == "NHWC"
        act_l = pkg.LAYOUT_NHWC if nhwc else pkg.LAYOUT_NCHW
        q, cv = self.q, self.cv

        def T(dims, rec, name, data=None, const=0, layout=act_l, dtype=dt, scales=None):
            return pkg.make_tensor(fe, keep, dims, dtype, layout, data=data, is_const=const, name=name, sess=sess,
                                   scales=scales if scales is not None else (rec[0],), zps=(rec[1] if rec else 0,))

        ops, inputs, outputs = [], [], []

        def conv(name, t_in, c_out, h, rec, stem="csinn_conv2d_relu"):
            case = cv[name]
            bname = name.encode()
            if case["depthwise"]:
                w_l = pkg.LAYOUT_1HWO if nhwc else pkg.LAYOUT_O1HW
            else:
                w_l = pkg.LAYOUT_OHWI if nhwc else pkg.LAYOUT_OIHW
            t_w = T(case["w_shape"], None, bname + b"_w", case["kernel"], 1, w_l, scales=tuple(case["k_scale"]))
            t_b = T((case["co"],), None, bname + b"_b", case["bias"], 1, pkg.LAYOUT_O, pkg.DTYPE_INT32 if int8 else dt,
                    scales=tuple(case["b_scale"]))
            p = pkg.conv_params(fe, keep, api, act_l, case["stride"], case["pad"], case["dilation"], case["group"], 0, sess,
                                bname)
            t_out = T(self._shape(c_out, h), rec, bname + b"_out")
            ops.append((stem, (t_in, t_out, t_w, t_b, p)))
            return t_out

        def siso(stem, name, t_in, shape, rec, params):
            t_out = T(shape, rec, name + b"_out")
            ops.append((stem, (t_in, t_out, params)))
            return t_out

        def cat(name, parts, c_out, h, rec):
            """the concat layer -- or, without concats, its inputs as graph outputs and its output as a graph input"""
            t_out = T(self._shape(c_out, h), rec, name + b"_out")
            if self.concats:
                p = pkg.concat_params(fe, keep, api, act_l, len(parts), self.c_axis, sess, name)
                ops.append(("csinn_concat", (pkg.tensor_array(keep, parts), t_out, p)))
            else:
                outputs.extend(t for t in parts if not t.contents.is_const)
                inputs.append(t_out)
            return t_out

        h, h2 = self.hw, self.h2
        t_in = T(self._shape(16, h), self.q_in, b"data")
        inputs.append(t_in)
        t0 = conv("c0", t_in, 32, h, q["c0"])
        sq = conv("sq", t0, 16, h, q["sq"])
        e1c = conv("e1", sq, 32, h, q["e1c"], stem="csinn_conv2d")
        e1 = siso("csinn_relu", b"e1_relu", e1c, self._shape(32, h), q["e1"],
                  pkg.siso_params(fe, keep, api, "relu", act_l, 1, sess, b"e1_relu"))
        e3 = conv("e3", sq, 32, h, q["e3"])
        parts = [e1, e3]
        if self.const_c:
            parts.append(T(self._shape(self.const_c, h), q["k"], b"fire_const", self.konst, 1))
        c1 = cat(b"fire_concat", parts, self.c_cat1, h, q["cat1"])
        mp = siso("csinn_maxpool2d", b"maxpool", c1, self._shape(self.c_cat1, h2), q["mp"],
                  pkg.pool_params(fe, keep, api, act_l, (3, 3), (2, 2), (1, 1, 1, 1), 0, False, sess, b"maxpool"))
        b1 = conv("b1", mp, 16, h2, q["b1"])
        b2 = conv("b2", conv("b2a", mp, 16, h2, q["b2a"]), 32, h2, q["b2"])
        b3a = conv("b3a", mp, 16, h2, q["b3a"])
        b3d = conv("b3d", b3a, 16, h2, q["b3d"], stem="csinn_conv2d")
        b3 = conv("b3", b3d, 16, h2, q["b3"])
        b4p = siso("csinn_avgpool2d", b"avgpool", mp, self._shape(self.c_cat1, h2), q["b4p"],
                   pkg.pool_params(fe, keep, api, act_l, (3, 3), (1, 1), (1, 1, 1, 1), 0, False, sess, b"avgpool"))
        b4 = conv("b4", b4p, 16, h2, q["b4"])
        c2 = cat(b"inception_concat", [b1, b2, b3, b4], self.c_cat2, h2, q["cat2"])
        g = siso("csinn_global_avgpool2d", b"gap", c2, self._shape(self.c_cat2, 1), q["gap"],
                 pkg.siso_params(fe, keep, api, "pool", act_l, 1, sess, b"gap"))
        logits = conv("fc", g, self.classes, 1, q["fc"], stem="csinn_conv2d")
        prob = siso("csinn_softmax", b"softmax", logits, self._shape(self.classes, 1), self.q_out,
                    pkg.siso_params(fe, keep, api, "softmax", act_l, self.c_axis, sess, b"softmax"))
        outputs.append(prob)
        assert (len(inputs), len(outputs)) == (n_in, n_out)
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
        self._keep, self._sess, self._out_shape, self._in_q = keep, sess, self._shape(self.classes, 1), self.q_in
        self.layer_count = len(ops)
        return sess

    run = tail.MiniNet.run
    close = tail.MiniNet.close

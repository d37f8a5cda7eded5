"""Shared helpers for the sigmoid family, leaky_relu and the broadcasting mul (CSINN_OP_SIGMOID / _HARD_SIGMOID / _SILU /
_LEAKY_RELU / _MUL).

  eltwise_cases()               deterministic single-op problems: every int8 byte through every record pair, every binary16
                                pattern, every pair of int8 operands, the smallest shapes at which each kernel form (16 bytes
                                per lane, one byte per thread; mul: vec, row, generic) can still go wrong
  eltwise_numpy(case)           plain numpy restatement of the reference (source/reference/sigmoid.c:33, silu.c:33,
                                hard_sigmoid.c:31-37, leaky_relu.c:33, mul.c:21-40 inside shl_ref_siso / diso_callback_base):
                                dequantise, the formula in the reference's precision (the C library's double exp), requantise
  eltwise_run(fe, api, case)    csinn_<op>_init + csinn_<op> through a front-end (layer mode), host or DMABUF tensors
  SeNet                         conv -> squeeze-and-excite (global_avgpool -> 1x1 -> relu -> 1x1 -> hard_sigmoid | sigmoid ->
                                mul) -> 1x1 -> silu | leaky_relu -> mul by a per-channel constant -> global_avgpool ->
                                classifier -> softmax through the csinn session API (graph mode), with an oracle replay
The genuine library's outputs for eltwise_cases() live in tests/golden/eltwise_cases.npz (make_eltwise_golden.py).
"""
import ctypes as C
import fractions
import math
import os
import zlib

import numpy as np

import cases
import pool_cases
import tail
from cases import pkg
from pool_cases import Q_F16, _q, assert_same, bits  # noqa: F401

UNARY = ("sigmoid", "hard_sigmoid", "silu", "leaky_relu")
OPS = {"sigmoid": pkg.OP_SIGMOID, "hard_sigmoid": pkg.OP_HARD_SIGMOID, "silu": pkg.OP_SILU, "leaky_relu": pkg.OP_LEAKY_RELU,
       "mul": pkg.OP_MUL}
KIND = {"sigmoid": pkg.UNARY_SIGMOID, "hard_sigmoid": pkg.UNARY_HARD_SIGMOID, "silu": pkg.UNARY_SILU,
        "leaky_relu": pkg.UNARY_LEAKY_RELU}
# (input record, output record) of the int8 unary cases: each is walked over all 256 bytes by every op
RECORD_PAIRS = {
    "ident": (_q(2.0 ** -4, -5), _q(2.0 ** -4, -5)),
    "conv": (_q(0.0473, -9), _q(0.0219, 4)),             # converter scales
    "sat": (_q(2.0 ** -4, -5), _q(2.0 ** -6, 100)),      # the out record saturates
    "gate": (_q(2.0 ** -4, -5), _q(1.0 / 256, -128)),    # sigmoid's natural output record
}
# (a record, b record, out record) of the int8 mul cases: each is walked over the 256 x 256 grid of operand pairs
RECORD_TRIPLES = {
    "pow2": (_q(2.0 ** -4, -5), _q(2.0 ** -7, -128), _q(2.0 ** -4, -5)),   # a feature map times a gate
    "conv": (_q(0.0473, -9), _q(0.0219, 4), _q(0.0311, 3)),
    "sat": (_q(2.0 ** -4, -5), _q(2.0 ** -3, 9), _q(2.0 ** -6, 100)),
}
SLOPES = (0.1, 0.0, -0.5)  # leaky_relu's n
F16_SCALARS = {"one": 0x3C00, "minus_zero": 0x8000, "half": 0x3800, "three": 0x4200, "max": 0x7BFF, "min_subnormal": 0x0001,
               "inf": 0x7C00, "nan": 0x7E00}


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _data(rng, dtype, shape):
    if dtype == "int8":
        return rng.integers(-128, 128, shape, dtype=np.int8)
    return (3.0 * rng.standard_normal(shape)).astype(np.float16)


def eltwise_cases():
    out = []

    def unary(name, op, dtype, x, q=None, n=0.0):
        in_q, out_q = q if dtype == "int8" else Q_F16
        out.append(dict(name=name, op=op, dtype=dtype, x=np.ascontiguousarray(x), in_q=in_q, out_q=out_q, n=float(np.float32(n)),
                        layout="NHWC"))

    def mul(name, dtype, a_shape, b_shape, q=None, layout="NHWC", small_first=False, b_const=False, x=None, y=None):
        """x has a_shape (the output's), y has b_shape; small_first: y is given as the FIRST input"""
        rng = _rng(name)
        x = _data(rng, dtype, a_shape) if x is None else x
        y = _data(rng, dtype, b_shape) if y is None else y
        qa, qb, qo = q if dtype == "int8" else (Q_F16[0],) * 3
        out.append(dict(name=name, op="mul", dtype=dtype, x=np.ascontiguousarray(x), y=np.ascontiguousarray(y), in_q=qa, in1_q=qb,
                        out_q=qo, layout=layout, small_first=small_first, b_const=b_const))

    every = np.arange(-128, 128, dtype=np.int16).astype(np.int8)
    patterns = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    # ---- int8 unary: all 256 bytes through every record pair; leaky_relu with every slope -------------------------------
    for op in UNARY:
        for key, q in RECORD_PAIRS.items():
            for n in SLOPES if op == "leaky_relu" else (0.0,):
                tag = "_n%g" % n if op == "leaky_relu" else ""
                unary("%s_i8_all_%s%s" % (op, key, tag), op, "int8", every, q, n)
        # counts around the 16-byte piece, and a tail behind 256 whole pieces
        for count in (1, 15, 16, 17, 4096 + 5):
            unary("%s_i8_count%d" % (op, count), op, "int8", _data(_rng("%s i8 %d" % (op, count)), "int8", (count,)),
                  RECORD_PAIRS["conv"], 0.1)
    # ---- binary16 unary: all 65 536 patterns (NaNs, infinities, signed zeros, subnormals, 65504) -----------------------
    for op in UNARY:
        unary("%s_f16_all" % op, op, "f16", patterns, n=0.1)
        for count in (1, 7, 8, 9):
            unary("%s_f16_count%d" % (op, count), op, "f16", _data(_rng("%s f16 %d" % (op, count)), "f16", (count,)), n=-0.5)
    # ---- int8 mul: the 256 x 256 grid of all operand pairs, same shape ------------------------------------------------
    grid_a, grid_b = np.repeat(every, 256).reshape(256, 256), np.tile(every, 256).reshape(256, 256)
    for key, q in RECORD_TRIPLES.items():
        mul("mul_i8_grid_" + key, "int8", (256, 256), (256, 256), q, layout="NC", x=grid_a, y=grid_b)
    # ---- binary16 mul: all patterns times a broadcast scalar -----------------------------------------------------------
    for key, h in F16_SCALARS.items():
        mul("mul_f16_all_by_" + key, "f16", (65536,), (1,), layout="N", x=patterns, y=np.array([h], np.uint16).view(np.float16))
    # ---- broadcast geometry, both dtypes -------------------------------------------------------------------------------
    conv = RECORD_TRIPLES["conv"]
    for dtype in ("int8", "f16"):
        d = "i8" if dtype == "int8" else "f16"
        mul("mul_%s_nhwc_gate_c16" % d, dtype, (2, 3, 5, 16), (2, 1, 1, 16), conv)           # vec, b along N and C
        mul("mul_%s_nhwc_gate_c20" % d, dtype, (2, 3, 5, 20), (2, 1, 1, 20), conv)           # int8: generic; f16: generic (20 % 8)
        mul("mul_%s_nhwc_channels" % d, dtype, (2, 3, 5, 16), (16,), conv)                   # vec, a lower-rank b
        mul("mul_%s_nhwc_111c" % d, dtype, (2, 3, 5, 16), (1, 1, 1, 16), conv)
        mul("mul_%s_scalar" % d, dtype, (2, 3, 5, 16), (1,), conv)                           # vec, scalar
        mul("mul_%s_scalar_tail" % d, dtype, (3, 7, 5), (1,), conv, layout="N")              # 105 elements: pieces + tail
        mul("mul_%s_same_tail" % d, dtype, (3, 7, 5), (3, 7, 5), conv, layout="N")
        mul("mul_%s_nchw_gate" % d, dtype, (2, 3, 4, 5), (2, 3, 1, 1), conv, layout="NCHW")  # row
        mul("mul_%s_nchw_channels" % d, dtype, (2, 3, 4, 5), (1, 3, 1, 1), conv, layout="NCHW")
        for hw in ((1, 1), (2, 2), (1, 37)):                                                 # row-form tails: H W = 1, 4, 37
            mul("mul_%s_nchw_hw%d" % (d, hw[0] * hw[1]), dtype, (2, 3) + hw, (2, 3, 1, 1), conv, layout="NCHW")
        mul("mul_%s_nchw_middle" % d, dtype, (2, 3, 4, 5), (1, 1, 4, 1), conv, layout="NCHW")  # row: b varies along H only
        mul("mul_%s_small_first_nhwc" % d, dtype, (2, 3, 5, 16), (2, 1, 1, 16), conv, small_first=True)
        mul("mul_%s_small_first_nchw" % d, dtype, (2, 3, 4, 5), (1, 3, 1, 1), conv, layout="NCHW", small_first=True)
        mul("mul_%s_const_channels" % d, dtype, (2, 3, 5, 16), (16,), conv, b_const=True)
        mul("mul_%s_const_nchw" % d, dtype, (2, 3, 4, 5), (1, 3, 1, 1), conv, layout="NCHW", b_const=True)
    # ---- more than one workgroup ----------------------------------------------------------------------------------------
    # (a block of 4 096 random values over and over: the golden file stays small)
    def tiled(dtype, shape):
        n = int(np.prod(shape))
        block = _data(_rng("big " + dtype), dtype, (4096,))
        return np.resize(block, n).reshape(shape)
    big = tiled("int8", (2, 56, 56, 64))
    unary("silu_i8_2x56x56x64", "silu", "int8", big, RECORD_PAIRS["conv"])
    mul("mul_i8_2x56x56x64_gate", "int8", (2, 56, 56, 64), (2, 1, 1, 64), RECORD_TRIPLES["pow2"], x=big)
    mul("mul_f16_2x64x28x28_gate", "f16", (2, 64, 28, 28), (2, 64, 1, 1), layout="NCHW", x=tiled("f16", (2, 64, 28, 28)))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


# ------------------------------------------------------------------------------------ numpy restatement
def _exp(v):
    """the C library's double exp, element by element (numpy's own vector exp is another implementation)"""
    def one(t):
        try:
            return math.exp(t)
        except OverflowError:
            return math.inf
    return np.array([one(float(t)) for t in v.ravel()], dtype=np.float64).reshape(v.shape)


_FIFTH, _HALF = fractions.Fraction(0.2), fractions.Fraction(0.5)  # the doubles 0.2 and 0.5, exactly


def _nan_like(sign_source, flip=False):
    """a float32 NaN with the sign bit of `sign_source` (flipped on request)"""
    s = np.signbit(sign_source) ^ flip
    return np.where(s, np.uint32(0xFFC00000), np.uint32(0x7FC00000)).astype(np.uint32).view(np.float32)


def unary_f32(op, v, n):
    """the reference's float function on dequantised values.  A NaN keeps its sign on the way through (x86 operations hand
    a NaN operand on); sigmoid's is negated first, by -val"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    with np.errstate(all="ignore"):
        if op == "sigmoid":
            r = (1.0 / (1.0 + _exp((-v).astype(np.float64)))).astype(np.float32)
        elif op == "silu":
            r = (v.astype(np.float64) / (1.0 + _exp((-v).astype(np.float64)))).astype(np.float32)
        elif op == "hard_sigmoid":
            d = v.astype(np.float64)
            # 0.2 x + 0.5 is ONE fused multiply-add in the reference's build (-O3 -mfma): exact, rounded once
            inside = np.flatnonzero((d.ravel() >= -2.5) & (d.ravel() <= 2.5))
            fused = np.array([float(_FIFTH * fractions.Fraction(float(t)) + _HALF) for t in d.ravel()[inside]], dtype=np.float64)
            r = np.where(d < -2.5, 0.0, 1.0).ravel()
            r[inside] = fused
            r = r.reshape(d.shape).astype(np.float32)
        elif op == "leaky_relu":
            r = np.where(v > 0, v, v * np.float32(n)).astype(np.float32)
        else:
            raise ValueError(op)
    return np.where(np.isnan(v), _nan_like(v, flip=op == "sigmoid"), r)


def mul_f32(a, b):
    """one float32 product of the layer's first input a and second input b.  NaNs as the reference's x86 build hands them
    on: an operand's NaN keeps its sign (the SECOND input's when both are NaNs: mul.c:23 compiles to src1 * src0), inf * 0
    gives the default NaN, whose sign bit is set"""
    with np.errstate(all="ignore"):
        p = (a * b).astype(np.float32)
    made = np.isnan(p) & ~np.isnan(a) & ~np.isnan(b)
    p = np.where(np.isnan(b), _nan_like(b), np.where(np.isnan(a), _nan_like(a), p))
    return np.where(made, np.float32(np.uint32(0xFFC00000).view(np.float32)), p)


def eltwise_numpy(case):
    dt = case["dtype"]
    x = pool_cases.dequantise(case["x"], dt, case["in_q"])
    if case["op"] == "mul":
        y = np.broadcast_to(pool_cases.dequantise(case["y"], dt, case["in1_q"]), x.shape)
        r = mul_f32(y, x) if case.get("small_first") else mul_f32(x, y)
    else:
        r = unary_f32(case["op"], x, case["n"])
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(pool_cases.requantise(r, dt, case["out_q"])).reshape(case["x"].shape)


def golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eltwise_cases.npz")
    blob = np.load(path)
    return {k: blob[k] for k in blob.files}


# ------------------------------------------------------------------------------------ through csinn_*
_LAYOUTS = {"NHWC": pkg.LAYOUT_NHWC, "NCHW": pkg.LAYOUT_NCHW, "NC": pkg.LAYOUT_NC, "N": pkg.LAYOUT_N}


def eltwise_run(fe, api, case, device=None, poison=None, in_skew=0, **override):
    """layer mode through csinn_<op> (+ _init).  device: a cases.HipDevice -- every non-constant tensor then lives in HBM as
    a DMABUF tensor, the first input `in_skew` ELEMENTS into its allocation.  override: out_shape / out_dtype / in1_dtype /
    scales / out_q ... for the refusal tests.  Returns the output, or (status, output buffer) when `poison` (a byte the
    output is pre-filled with) is given."""
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, api, keep)
    np_dt = {"int8": np.int8, "f16": np.float16}
    code = {"int8": pkg.DTYPE_INT8, "f16": pkg.DTYPE_FLOAT16}
    dt = case["dtype"]
    layout = _LAYOUTS[case["layout"]]
    x = case["x"]
    out_dt = override.get("out_dtype", dt)
    out = np.zeros(override.get("out_shape", x.shape), dtype=np_dt[out_dt])
    if poison is not None:
        out.view(np.uint8)[...] = poison
    allocs = []

    def tensor(arr, q, name, dtype=dt, const=0, skew=0, scales=None):
        ptr = None
        if device is not None and not const:
            base = device.alloc(arr.nbytes + 64)
            allocs.append(base)
            ptr = base + skew * arr.itemsize
            device.upload(ptr, arr)
        return pkg.make_tensor(fe, keep, arr.shape, code[dtype], layout, data=arr, scales=scales or (q[0],), zps=(q[1],),
                               name=name, sess=sess, device_ptr=ptr, is_const=const), ptr

    t_x, _ = tensor(x, case["in_q"], b"in0", skew=in_skew, scales=override.get("scales"))
    t_out, dev_out = tensor(out, override.get("out_q", case["out_q"]), b"out", dtype=out_dt)
    op = case["op"]
    if op == "mul":
        y = case["y"] if "in1_dtype" not in override else case["y"].astype(np_dt[override["in1_dtype"]])
        t_y, _ = tensor(y, case["in1_q"], b"in1", dtype=override.get("in1_dtype", dt), const=1 if case["b_const"] else 0)
        params = pkg.siso_params(fe, keep, api, "mul", layout, 1, sess, b"mul")
        args = (t_y, t_x, t_out, params) if case["small_first"] else (t_x, t_y, t_out, params)
    else:
        params = pkg.siso_params(fe, keep, api, op, layout, 1, sess, op.encode(), n=case["n"])
        args = (t_x, t_out, params)
    rc = getattr(fe, "csinn_%s_init" % op)(*args)
    if rc == pkg.CSINN_TRUE:
        rc = getattr(fe, "csinn_" + op)(*args)
    if dev_out is not None:
        out = device.download(dev_out, out.shape, out.dtype)
    for p in allocs:
        device.free(p)
    if poison is not None:
        return rc, out
    if rc != pkg.CSINN_TRUE:
        raise pkg.MI355XError("csinn_%s returned %d" % (op, rc))
    return out


def mul_desc(case, shape_a=None, shape_b=None):
    """struct shl_mi355x_mul_desc of a mul case: the output's dims collapsed into groups along which b varies or is
    broadcast (dims of size 1 join either neighbour), b's stride per group"""
    a_shape = tuple(shape_a if shape_a is not None else case["x"].shape)
    b_shape = tuple(shape_b if shape_b is not None else case["y"].shape)
    b_shape = (1,) * (len(a_shape) - len(b_shape)) + b_shape
    dims, cls = [], []
    for da, db in zip(a_shape, b_shape):
        if da == 1:
            continue
        varies = db != 1
        if cls and cls[-1] == varies:
            dims[-1] *= da
        else:
            dims.append(da)
            cls.append(varies)
    if not dims:
        dims, cls = [int(np.prod(a_shape))], [True]
    d = pkg.MulDesc()
    d.dtype = pkg.SHL_I8 if case["dtype"] == "int8" else pkg.SHL_F16
    d.ngroups = len(dims)
    stride = 1
    for g in range(len(dims) - 1, -1, -1):
        d.dim[g] = dims[g]
        d.b_stride[g] = stride if cls[g] else 0
        if cls[g]:
            stride *= dims[g]
    (d.a_scale, d.a_zp), (d.b_scale, d.b_zp), (d.out_scale, d.out_zp) = case["in_q"], case["in1_q"], case["out_q"]
    d.a_is_second = 1 if case.get("small_first") else 0
    return d


# ------------------------------------------------------------------------------------ a squeeze-and-excite model
class SeNet:
    """data -> conv3x3+relu (16 -> 32 @8x8) -> [global_avgpool -> 1x1 (32 -> 8) -> relu -> 1x1 (8 -> 32) -> hard_sigmoid |
    sigmoid] -> mul(conv output, gate) -> 1x1 (32 -> 32) -> silu | leaky_relu -> mul by a constant [32] (NCHW: [1,32,1,1])
    -> global_avgpool -> 1x1 classifier -> softmax, int8 NHWC or fp16 NCHW, through the csinn session API in graph mode.
    variant 0: hard_sigmoid gate and silu (an SE block with swish); variant 1: sigmoid gate and leaky_relu."""

    def __init__(self, dtype="int8", layout="NHWC", variant=0, seed=41, hw=8, classes=24):
        self.dtype, self.layout, self.hw, self.classes, self.variant = dtype, layout, hw, classes, variant
        self.gate_op = ("hard_sigmoid", "sigmoid")[variant]
        self.act_op = ("silu", "leaky_relu")[variant]
        self.slope = 0.1
        int8 = dtype == "int8"
        rng = np.random.default_rng(seed)
        q1 = lambda s, z: _q(s, z) if int8 else _q(1.0, 0)
        self.q_in = q1(2.0 ** -4, -5)

        def conv(cin, cout, k, act, hin, q_prev, out_q, k_log2=-7):
            case = cases.make_case(int(rng.integers(1 << 30)), layout=layout, dtype=dtype, n=1, h=hin, w=hin, c=cin, co=cout,
                                   k=(k, k), pad=(k // 2,) * 4, act=act)
            if int8:
                case["in_scale"], case["in_zp"] = q_prev
                case["k_scale"] = np.array([2.0 ** k_log2], dtype=np.float32)
                case["b_scale"] = (np.float32(case["in_scale"]) * case["k_scale"]).astype(np.float32)
                case["bias"] = rng.integers(-2000, 2001, (case["co"],), dtype=np.int32)
                case["out_scale"], case["out_zp"] = out_q
            return case

        q = self.q = {}
        q["c0"] = q1(2.0 ** -3, -100)
        q["sq"] = q1(2.0 ** -5, -128)
        # fc1: a convolution and a relu LAYER with one record, which is what lets a session fold the relu into the convolution
        q["fc1c"], q["fc1"] = q1(2.0 ** -4, -100), q1(2.0 ** -4, -100)
        q["fc2"] = q1(2.0 ** -4, 3)
        q["gate"] = q1(1.0 / 256, -128)
        q["se"] = q1(2.0 ** -3, -100)
        q["pw"] = q1(2.0 ** -3, -20)
        q["act"] = q1(2.0 ** -4, -60)
        q["k"] = q1(2.0 ** -6, -10)          # the per-channel constant
        q["scaled"] = q1(2.0 ** -4, -50)
        q["gap"] = q1(2.0 ** -5, -60)
        cv = self.cv = {}
        cv["c0"] = conv(16, 32, 3, 1, hw, self.q_in, q["c0"])
        cv["fc1"] = conv(32, 8, 1, 0, 1, q["sq"], q["fc1c"], k_log2=-5)    # followed by a relu LAYER (folded in a session)
        cv["fc2"] = conv(8, 32, 1, 0, 1, q["fc1"], q["fc2"], k_log2=-5)
        cv["pw"] = conv(32, 32, 1, 0, hw, q["se"], q["pw"])
        cv["fc"] = conv(32, classes, 1, 0, 1, q["gap"], q1(2.0 ** -4, -11), k_log2=-6)
        q["fc"] = q1(cv["fc"]["out_scale"], cv["fc"]["out_zp"])
        self.q_out = _q(1.0 / 256, -128) if int8 else _q(1.0, 0)
        krng = np.random.default_rng(seed + 1)
        kshape = (32,) if layout == "NHWC" else (1, 32, 1, 1)
        self.konst = krng.integers(-128, 128, kshape, dtype=np.int8) if int8 else (0.5 + krng.random(kshape)).astype(np.float16)

    def _shape(self, c, h):
        return (1, h, h, c) if self.layout == "NHWC" else (1, c, h, h)

    @property
    def c_axis(self):
        return 3 if self.layout == "NHWC" else 1

    def input(self, k):
        rng = np.random.default_rng(700 + k)
        shape = self._shape(16, self.hw)
        return rng.integers(-100, 100, shape, dtype=np.int8) if self.dtype == "int8" else rng.standard_normal(shape).astype(np.float16)

    # -- oracle chain: convolutions, relu, pools and softmax through the C oracle, the new layers through eltwise_numpy
    def oracle(self, x):
        form = "ref" if self.dtype == "int8" else "f16"
        q, cv = self.q, self.cv
        so = lambda **kw: tail.siso_oracle(dict(dtype=self.dtype, layout=self.layout, axis=1, **kw))

        def run_conv(name, cur):
            case = dict(cv[name])
            case["input"] = np.ascontiguousarray(cur)
            return cases.oracle_run(case, form)

        def unary(op, cur, in_q, out_q):
            return eltwise_numpy(dict(op=op, dtype=self.dtype, x=cur, in_q=in_q, out_q=out_q, n=float(np.float32(self.slope))))

        def mul(a, b, qa, qb, qo):
            return eltwise_numpy(dict(op="mul", dtype=self.dtype, x=a, y=b, in_q=qa, in1_q=qb, out_q=qo))
        y0 = run_conv("c0", x)
        sq = so(kind="pool", x=y0, in_q=q["c0"], out_q=q["sq"])
        f1 = so(kind="relu", x=run_conv("fc1", sq), in_q=q["fc1c"], out_q=q["fc1"])
        gate = unary(self.gate_op, run_conv("fc2", f1), q["fc2"], q["gate"])
        se = mul(y0, gate, q["c0"], q["gate"], q["se"])
        act = unary(self.act_op, run_conv("pw", se), q["pw"], q["act"])
        scaled = mul(act, self.konst, q["act"], q["k"], q["scaled"])
        g = so(kind="pool", x=scaled, in_q=q["scaled"], out_q=q["gap"])
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
        fe.csinn_set_input_number(1, sess)
        fe.csinn_set_output_number(1, sess)
        nhwc = self.layout == "NHWC"
        act_l = pkg.LAYOUT_NHWC if nhwc else pkg.LAYOUT_NCHW
        q, cv = self.q, self.cv

        def T(dims, rec, name, data=None, const=0, layout=act_l, dtype=dt, scales=None):
            return pkg.make_tensor(fe, keep, dims, dtype, layout, data=data, is_const=const, name=name, sess=sess,
                                   scales=scales if scales is not None else (rec[0],), zps=(rec[1] if rec else 0,))

        ops = []

        def conv(name, t_in, c_out, h, rec, stem="csinn_conv2d"):
            case = cv[name]
            bname = name.encode()
            t_w = T(case["w_shape"], None, bname + b"_w", case["kernel"], 1, pkg.LAYOUT_OHWI if nhwc else pkg.LAYOUT_OIHW,
                    scales=tuple(case["k_scale"]))
            t_b = T((case["co"],), None, bname + b"_b", case["bias"], 1, pkg.LAYOUT_O, pkg.DTYPE_INT32 if int8 else dt,
                    scales=tuple(case["b_scale"]))
            p = pkg.conv_params(fe, keep, api, act_l, case["stride"], case["pad"], case["dilation"], case["group"], 0, sess, bname)
            t_out = T(self._shape(c_out, h), rec, bname + b"_out")
            ops.append((stem, (t_in, t_out, t_w, t_b, p)))
            return t_out

        def siso(kind, name, t_in, shape, rec, **kw):
            t_out = T(shape, rec, name + b"_out")
            stem = {"pool": "csinn_global_avgpool2d"}.get(kind, "csinn_" + kind)
            ops.append((stem, (t_in, t_out, pkg.siso_params(fe, keep, api, kind, act_l, self.c_axis, sess, name, **kw))))
            return t_out

        def mul(name, t_a, t_b, shape, rec):
            t_out = T(shape, rec, name + b"_out")
            ops.append(("csinn_mul", (t_a, t_b, t_out, pkg.siso_params(fe, keep, api, "mul", act_l, 1, sess, name))))
            return t_out

        h = self.hw
        t_in = T(self._shape(16, h), self.q_in, b"data")
        y0 = conv("c0", t_in, 32, h, q["c0"], stem="csinn_conv2d_relu")
        sq = siso("pool", b"squeeze", y0, self._shape(32, 1), q["sq"])
        f1c = conv("fc1", sq, 8, 1, q["fc1c"])
        f1 = siso("relu", b"fc1_relu", f1c, self._shape(8, 1), q["fc1"])
        f2 = conv("fc2", f1, 32, 1, q["fc2"])
        gate = siso(self.gate_op, b"gate", f2, self._shape(32, 1), q["gate"])
        se = mul(b"excite", y0, gate, self._shape(32, h), q["se"])
        pw = conv("pw", se, 32, h, q["pw"])
        act = siso(self.act_op, b"act", pw, self._shape(32, h), q["act"], **({"n": self.slope} if self.act_op == "leaky_relu" else {}))
        t_k = T(self.konst.shape, q["k"], b"channel_scale", self.konst, 1, act_l if self.konst.ndim == 4 else pkg.LAYOUT_N)
        scaled = mul(b"scale", act, t_k, self._shape(32, h), q["scaled"])
        g = siso("pool", b"gap", scaled, self._shape(32, 1), q["gap"])
        logits = conv("fc", g, self.classes, 1, q["fc"])
        prob = siso("softmax", b"softmax", logits, self._shape(self.classes, 1), self.q_out)
        for stem, args in ops:
            assert getattr(fe, stem + "_init")(*args) == pkg.CSINN_TRUE, stem
        fe.csinn_set_tensor_entry(t_in, sess)
        fe.csinn_set_input(0, t_in, sess)
        for stem, args in ops:
            assert getattr(fe, stem)(*args) == pkg.CSINN_TRUE, stem
        fe.csinn_set_output(0, prob, sess)
        rc = fe.csinn_session_setup(sess)
        assert rc == pkg.CSINN_TRUE or getattr(fe, "kind", "") == "reference"
        self._keep, self._sess, self._out_shape, self._in_q = keep, sess, self._shape(self.classes, 1), self.q_in
        self.layer_count = len(ops)
        return sess

    run = tail.MiniNet.run
    close = tail.MiniNet.close

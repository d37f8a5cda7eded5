"""Shared helpers for resize (CSINN_OP_RESIZE): nearest-neighbour and bilinear, align_corners off and on, int8 and binary16,
NHWC and NCHW.

  resize_cases()                deterministic single-op problems: the smallest shapes at which each kernel form (16 bytes of
                                a pixel's channels per thread, dwords of an NCHW row, one output per thread) can still go
                                wrong
  resize_numpy(case)            plain numpy restatement of the reference (source/reference/resize.c:21-124 inside
                                shl_ref_siso_callback_base): dequantise, the float32 routine with the reference's index
                                arithmetic and its build's fused multiply-adds (modelled exactly, one rounding), requantise
  resize_run(fe, api, case)     csinn_resize_init + csinn_resize through a front-end (layer mode), host or DMABUF tensors
  reference_run(fe, case)       the same on the genuine library, NCHW nearest batches one image at a time (the reference
                                advances the output by the input's batch size there, resize.c:179 / :397)
  PyramidNet                    three stride-2 convolutions -> lateral 1x1 -> resize nearest 2x -> add -> 3x3 -> resize
                                bilinear -> concat -> 1x1 -> global_avgpool -> classifier -> softmax through the csinn
                                session API (graph mode), with an oracle replay
The genuine library's outputs for resize_cases() live in tests/golden/resize_cases.npz (make_resize_golden.py).
"""
import fractions
import os
import zlib

import numpy as np

import cases
import concat_cases
import eltwise_cases
import pool_cases
import tail
from cases import pkg
from pool_cases import Q_F16, _q, assert_same, bits  # noqa: F401

MODES = {"nearest": pkg.RESIZE_NEAREST_NEIGHBOR, "bilinear": pkg.RESIZE_BILINEAR}
RECORD_PAIRS = {k: eltwise_cases.RECORD_PAIRS[k] for k in ("ident", "conv", "sat")}
# (in_h, in_w, out_h, out_w, align_corners values)
GEOMETRIES = [
    (1, 1, 3, 4, (False, True)),       # one source pixel; the align_corners scale is 0
    (2, 2, 4, 4, (False, True)),       # integer factor
    (3, 5, 6, 10, (False, True)),      # integer factor, H != W; run at batch 2
    (3, 5, 7, 11, (False, True)),      # an inexact float scale, up; carries the channel sweep
    (7, 9, 3, 4, (False, True)),       # down
    (4, 6, 4, 6, (False, True)),       # identity: every weight is exactly 0 or 1
    (5, 4, 1, 1, (False,)),            # output extent 1 (align_corners would divide by zero)
    (13, 17, 29, 37, (False, True)),   # rows longer than a wave's share
]
# (dtype, layout, channels): 16-byte pieces; no whole pieces (one output per thread); NCHW rows
FORMATS = [("int8", "NHWC", 16), ("f16", "NHWC", 8), ("int8", "NHWC", 15), ("f16", "NHWC", 7), ("int8", "NCHW", 3), ("f16", "NCHW", 3)]
SWEEP = [("int8", "NHWC", 1), ("int8", "NHWC", 17), ("int8", "NHWC", 32), ("f16", "NHWC", 9), ("f16", "NHWC", 16)]
SPECIALS = (0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x8000, 0x0001, 0x7BFF, 0xFBFF)  # inf, -inf, NaN, -NaN, -0, subnormal, +-65504


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _data(rng, dtype, shape):
    if dtype == "int8":
        return rng.integers(-128, 128, shape, dtype=np.int8)
    return (3.0 * rng.standard_normal(shape)).astype(np.float16)


def tiled(dtype, shape):
    """a block of 4 096 random values over and over: the golden file stays small"""
    block = _data(_rng("big " + dtype), dtype, (4096,))
    return np.resize(block, int(np.prod(shape))).reshape(shape)


def f16_specials(layout, c):
    """1 x 4 x 4 x c: every special value once per channel pair, each beside ordinary values, and two specials side by side"""
    x = (2.0 * np.random.default_rng(77 + c).standard_normal((1, 4, 4, c))).astype(np.float16).view(np.uint16)
    spots = [(0, 0), (0, 2), (1, 1), (1, 3), (2, 0), (2, 2), (3, 1), (3, 3)]
    for ch in range(c):
        for k, (y, xx) in enumerate(spots):
            x[0, y, xx, ch] = SPECIALS[(k + ch) % len(SPECIALS)]
    x[0, 3, 2, :] = 0x7C00        # an infinity beside (3, 1) and (3, 3)
    x[0, 0, 1, 0::2] = 0xFE00     # a negative NaN between two specials
    x = x.view(np.float16)
    return np.ascontiguousarray(x if layout == "NHWC" else x.transpose(0, 3, 1, 2))


def resize_cases():
    out = []

    def add(name, mode, align, dtype, layout, n, c, h, w, ho, wo, q=None, x=None):
        in_q, out_q = q if dtype == "int8" else Q_F16
        shape = (n, h, w, c) if layout == "NHWC" else (n, c, h, w)
        if x is None:
            x = _data(_rng(name), dtype, shape)
        assert x.shape == shape, (name, x.shape, shape)
        out.append(dict(name=name, mode=mode, align=bool(align), dtype=dtype, layout=layout, n=n, c=c, h=h, w=w, ho=ho, wo=wo,
                        in_q=in_q, out_q=out_q, x=np.ascontiguousarray(x),
                        out_shape=(n, ho, wo, c) if layout == "NHWC" else (n, c, ho, wo)))

    records = list(RECORD_PAIRS.values())
    k = 0
    for h, w, ho, wo, aligns in GEOMETRIES:
        formats = list(FORMATS)
        if (h, w, ho, wo) == (3, 5, 7, 11):
            formats += SWEEP
        if (h, w, ho, wo) == (13, 17, 29, 37):
            formats = [f for f in FORMATS if f[2] not in (15, 7)]
        n = 2 if (h, w, ho, wo) == (3, 5, 6, 10) else 1
        for mode in MODES:
            for align in aligns:
                for dtype, layout, c in formats:
                    name = "%s%s_%dx%d_to_%dx%d_%s_%s_c%d" % (mode, "_ac" if align else "", h, w, ho, wo,
                                                              "i8" if dtype == "int8" else "f16", layout.lower(), c)
                    add(name, mode, align, dtype, layout, n, c, h, w, ho, wo, records[k % 3])
                    k += 1
    # ---- int8 values: every byte once, through every record pair, both modes
    every = np.arange(-128, 128, dtype=np.int16).astype(np.int8).reshape(1, 16, 16, 1)
    for mode in MODES:
        for key, q in RECORD_PAIRS.items():
            add("%s_i8_all_%s_to_32x32" % (mode, key), mode, False, "int8", "NHWC", 1, 1, 16, 16, 32, 32, q, x=every)
            add("%s_ac_i8_all_%s_to_31x31" % (mode, key), mode, True, "int8", "NHWC", 1, 1, 16, 16, 31, 31, q, x=every)
    # ---- binary16 values: infinities, NaNs, -0, a subnormal, +-65504 beside ordinary values; the identity geometry puts
    # zero weights next to them
    for layout, c in (("NHWC", 8), ("NCHW", 2), ("NHWC", 3)):
        x = f16_specials(layout, c)
        for mode in MODES:
            tag = "%s_f16_specials_%s_c%d" % (mode, layout.lower(), c)
            add(tag + "_identity", mode, False, "f16", layout, 1, c, 4, 4, 4, 4, x=x)
            add(tag + "_to_7x9", mode, False, "f16", layout, 1, c, 4, 4, 7, 9, x=x)
            add(tag + "_ac_to_7x9", mode, True, "f16", layout, 1, c, 4, 4, 7, 9, x=x)
            add(tag + "_ac_to_7x7", mode, True, "f16", layout, 1, c, 4, 4, 7, 7, x=x)   # scale 0.5: zero weights on every other tap
    # ---- more than one workgroup
    for mode in MODES:
        add(mode + "_i8_nhwc_1x28x28x32_to_56x56", mode, False, "int8", "NHWC", 1, 32, 28, 28, 56, 56, RECORD_PAIRS["conv"],
            x=tiled("int8", (1, 28, 28, 32)))
        add(mode + "_f16_nchw_1x32x14x14_to_28x28", mode, False, "f16", "NCHW", 1, 32, 14, 14, 28, 28, x=tiled("f16", (1, 32, 14, 14)))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


# ------------------------------------------------------------------------------------ numpy restatement
def scale_of(i, o, align):
    """height_scale / width_scale: ONE float division (resize.c:37-43)"""
    with np.errstate(all="ignore"):
        return np.float32(i - 1) / np.float32(o - 1) if align else np.float32(i) / np.float32(o)


def _coords(o, scale):
    return (np.arange(o, dtype=np.float32) * np.float32(scale)).astype(np.float32)  # y * height_scale, one float product


def nearest_indices(i, o, align):
    s = _coords(o, scale_of(i, o, align)).astype(np.float64)
    idx = np.floor(s + 0.5) if align else np.floor(s)  # round(): halves away from zero (s >= 0)
    return np.minimum(idx.astype(np.int64), i - 1)


def _round_to_f32(fr):
    """the float32 nearest the Fraction `fr`, ties to even"""
    d = np.float32(float(fr))
    best = None
    for cand in (np.nextafter(d, np.float32(-np.inf)), d, np.nextafter(d, np.float32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(fractions.Fraction(float(cand)) - fr)
        even = (int(np.float32(cand).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[1]):
            best = (err, even, cand)
    return np.float32(best[2])


def fma32(a, b, c):
    """fused multiply-add in float32, rounded ONCE.  The product of two float32 values is exact in float64; adding c there
    rounds to 53 bits, and rounding that to 24 can differ from the single rounding only when the float64 sum sits exactly
    half-way between two float32 values: those elements (and tiny ones, where float32 is subnormal) are redone in exact
    rational arithmetic.  Signed zeros, infinities and NaNs come out of the float64 operations as they do of the fused one."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    with np.errstate(all="ignore"):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        r = s.astype(np.float32)
    u = np.ascontiguousarray(s).view(np.uint64)
    doubt = np.isfinite(s) & (s != 0) & (((u & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) | (np.abs(s) < 2.0 ** -120))
    r = np.ascontiguousarray(r)
    for i in np.flatnonzero(doubt.ravel()):
        exact = fractions.Fraction(float(a.ravel()[i])) * fractions.Fraction(float(b.ravel()[i])) + fractions.Fraction(float(c.ravel()[i]))
        r.ravel()[i] = _round_to_f32(exact)
    return r


def bilinear_f32(f, ho, wo, align):
    """shl_ref_resize_bilinear_nhwc_f32 on float32 [n, h, w, c], as the reference's -O3 -mfma build computes it: the (y1, x0)
    term is two products, then the (y0, x0), (y0, x1) and (y1, x1) terms are added, each by ONE fused multiply-add of
    (v w_y) and w_x -- the only one of the twelve ways to fuse the three additions that equals the genuine library's
    float32 output on every element (test_resize_cpu.py holds the comparison)"""
    n, h, w, c = f.shape
    sy, sx = _coords(ho, scale_of(h, ho, align)), _coords(wo, scale_of(w, wo, align))
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    dy, dx = (sy - y0.astype(np.float32)).astype(np.float32), (sx - x0.astype(np.float32)).astype(np.float32)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    wy = ((np.float32(1) - dy).reshape(1, ho, 1, 1), dy.reshape(1, ho, 1, 1))
    wx = ((np.float32(1) - dx).reshape(1, 1, wo, 1), dx.reshape(1, 1, wo, 1))
    terms = [(f[:, y0][:, :, x0], wy[0], wx[0]), (f[:, y1][:, :, x0], wy[1], wx[0]),
             (f[:, y0][:, :, x1], wy[0], wx[1]), (f[:, y1][:, :, x1], wy[1], wx[1])]
    with np.errstate(all="ignore"):
        acc = ((terms[1][0] * terms[1][1]).astype(np.float32) * terms[1][2]).astype(np.float32)
        for v, a, b in (terms[0], terms[2], terms[3]):
            acc = fma32((v * a).astype(np.float32), b, acc)
        # a NaN keeps only its sign on the way to binary16.  An operand NaN goes through the x86 operations with its sign,
        # a NaN the arithmetic makes (inf * 0, inf - inf) is the default one, sign bit set.  A fused multiply-add hands on
        # the NaN of its product operand v w_y before its addend's, so the last such operand of the chain wins and the
        # (y1, x0) term comes last; what only a fused operation makes yields to every operand NaN
        sign = np.zeros(acc.shape, np.int8)  # 0: none yet, 1: positive, 2: negative
        one = np.float32(1)
        for v, a, b in ((terms[3][0], terms[3][1], one), (terms[2][0], terms[2][1], one), (terms[0][0], terms[0][1], one), terms[1]):
            made = np.isnan(((v * a).astype(np.float32) * b).astype(np.float32))
            state = np.where(np.isnan(v), np.where(np.signbit(v), 2, 1), np.where(made, 2, 0)).astype(np.int8)
            sign = np.where(sign == 0, state, sign)
    nan = np.where(sign == 1, np.uint32(0x7FC00000), np.uint32(0xFFC00000)).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(acc), nan, acc).astype(np.float32)


def resize_numpy(case):
    nhwc = case["layout"] == "NHWC"
    x = case["x"] if nhwc else case["x"].transpose(0, 2, 3, 1)
    ho, wo = case["ho"], case["wo"]
    with np.errstate(all="ignore"):
        f = pool_cases.dequantise(np.ascontiguousarray(x), case["dtype"], case["in_q"])
        if case["mode"] == "nearest":
            iy, ix = nearest_indices(x.shape[1], ho, case["align"]), nearest_indices(x.shape[2], wo, case["align"])
            r = f[:, iy][:, :, ix]
        else:
            r = bilinear_f32(f, ho, wo, case["align"])
        out = pool_cases.requantise(np.ascontiguousarray(r), case["dtype"], case["out_q"])
    return np.ascontiguousarray(out if nhwc else out.transpose(0, 3, 1, 2))


def add_numpy(a, b, dtype, qa, qb, qo):
    """shl_ref_add_quant: both operands dequantised, one float32 sum, requantised"""
    with np.errstate(all="ignore"):
        s = (pool_cases.dequantise(a, dtype, qa) + pool_cases.dequantise(b, dtype, qb)).astype(np.float32)
        return np.ascontiguousarray(pool_cases.requantise(s, dtype, qo))


def golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_cases.npz")
    blob = np.load(path)
    return {k: blob[k] for k in blob.files}


# ------------------------------------------------------------------------------------ through csinn_*
def resize_run(fe, api, case, device=None, poison=None, in_skew=0, **override):
    """layer mode through csinn_resize (+ _init).  device: a cases.HipDevice -- both tensors then live in HBM as DMABUF
    tensors, the input `in_skew` ELEMENTS into its allocation.  override: out_shape / out_dtype / mode / scales / out_q /
    in_shape for the refusal tests.  Returns the output, or (status, output buffer) when `poison` (a byte the output is
    pre-filled with) is given."""
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, api, keep)
    np_dt = {"int8": np.int8, "f16": np.float16, "f32": np.float32}
    code = {"int8": pkg.DTYPE_INT8, "f16": pkg.DTYPE_FLOAT16, "f32": pkg.DTYPE_FLOAT32}
    dt = override.get("in_dtype", case["dtype"])
    layout = pkg.LAYOUT_NHWC if case["layout"] == "NHWC" else pkg.LAYOUT_NCHW
    x = case["x"].astype(np_dt[dt]) if dt != case["dtype"] else case["x"]
    if "in_shape" in override:
        x = np.zeros(override["in_shape"], x.dtype)
    out_dt = override.get("out_dtype", dt)
    out = np.zeros(override.get("out_shape", case["out_shape"]), dtype=np_dt[out_dt])
    if poison is not None:
        out.view(np.uint8)[...] = poison
    allocs = []

    def tensor(arr, q, name, dtype, skew=0, scales=None):
        ptr = None
        if device is not None:
            base = device.alloc(arr.nbytes + 64)
            allocs.append(base)
            ptr = base + skew * arr.itemsize
            device.upload(ptr, arr)
        return pkg.make_tensor(fe, keep, arr.shape, code[dtype], layout, data=arr, scales=scales or (q[0],), zps=(q[1],),
                               name=name, sess=sess, device_ptr=ptr), ptr

    t_x, _ = tensor(x, case["in_q"], b"in", dt, skew=in_skew, scales=override.get("scales"))
    t_out, dev_out = tensor(out, override.get("out_q", case["out_q"]), b"out", out_dt)
    params = pkg.resize_params(fe, keep, api, layout, override.get("mode", MODES[case["mode"]]),
                               override.get("align", case["align"]), sess)
    rc = fe.csinn_resize_init(t_x, t_out, params)
    if rc == pkg.CSINN_TRUE:
        rc = fe.csinn_resize(t_x, t_out, params)
    if dev_out is not None:
        out = device.download(dev_out, out.shape, out.dtype)
    for p in allocs:
        device.free(p)
    if poison is not None:
        return rc, out
    if rc != pkg.CSINN_TRUE:
        raise pkg.MI355XError("csinn_resize returned %d" % rc)
    return out


def reference_run(fe, case):
    """the genuine library's answer: NCHW nearest batches are driven one image at a time and stacked, since the reference
    advances its output pointer by the INPUT's batch size there (resize.c:179, :397)"""
    if case["layout"] == "NCHW" and case["mode"] == "nearest" and case["n"] > 1:
        outs = []
        for i in range(case["n"]):
            one = dict(case, n=1, x=np.ascontiguousarray(case["x"][i:i + 1]), out_shape=(1,) + tuple(case["out_shape"][1:]))
            outs.append(resize_run(fe, pkg.API_REF, one))
        return np.concatenate(outs, axis=0)
    return resize_run(fe, pkg.API_REF, case)


def resize_desc(case, **override):
    """struct shl_mi355x_resize_desc of a case: the scales by one float32 division each, the int8 nearest table by the
    restatement's own dequantise -> requantise"""
    d = pkg.ResizeDesc()
    d.dtype = pkg.SHL_I8 if case["dtype"] == "int8" else pkg.SHL_F16
    d.layout = pkg.SHL_NHWC if case["layout"] == "NHWC" else pkg.SHL_NCHW
    d.n, d.c, d.in_h, d.in_w, d.out_h, d.out_w = case["n"], case["c"], case["h"], case["w"], case["ho"], case["wo"]
    d.mode = MODES[case["mode"]]
    d.align_corners = int(case["align"])
    for k, v in override.items():
        setattr(d, k, v)
    if not (d.align_corners and (d.out_h == 1 or d.out_w == 1)) and d.out_h > 0 and d.out_w > 0:
        d.height_scale = float(scale_of(d.in_h, d.out_h, d.align_corners))
        d.width_scale = float(scale_of(d.in_w, d.out_w, d.align_corners))
    (d.in_scale, d.in_zp), (d.out_scale, d.out_zp) = case["in_q"], case["out_q"]
    if case["dtype"] == "int8":
        every = np.arange(256, dtype=np.uint8).view(np.int8)
        with np.errstate(all="ignore"):
            table = pool_cases.requantise(pool_cases.dequantise(every, "int8", case["in_q"]), "int8", case["out_q"])
        d.table[:] = table.view(np.uint8).tolist()
    return d


# ------------------------------------------------------------------------------------ a feature-pyramid model
class PyramidNet:
    """data (8 ch) -> stem 3x3 s2 + relu (C3, 16 ch) -> 3x3 s2 + relu (C4, 32 ch) -> 3x3 s2 + relu (C5, 32 ch) -> lateral
    1x1 on C5 (16 ch) -> resize nearest 2x -> add(., lateral 1x1 of C4) -> 3x3 -> resize bilinear to C3's size -> concat with
    C3 -> 1x1 (32 ch) -> global_avgpool -> classifier -> softmax, int8 NHWC or fp16 NCHW, through the csinn session API in
    graph mode: the top-down path of an FPN.  variant 0: 16x16 input, maps 8 / 4 / 2, bilinear 4 -> 8; variant 1: 13x13
    input, maps 7 / 4 / 2, bilinear 4 -> 7 with align_corners (scale 3 / 6).  The seed is one at which the C oracle's
    binary16 convolutions equal the genuine library's on both inputs (its NCHW path sums in another order, and about one
    output in a thousand falls on a tie: seeds 53, 55, 57 do not qualify), so that test_resize_cpu.py can hold the whole
    chain against the genuine graph executor bit for bit."""

    def __init__(self, dtype="int8", layout="NHWC", variant=0, seed=54, classes=24):
        self.dtype, self.layout, self.variant, self.classes = dtype, layout, variant, classes
        self.hw = hw = (16, 13)[variant]
        self.align = bool(variant)
        int8 = dtype == "int8"
        rng = np.random.default_rng(seed)
        q1 = lambda s, z: _q(s, z) if int8 else _q(1.0, 0)
        self.q_in = q1(2.0 ** -4, -5)
        half = lambda h: (h + 2 - 3) // 2 + 1
        self.h3, self.h4, self.h5 = half(hw), half(half(hw)), half(half(half(hw)))
        assert 2 * self.h5 == self.h4

        def conv(cin, cout, k, stride, act, hin, q_prev, out_q, k_log2=-7):
            case = cases.make_case(int(rng.integers(1 << 30)), layout=layout, dtype=dtype, n=1, h=hin, w=hin, c=cin, co=cout,
                                   k=(k, k), stride=(stride, stride), pad=(k // 2,) * 4, act=act)
            if int8:
                case["in_scale"], case["in_zp"] = q_prev
                case["k_scale"] = np.array([2.0 ** k_log2], dtype=np.float32)
                case["b_scale"] = (np.float32(case["in_scale"]) * case["k_scale"]).astype(np.float32)
                case["bias"] = rng.integers(-2000, 2001, (case["co"],), dtype=np.int32)
                case["out_scale"], case["out_zp"] = out_q
            return case

        q = self.q = {}
        q["c3"], q["c4"], q["c5"] = q1(2.0 ** -3, -100), q1(2.0 ** -3, -90), q1(2.0 ** -2, -100)
        q["l5"], q["up5"], q["l4"] = q1(2.0 ** -3, -10), q1(2.0 ** -3, 4), q1(2.0 ** -3, 7)
        q["sum"], q["p4"], q["up4"] = q1(2.0 ** -2, -3), q1(2.0 ** -2, 11), q1(0.21, 5)
        q["cat"], q["mix"], q["gap"] = q1(2.0 ** -2, -40), q1(2.0 ** -2, -20), q1(2.0 ** -4, -60)
        cv = self.cv = {}
        cv["c3"] = conv(8, 16, 3, 2, 1, hw, self.q_in, q["c3"])
        cv["c4"] = conv(16, 32, 3, 2, 1, self.h3, q["c3"], q["c4"])
        cv["c5"] = conv(32, 32, 3, 2, 1, self.h4, q["c4"], q["c5"])
        cv["l5"] = conv(32, 16, 1, 1, 0, self.h5, q["c5"], q["l5"], k_log2=-6)
        cv["l4"] = conv(32, 16, 1, 1, 0, self.h4, q["c4"], q["l4"], k_log2=-6)
        cv["p4"] = conv(16, 16, 3, 1, 0, self.h4, q["sum"], q["p4"], k_log2=-6)
        cv["mix"] = conv(32, 32, 1, 1, 0, self.h3, q["cat"], q["mix"], k_log2=-6)
        cv["fc"] = conv(32, classes, 1, 1, 0, 1, q["gap"], q1(2.0 ** -4, -11), k_log2=-6)
        q["fc"] = q1(cv["fc"]["out_scale"], cv["fc"]["out_zp"])
        self.q_out = _q(1.0 / 256, -128) if int8 else _q(1.0, 0)

    def _shape(self, c, h):
        return (1, h, h, c) if self.layout == "NHWC" else (1, c, h, h)

    @property
    def c_axis(self):
        return 3 if self.layout == "NHWC" else 1

    def input(self, k):
        rng = np.random.default_rng(900 + k)
        shape = self._shape(8, self.hw)
        return rng.integers(-100, 100, shape, dtype=np.int8) if self.dtype == "int8" else rng.standard_normal(shape).astype(np.float16)

    # -- oracle chain: convolutions, the pool and softmax through the C oracle, resize / add / concat through numpy
    def oracle(self, x):
        form = "ref" if self.dtype == "int8" else "f16"
        q, cv = self.q, self.cv

        def run_conv(name, cur):
            case = dict(cv[name])
            case["input"] = np.ascontiguousarray(cur)
            return cases.oracle_run(case, form)

        def resize(cur, mode, align, h, ho, in_q, out_q):
            c = cur.shape[self.c_axis]
            return resize_numpy(dict(mode=mode, align=align, dtype=self.dtype, layout=self.layout, x=cur, n=1, c=c, h=h, w=h,
                                     ho=ho, wo=ho, in_q=in_q, out_q=out_q))
        c3 = run_conv("c3", x)
        c4 = run_conv("c4", c3)
        c5 = run_conv("c5", c4)
        up5 = resize(run_conv("l5", c5), "nearest", False, self.h5, self.h4, q["l5"], q["up5"])
        s = add_numpy(up5, run_conv("l4", c4), self.dtype, q["up5"], q["l4"], q["sum"])
        up4 = resize(run_conv("p4", s), "bilinear", self.align, self.h4, self.h3, q["p4"], q["up4"])
        cat = concat_cases.concat_numpy(dict(axis=self.c_axis, dtype=self.dtype, xs=[up4, c3], in_qs=[q["up4"], q["c3"]],
                                             out_q=q["cat"], out_shape=self._shape(32, self.h3)))
        mix = run_conv("mix", cat)
        g = tail.siso_oracle(dict(kind="pool", x=mix, dtype=self.dtype, layout=self.layout, axis=1, in_q=q["mix"], out_q=q["gap"]))
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

        def resize(name, t_in, c, ho, rec, mode, align):
            t_out = T(self._shape(c, ho), rec, name + b"_out")
            ops.append(("csinn_resize", (t_in, t_out, pkg.resize_params(fe, keep, api, act_l, MODES[mode], align, sess, name))))
            return t_out

        t_in = T(self._shape(8, self.hw), self.q_in, b"data")
        c3 = conv("c3", t_in, 16, self.h3, q["c3"], stem="csinn_conv2d_relu")
        c4 = conv("c4", c3, 32, self.h4, q["c4"], stem="csinn_conv2d_relu")
        c5 = conv("c5", c4, 32, self.h5, q["c5"], stem="csinn_conv2d_relu")
        l5 = conv("l5", c5, 16, self.h5, q["l5"])
        up5 = resize(b"up5", l5, 16, self.h4, q["up5"], "nearest", False)
        l4 = conv("l4", c4, 16, self.h4, q["l4"])
        t_sum = T(self._shape(16, self.h4), q["sum"], b"sum_out")
        ops.append(("csinn_add", (up5, l4, t_sum, pkg.siso_params(fe, keep, api, "add", act_l, 1, sess, b"add"))))
        p4 = conv("p4", t_sum, 16, self.h4, q["p4"])
        up4 = resize(b"up4", p4, 16, self.h3, q["up4"], "bilinear", self.align)
        t_cat = T(self._shape(32, self.h3), q["cat"], b"cat_out")
        ops.append(("csinn_concat", (pkg.tensor_array(keep, [up4, c3]), t_cat,
                                     pkg.concat_params(fe, keep, api, act_l, 2, self.c_axis, sess, b"cat"))))
        mix = conv("mix", t_cat, 32, self.h3, q["mix"])
        t_g = T(self._shape(32, 1), q["gap"], b"gap_out")
        ops.append(("csinn_global_avgpool2d", (mix, t_g, pkg.siso_params(fe, keep, api, "pool", act_l, self.c_axis, sess, b"gap"))))
        logits = conv("fc", t_g, self.classes, 1, q["fc"])
        prob = T(self._shape(self.classes, 1), self.q_out, b"softmax_out")
        ops.append(("csinn_softmax", (logits, prob, pkg.siso_params(fe, keep, api, "softmax", act_l, self.c_axis, sess, b"softmax"))))
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

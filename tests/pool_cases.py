"""Shared helpers for the windowed pools (CSINN_OP_MAXPOOL2D / CSINN_OP_AVGPOOL2D).

  pool_cases()                  deterministic single-op problems: the smallest shapes at which each kernel form
                                (NHWC 16-byte pieces, NCHW rows of four, one output per thread) can still go wrong
  pool_numpy(case)              plain numpy restatement of the reference (source/reference/maxpool.c:21-124,
                                averagepool.c:21-138 inside shl_ref_siso_callback_base): a float32 loop in the
                                reference's tap order
  pool_run(fe, api, case)       csinn_<op>_init + csinn_<op> through a front-end (layer mode)
  PoolNet                       conv -> maxpool -> conv -> add -> relu -> avgpool -> global_avgpool -> classifier -> softmax
                                through the csinn session API (graph mode), with an oracle replay
The genuine library's outputs for pool_cases() live in tests/golden/pool_cases.npz (make_pool_golden.py).
"""
import zlib

import numpy as np

import cases
import tail
from cases import pkg

FLT_MAX = np.float32(3.4028234663852886e38)


def _q(scale, zp):
    return (float(np.float32(scale)), int(zp))


Q_SAME = _q(2.0 ** -4, -5)                                   # in == out: the identity path of the int8 max
Q_POW2 = (_q(2.0 ** -4, -5), _q(2.0 ** -3, 9))               # exact arithmetic, different zero points
Q_CONV = (_q(0.0473, -9), _q(0.0219, 4))                     # converter scales
Q_SAT = (_q(2.0 ** -4, -5), _q(2.0 ** -6, 100))              # the out record saturates
Q_F16 = (_q(1.0, 0), _q(1.0, 0))


def out_dim(i, k, s, p0, p1, ceil_mode):
    """shl_gref_pooling2d_infer_shape (source/graph_ref/utils.c:146-187)"""
    return (i + p0 + p1 - k + (s - 1 if ceil_mode else 0)) // s + 1


# (name, in_h, in_w, kernel, stride, pad (top, left, down, right), ceil_mode)
GEOMETRIES = [
    ("k3s2p1_8x8", 8, 8, (3, 3), (2, 2), (1, 1, 1, 1), 0),      # ResNet's pool, even
    ("k3s2p1_7x7", 7, 7, (3, 3), (2, 2), (1, 1, 1, 1), 0),      # ... and odd
    ("k2s2_8x8", 8, 8, (2, 2), (2, 2), (0, 0, 0, 0), 0),
    ("k3s1p1_6x6", 6, 6, (3, 3), (1, 1), (1, 1, 1, 1), 0),
    ("k3x2s2x1_9x6", 9, 6, (3, 2), (2, 1), (0, 0, 0, 0), 0),    # H != W, kernel and stride not square
    ("k3s2asym_8x8", 8, 8, (3, 3), (2, 2), (0, 1, 1, 0), 0),    # pad top 0, left 1, down 1, right 0
    ("k2s2ceil_7x7", 7, 7, (2, 2), (2, 2), (0, 0, 0, 0), 1),    # 4 outputs, the last window partial
    ("k5p2_4x4", 4, 4, (5, 5), (1, 1), (2, 2, 2, 2), 0),        # every window clipped
]
# (dtype, layout, channels): one 16-byte piece; no multiple of 16 bytes (one output per thread); f16 piece; NCHW rows
FORMATS = [("int8", "NHWC", 16), ("int8", "NHWC", 20), ("f16", "NHWC", 8), ("int8", "NCHW", 3), ("f16", "NCHW", 2)]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _data(rng, dtype, shape):
    if dtype == "int8":
        return rng.integers(-128, 128, shape, dtype=np.int8)
    return (3.0 * rng.standard_normal(shape)).astype(np.float16)


def _f16_specials(layout, c, nan):
    """1 x 4 x 4 x c for 2x2 stride-2 windows: window (0,0) signed zeros, (0,1) subnormals, (1,0) infinities,
    (1,1) values whose sum leaves the binary16 range; nan: a NaN beside finite values and one all-NaN window"""
    x = np.zeros((1, 4, 4, c), dtype=np.uint16)
    rng = np.random.default_rng(99 + c)
    x[:] = (2.0 * rng.standard_normal(x.shape)).astype(np.float16).view(np.uint16)
    even, odd = slice(0, None, 2), slice(1, None, 2)
    x[0, 0, 0, even], x[0, 0, 1, even], x[0, 1, 0, even], x[0, 1, 1, even] = 0x8000, 0x0000, 0x8000, 0x0000
    x[0, 0, 0, odd], x[0, 0, 1, odd], x[0, 1, 0, odd], x[0, 1, 1, odd] = 0x0000, 0x8000, 0x8000, 0x8000
    x[0, 0, 2, :], x[0, 0, 3, :], x[0, 1, 2, :], x[0, 1, 3, :] = 0x0001, 0x8001, 0x8000, 0x8001
    x[0, 1, 3, odd] = 0x0002
    x[0, 2, 0, even] = 0x7C00   # +inf beside finite values
    x[0, 2:4, 0:2, odd] = 0xFC00  # a window of -inf
    x[0, 2:4, 2:4, :] = 0x7BFF  # 65504 four times: the sum leaves the binary16 range
    x[0, 3, 3, odd] = 0x7BFE    # 65472: the average 65496 rounds at the top binade
    if nan:
        x[0, 0, 0, even] = 0x7E00          # NaN first, finite values behind it
        x[0, 0, 3, even] = 0xFE00          # NaN in the middle of a window
        x[0, 2:4, 0:2, even] = 0x7E01      # all NaN
    x = x.view(np.float16)
    return x if layout == "NHWC" else np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def pool_cases():
    out = []

    def add(name, kind, dtype, layout, n, c, h, w, kernel, stride, pad, ceil_mode=0, cip=0, q=None, x=None):
        in_q, out_q = q if q is not None else Q_F16
        if dtype == "f16":
            in_q, out_q = Q_F16
        ho = out_dim(h, kernel[0], stride[0], pad[0], pad[2], ceil_mode)
        wo = out_dim(w, kernel[1], stride[1], pad[1], pad[3], ceil_mode)
        shape = (n, h, w, c) if layout == "NHWC" else (n, c, h, w)
        if x is None:
            x = _data(_rng(name), dtype, shape)
        assert x.shape == shape, (name, x.shape, shape)
        out.append(dict(name=name, kind=kind, dtype=dtype, layout=layout, n=n, c=c, h=h, w=w, ho=ho, wo=wo,
                        kernel=tuple(kernel), stride=tuple(stride), pad=tuple(pad), ceil_mode=ceil_mode, cip=cip,
                        in_q=in_q, out_q=out_q, x=np.ascontiguousarray(x),
                        out_shape=(n, ho, wo, c) if layout == "NHWC" else (n, c, ho, wo)))

    records = [(Q_SAME, Q_SAME), Q_POW2, Q_CONV]
    k = 0
    for gname, h, w, kernel, stride, pad, ceil_mode in GEOMETRIES:
        clipped = any(pad) or ceil_mode
        for dtype, layout, c in FORMATS:
            n = 3 if gname == "k3s2p1_7x7" else 1  # batch 3: image strides
            tag = "%s_%s_%s_c%d" % (gname, dtype, layout.lower(), c)
            add("max_" + tag, "max", dtype, layout, n, c, h, w, kernel, stride, pad, ceil_mode, 0, records[k % 3])
            add("avg_" + tag, "avg", dtype, layout, n, c, h, w, kernel, stride, pad, ceil_mode, 0, records[(k + 1) % 3])
            if clipped:
                add("avgcip_" + tag, "avg", dtype, layout, n, c, h, w, kernel, stride, pad, ceil_mode, 1,
                    records[(k + 2) % 3])
            k += 1
    res = ((3, 3), (2, 2), (1, 1, 1, 1))
    for kind in ("max", "avg"):
        # channels: three 16-byte pieces, fewer channels than a dword, three f16 pieces
        add(kind + "_c48_i8_nhwc", kind, "int8", "NHWC", 2, 48, 7, 5, *res, q=Q_CONV)
        add(kind + "_c3_i8_nhwc", kind, "int8", "NHWC", 2, 3, 7, 5, *res, q=Q_POW2)
        add(kind + "_c24_f16_nhwc", kind, "f16", "NHWC", 2, 24, 7, 5, *res)
        # NCHW rows of 1, 4, 5 and 7 outputs: tails of the groups of four, packed stores at odd addresses
        for wo in (1, 4, 5, 7):
            for dtype in ("int8", "f16"):
                add("%s_nchw_wo%d_%s" % (kind, wo, dtype), kind, dtype, "NCHW", 2, 3, 6, 2 * wo, (2, 2), (2, 2),
                    (0, 0, 0, 0), q=Q_CONV)
        # NCHW rows wide enough for groups whose windows lie inside the image (fetched as spans of whole dwords), odd
        # row length: every byte alignment
        for kk, ss, pp in ((3, 2, 1), (2, 2, 0), (3, 1, 1)):
            for dtype in ("int8", "f16"):
                add("%s_nchw_span_k%ds%d_%s" % (kind, kk, ss, dtype), kind, dtype, "NCHW", 2, 2, 5, 37, (kk, kk), (ss, ss),
                    (pp,) * 4, q=Q_CONV if kk == 3 else (Q_SAME, Q_SAME))
        add(kind + "_nchw_c1_i8", kind, "int8", "NCHW", 1, 1, 9, 11, *res, q=(Q_SAME, Q_SAME))
        add(kind + "_nchw_c1_f16", kind, "f16", "NCHW", 1, 1, 9, 11, *res)
        # int8 records: both extremes in every window position, a saturating out record
        for layout, c in (("NHWC", 16), ("NCHW", 3), ("NHWC", 5)):
            shape = (1, 8, 8, c) if layout == "NHWC" else (1, c, 8, 8)
            ext = _rng(kind + layout + "ext").choice(np.array([-128, 127], dtype=np.int8), shape)
            for qn, q in (("same", (Q_SAME, Q_SAME)), ("conv", Q_CONV), ("pow2", Q_POW2)):
                add("%s_extremes_%s_%s_c%d" % (kind, qn, layout.lower(), c), kind, "int8", layout, 1, c, 8, 8, *res, q=q, x=ext)
            add("%s_saturating_%s_c%d" % (kind, layout.lower(), c), kind, "int8", layout, 1, c, 8, 8, *res, q=Q_SAT)
        # binary16 special values
        for layout, c in (("NHWC", 8), ("NCHW", 4), ("NHWC", 3)):
            add("%s_f16_specials_%s_c%d" % (kind, layout.lower(), c), kind, "f16", layout, 1, c, 4, 4, (2, 2), (2, 2),
                (0, 0, 0, 0), x=_f16_specials(layout, c, nan=False))
            if kind == "max":
                add("max_f16_nan_%s_c%d" % (layout.lower(), c), "max", "f16", layout, 1, c, 4, 4, (2, 2), (2, 2),
                    (0, 0, 0, 0), x=_f16_specials(layout, c, nan=True))
    # more than one wave and workgroup per image
    add("max_resnet_2x56x56x64_i8_nhwc", "max", "int8", "NHWC", 2, 64, 56, 56, *res, q=Q_CONV)
    add("avg_1x40x40x32_f16_nhwc", "avg", "f16", "NHWC", 1, 32, 40, 40, *res, cip=1)
    add("max_2x8x56x56_f16_nchw", "max", "f16", "NCHW", 2, 8, 56, 56, *res)
    add("avg_2x8x56x56_i8_nchw", "avg", "int8", "NCHW", 2, 8, 56, 56, *res, q=Q_POW2)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


# ------------------------------------------------------------------------------------ numpy restatement
def f32_to_f16_ref(v):
    """float32_to_float16_base (source/nn2/utils.c:576-620): saturate beyond +-65519, drop 12 mantissa bits,
    scale by 2^-112, + 0x1000, >> 13"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    u = v.view(np.uint32)
    sign = u & np.uint32(0x80000000)
    a = u ^ sign
    scaled = (a & np.uint32(0xFFFFF000)).view(np.float32) * np.float32(2.0 ** -112)
    t = np.minimum(scaled.view(np.uint32) + np.uint32(0x1000), np.uint32(31 << 23)) >> np.uint32(13)
    h = np.where(a > 0x7F800000, np.uint32(0x7FFF), np.where(a == 0x7F800000, np.uint32(0x7C00), t))
    h = h | (sign >> np.uint32(16))
    h = np.where(v > np.float32(65519.0), np.uint32(0x7BFF), np.where(v < np.float32(-65519.0), np.uint32(0xFBFF), h))
    return h.astype(np.uint16)


def dequantise(x, dtype, q):
    if dtype == "int8":  # int8_to_float_base (source/nn2/utils.c:499-502)
        return (x.astype(np.float32) - np.float32(q[1])) * np.float32(q[0])
    return x.astype(np.float32)  # exact


def requantise(v, dtype, q):
    if dtype == "int8":  # float_to_int8_base (:550-560)
        r = np.rint(v / np.float32(q[0])) + np.float32(q[1])
        return np.clip(r, -128, 127).astype(np.int8)
    return f32_to_f16_ref(v).view(np.float16)


def pool_numpy(case):
    nhwc = case["layout"] == "NHWC"
    x = case["x"] if nhwc else case["x"].transpose(0, 2, 3, 1)
    kh, kw = case["kernel"]
    sh, sw = case["stride"]
    pt, pl = case["pad"][0], case["pad"][1]
    n, h, w, c = x.shape
    ho, wo = case["ho"], case["wo"]
    with np.errstate(all="ignore"):
        f = dequantise(x, case["dtype"], case["in_q"])
        res = np.empty((n, ho, wo, c), dtype=np.float32)
        for oy in range(ho):
            y0 = oy * sh - pt
            ys, ye = max(0, -y0), min(kh, h - y0)
            for ox in range(wo):
                x0 = ox * sw - pl
                xs, xe = max(0, -x0), min(kw, w - x0)
                if case["kind"] == "max":
                    acc = np.full((n, c), -FLT_MAX, dtype=np.float32)
                    for ky in range(ys, ye):
                        for kx in range(xs, xe):
                            v = f[:, y0 + ky, x0 + kx, :]
                            acc = np.where(v >= acc, v, acc)  # the C library's fmax: a NaN never wins, the last zero stays
                else:
                    acc = np.zeros((n, c), dtype=np.float32)
                    count = 0
                    for ky in range(ys, ye):
                        for kx in range(xs, xe):
                            acc = acc + f[:, y0 + ky, x0 + kx, :]
                            count += 1
                    if case["cip"]:
                        count = kh * kw
                    acc = acc / np.float32(count)
                res[:, oy, ox, :] = acc
        out = requantise(res, case["dtype"], case["out_q"])
    return out if nhwc else np.ascontiguousarray(out.transpose(0, 3, 1, 2))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.dtype == np.float16 else a


def assert_same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g.ravel() != w.ravel())
    assert bad.size == 0, "%s: %d of %d outputs differ, first at %d: got %r want %r" % (
        what, bad.size, g.size, bad[0], g.ravel()[bad[0]], w.ravel()[bad[0]])


# ------------------------------------------------------------------------------------ through csinn_*
def csinn_layout(case):
    return pkg.LAYOUT_NHWC if case["layout"] == "NHWC" else pkg.LAYOUT_NCHW


def pool_run(fe, api, case, device=None, poison=None, in_q=None, x=None, out_shape=None):
    """layer mode through csinn_maxpool2d / csinn_avgpool2d (+ _init); device: run on DMABUF tensors in HBM.
    Returns the output, or (status, output buffer) when `poison` (a byte the output is pre-filled with) is given:
    the refusal tests look at both."""
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, api, keep)
    x = np.ascontiguousarray(case["x"] if x is None else x)
    int8 = case["dtype"] == "int8"
    dt = pkg.DTYPE_INT8 if int8 else pkg.DTYPE_FLOAT16
    layout = csinn_layout(case)
    out = np.zeros(out_shape or case["out_shape"], dtype=x.dtype)
    if poison is not None:
        out.view(np.uint8)[...] = poison
    dev_in = dev_out = None
    if device is not None:
        dev_in = device.alloc(x.nbytes)
        device.upload(dev_in, x)
        dev_out = device.alloc(out.nbytes)
        device.upload(dev_out, out)
    (si, zi), (so, zo) = in_q or case["in_q"], case["out_q"]
    t_in = pkg.make_tensor(fe, keep, x.shape, dt, layout, data=x, scales=(si,), zps=(zi,), name=b"in", sess=sess,
                           device_ptr=dev_in)
    t_out = pkg.make_tensor(fe, keep, out.shape, dt, layout, data=out, scales=(so,), zps=(zo,), name=b"out", sess=sess,
                            device_ptr=dev_out)
    params = pkg.pool_params(fe, keep, api, layout, case["kernel"], case["stride"], case["pad"], case["ceil_mode"],
                             case["cip"], sess)
    stem = "csinn_maxpool2d" if case["kind"] == "max" else "csinn_avgpool2d"
    rc = getattr(fe, stem + "_init")(t_in, t_out, params)
    if rc == pkg.CSINN_TRUE:
        rc = getattr(fe, stem)(t_in, t_out, params)
    if device is not None:
        out = device.download(dev_out, out.shape, out.dtype)
        device.free(dev_in)
        device.free(dev_out)
    if poison is not None:
        return rc, out
    if rc != pkg.CSINN_TRUE:
        raise pkg.MI355XError("%s returned %d" % (stem, rc))
    return out


def pool_desc(case):
    d = pkg.PoolDesc()
    d.kind = pkg.POOL_MAX if case["kind"] == "max" else pkg.POOL_AVG
    d.dtype = pkg.SHL_I8 if case["dtype"] == "int8" else pkg.SHL_F16
    d.layout = pkg.SHL_NHWC if case["layout"] == "NHWC" else pkg.SHL_NCHW
    d.batch, d.c, d.in_h, d.in_w, d.out_h, d.out_w = case["n"], case["c"], case["h"], case["w"], case["ho"], case["wo"]
    d.kernel_h, d.kernel_w = case["kernel"]
    d.stride_h, d.stride_w = case["stride"]
    d.pad_top, d.pad_left = case["pad"][0], case["pad"][1]
    d.count_include_pad = int(case["cip"])
    (d.in_scale, d.in_zp), (d.out_scale, d.out_zp) = case["in_q"], case["out_q"]
    return d


def golden():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool_cases.npz")
    blob = np.load(path)
    return {k: blob[k] for k in blob.files}


# ------------------------------------------------------------------------------------ a model with both pools
class PoolNet:
    """data -> conv3x3+relu (16 -> 32 @16x16) -> maxpool 3x3 s2 pad 1 -> conv3x3 -> add(., maxpool output) -> relu ->
    avgpool2d 2x2 s2 -> global_avgpool2d -> 1x1 classifier -> softmax, int8 NHWC or fp16 NCHW, through the csinn
    session API in graph mode: ResNet's stem pool and a residual block whose shortcut is the pooled tensor."""

    def __init__(self, dtype="int8", layout="NHWC", seed=23, hw=16, c0=16, c1=32, classes=24):
        self.dtype, self.layout, self.hw, self.c0, self.c1, self.classes = dtype, layout, hw, c0, c1, classes
        int8 = dtype == "int8"
        rng = np.random.default_rng(seed)
        q1 = lambda s, z: _q(s, z) if int8 else _q(1.0, 0)
        self.q_in = q1(2.0 ** -4, -5)

        def conv(cin, cout, k, pad, act, hin, q_prev, out_log2, zp, k_log2=-7):
            case = cases.make_case(int(rng.integers(1 << 30)), layout=layout, dtype=dtype, n=1, h=hin, w=hin, c=cin, co=cout,
                                   k=(k, k), pad=(pad,) * 4, act=act)
            if int8:
                case["in_scale"], case["in_zp"] = q_prev
                case["k_scale"] = np.array([2.0 ** k_log2], dtype=np.float32)
                case["b_scale"] = (np.float32(case["in_scale"]) * case["k_scale"]).astype(np.float32)
                case["bias"] = rng.integers(-2000, 2001, (case["co"],), dtype=np.int32)
                case["out_scale"], case["out_zp"] = 2.0 ** out_log2, zp
            return case

        h2 = out_dim(hw, 3, 2, 1, 1, 0)
        h3 = out_dim(h2, 2, 2, 0, 0, 0)
        self.h2, self.h3 = h2, h3
        self.conv1 = conv(c0, c1, 3, 1, 1, hw, self.q_in, -3, -11)
        self.q_c1 = q1(self.conv1["out_scale"], self.conv1["out_zp"])
        self.q_mp = q1(2.0 ** -3, -20)        # another record than its input's: the max is requantised
        self.conv2 = conv(c1, c1, 3, 1, 0, h2, self.q_mp, -2, 3)
        self.q_c2 = q1(self.conv2["out_scale"], self.conv2["out_zp"])
        self.q_add = q1(2.0 ** -2, -30)
        self.q_relu = q1(2.0 ** -3, -128)
        self.q_ap = q1(2.0 ** -3, -120)
        self.q_gap = q1(2.0 ** -4, -128)
        self.fc = conv(c1, classes, 1, 0, 0, 1, self.q_gap, -4, -11, k_log2=-10)  # logits a few units apart
        self.q_fc = q1(self.fc["out_scale"], self.fc["out_zp"])
        self.q_out = _q(1.0 / 256, -128) if int8 else _q(1.0, 0)

    def _shape(self, c, h):
        return (1, h, h, c) if self.layout == "NHWC" else (1, c, h, h)

    def input(self, k):
        rng = np.random.default_rng(700 + k)
        shape = self._shape(self.c0, self.hw)
        return rng.integers(-100, 100, shape, dtype=np.int8) if self.dtype == "int8" else rng.standard_normal(shape).astype(np.float16)

    def _pool_case(self, kind, x, c, h, kernel, stride, pad, in_q, out_q):
        ho = out_dim(h, kernel[0], stride[0], pad[0], pad[2], 0)
        return dict(kind=kind, dtype=self.dtype, layout=self.layout, x=x, kernel=kernel, stride=stride, pad=pad, cip=0,
                    ho=ho, wo=ho, in_q=in_q, out_q=out_q)

    # -- oracle chain: convolutions through cases.oracle_run, pools through the numpy restatement
    def oracle(self, x):
        form = "ref" if self.dtype == "int8" else "f16"
        so = lambda **kw: tail.siso_oracle(dict(dtype=self.dtype, layout=self.layout, axis=1, **kw))

        def run_conv(case, cur):
            case = dict(case)
            case["input"] = np.ascontiguousarray(cur)
            return cases.oracle_run(case, form)
        y1 = run_conv(self.conv1, x)
        mp = pool_numpy(self._pool_case("max", y1, self.c1, self.hw, (3, 3), (2, 2), (1, 1, 1, 1), self.q_c1, self.q_mp))
        y2 = run_conv(self.conv2, mp)
        s = so(kind="add", x=y2, y=mp, in_q=self.q_c2, in1_q=self.q_mp, out_q=self.q_add)
        r = so(kind="relu", x=s, in_q=self.q_add, out_q=self.q_relu)
        ap = pool_numpy(self._pool_case("avg", r, self.c1, self.h2, (2, 2), (2, 2), (0, 0, 0, 0), self.q_relu, self.q_ap))
        g = so(kind="pool", x=ap, in_q=self.q_ap, out_q=self.q_gap)
        logits = run_conv(self.fc, g)
        return tail.siso_oracle(dict(kind="softmax", x=logits, dtype=self.dtype, layout=self.layout,
                                     axis=3 if self.layout == "NHWC" else 1, in_q=self.q_fc, out_q=self.q_out))

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

        def T(dims, q, name, data=None, const=0, layout=act_l, dtype=dt, scales=None):
            return pkg.make_tensor(fe, keep, dims, dtype, layout, data=data, is_const=const, name=name, sess=sess,
                                   scales=scales if scales is not None else (q[0],), zps=(q[1] if q else 0,))

        def conv_tensors(case, name):
            w_l = pkg.LAYOUT_OHWI if nhwc else pkg.LAYOUT_OIHW
            t_w = T(case["w_shape"], None, name + b"_w", case["kernel"], 1, w_l, scales=tuple(case["k_scale"]))
            t_b = T((case["co"],), None, name + b"_b", case["bias"], 1, pkg.LAYOUT_O, pkg.DTYPE_INT32 if int8 else dt,
                    scales=tuple(case["b_scale"]))
            p = pkg.conv_params(fe, keep, api, act_l, case["stride"], case["pad"], case["dilation"], 1, 0, sess, name)
            return t_w, t_b, p
        c1, h, h2, h3 = self.c1, self.hw, self.h2, self.h3
        t_in = T(self._shape(self.c0, h), self.q_in, b"data")
        t_c1 = T(self._shape(c1, h), self.q_c1, b"conv1_out")
        t_mp = T(self._shape(c1, h2), self.q_mp, b"maxpool_out")
        t_c2 = T(self._shape(c1, h2), self.q_c2, b"conv2_out")
        t_s = T(self._shape(c1, h2), self.q_add, b"sum")
        t_r = T(self._shape(c1, h2), self.q_relu, b"relu_out")
        t_ap = T(self._shape(c1, h3), self.q_ap, b"avgpool_out")
        t_g = T(self._shape(c1, 1), self.q_gap, b"gap_out")
        t_fc = T(self._shape(self.classes, 1), self.q_fc, b"logits")
        t_o = T(self._shape(self.classes, 1), self.q_out, b"prob")
        w1, b1, p1 = conv_tensors(self.conv1, b"conv1")
        w2, b2, p2 = conv_tensors(self.conv2, b"conv2")
        w3, b3, p3 = conv_tensors(self.fc, b"classifier")
        pmp = pkg.pool_params(fe, keep, api, act_l, (3, 3), (2, 2), (1, 1, 1, 1), 0, False, sess, b"maxpool")
        pap = pkg.pool_params(fe, keep, api, act_l, (2, 2), (2, 2), (0, 0, 0, 0), 0, False, sess, b"avgpool")
        pa = pkg.siso_params(fe, keep, api, "add", act_l, 1, sess, b"add")
        pr = pkg.siso_params(fe, keep, api, "relu", act_l, 1, sess, b"relu")
        pg = pkg.siso_params(fe, keep, api, "pool", act_l, 1, sess, b"gap")
        ps = pkg.siso_params(fe, keep, api, "softmax", act_l, 3 if nhwc else 1, sess, b"softmax")
        ops = [("csinn_conv2d_relu", (t_in, t_c1, w1, b1, p1)), ("csinn_maxpool2d", (t_c1, t_mp, pmp)),
               ("csinn_conv2d", (t_mp, t_c2, w2, b2, p2)), ("csinn_add", (t_c2, t_mp, t_s, pa)),
               ("csinn_relu", (t_s, t_r, pr)), ("csinn_avgpool2d", (t_r, t_ap, pap)),
               ("csinn_global_avgpool2d", (t_ap, t_g, pg)), ("csinn_conv2d", (t_g, t_fc, w3, b3, p3)),
               ("csinn_softmax", (t_fc, t_o, ps))]
        for stem, args in ops:
            assert getattr(fe, stem + "_init")(*args) == pkg.CSINN_TRUE, stem
        fe.csinn_set_tensor_entry(t_in, sess)
        fe.csinn_set_input(0, t_in, sess)
        for stem, args in ops:
            assert getattr(fe, stem)(*args) == pkg.CSINN_TRUE, stem
        fe.csinn_set_output(0, t_o, sess)
        rc = fe.csinn_session_setup(sess)
        assert rc == pkg.CSINN_TRUE or getattr(fe, "kind", "") == "reference"
        self._keep, self._sess, self._out_shape, self._in_q = keep, sess, self._shape(self.classes, 1), self.q_in
        return sess

    run = tail.MiniNet.run
    close = tail.MiniNet.close

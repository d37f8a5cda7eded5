"""Transposed convolution (csinn_deconv2d): the case list, a numpy restatement of the device contract in two variants, the
routes a case can take (C ABI, csinn_* on host or DMABUF tensors, the genuine library) and a small decoder for the session
tests.

The contract:
    int8      S = sum (q - zp_in) w over the (iy, ix, ky, kx, ic) that reach the output element, exact;
              f = fl(fl((float)S mult[oc]) + bias_f[oc]);  q = sat8(rint(f / s_out) + zp_out);  relu / relu6 as for conv2d
    binary16  fp32 sum of exact products in ascending (iy, ix, ic), fp32 bias add, the reference's f32 -> f16 rounding
deconv_scatter   the literal scatter of source/reference/deconvolution.c, in its order;
deconv_phase     one ordinary small convolution per output phase, as csrc/deconv.hip's MFMA form computes it: positions
                 outside the image read the pad page (zp_in / 0.0) and the int8 accumulator starts at acc_init.
Every shape exists in an "exact" regime (power-of-two scales, bias scale s_in s_k) and a "general" one (converter-like
scales).  Shapes are tiny on purpose: the kernel can go wrong at tile and phase edges, not at size.
"""
import ctypes as C
import os
import zlib

import numpy as np

import cases
import concat_cases
import eltwise_cases
import pool_cases
import tail
from cases import pkg

GATHER, PHASE = "gather", "phase"
HERE = os.path.dirname(os.path.abspath(__file__))


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def out_extent(i, k, s, p0, p1, out_pad=0):
    """shl_gref_deconv2d_infer_shape with dilation 1, plus output_padding"""
    return (i - 1) * s - (p0 + p1) + (k - 1) + 1 + out_pad


def make(name, dtype="int8", layout="NHWC", dw=False, n=1, h=4, w=4, c=32, co=32, k=(2, 2), stride=(2, 2), pad=(0, 0, 0, 0),
         out_pad=(0, 0), regime="exact", act=0, has_bias=True, per_channel=False, in_zp=-5, normal=False):
    """pad = (top, left, down, right).  normal: binary16 values from a normal distribution instead of multiples of 2^-4"""
    rng = _rng(name)
    kh, kw = k
    if dw:
        co = c
    ho = out_extent(h, kh, stride[0], pad[0], pad[2], out_pad[0])
    wo = out_extent(w, kw, stride[1], pad[1], pad[3], out_pad[1])
    nhwc = layout == "NHWC"
    if dw:
        w_shape = (1, kh, kw, c) if nhwc else (c, 1, kh, kw)
    else:
        w_shape = (co, kh, kw, c) if nhwc else (c, co, kh, kw)
    case = dict(name=name, dtype=dtype, layout=layout, dw=dw, n=n, h=h, w=w, c=c, co=co, kh=kh, kw=kw, stride=tuple(stride),
                pad=tuple(pad), out_pad=tuple(out_pad), ho=ho, wo=wo, regime=regime, act=act, has_bias=has_bias,
                per_channel=per_channel, group=c if dw else 1, w_shape=w_shape,
                in_shape=(n, h, w, c) if nhwc else (n, c, h, w), out_shape=(n, ho, wo, co) if nhwc else (n, co, ho, wo))
    kq = co if per_channel else 1
    if dtype == "int8":
        case["x"] = rng.integers(-128, 128, case["in_shape"], dtype=np.int8)
        case["kernel"] = rng.integers(-100, 101, w_shape, dtype=np.int8)
        case["bias"] = rng.integers(-10000, 10001, (co,), dtype=np.int32)
        if regime == "exact":
            s_in = 2.0 ** -4
            k_scale = np.array([2.0 ** -(7 + (i % 3 if per_channel else 0)) for i in range(kq)], dtype=np.float32)
        else:
            s_in = float(np.float32(0.0431 + 0.01 * rng.random()))
            k_scale = (0.0071 + 0.004 * rng.random(kq)).astype(np.float32)
        terms = -(-kh // stride[0]) * -(-kw // stride[1]) * (1 if dw else c)  # at most, per output element
        sigma = np.sqrt(max(terms, 1)) * 74.0 * 58.0 * s_in * float(k_scale.mean())
        b_scale = (np.float32(s_in) * k_scale).astype(np.float32)
        sigma = max(sigma, 10000 * float(b_scale.mean()) / 2)
        target = 3.0 * sigma / 127.0
        out_scale = float(2.0 ** np.ceil(np.log2(target))) if regime == "exact" else float(np.float32(target))
        case.update(in_q=(s_in, in_zp), out_q=(out_scale, 7), k_scale=k_scale, b_scale=b_scale)
    else:
        def vals(shape, sd):
            if normal:
                return (sd * rng.standard_normal(shape)).astype(np.float16)
            return (rng.integers(-32, 33, shape) / 16.0).astype(np.float16)  # multiples of 2^-4 in [-2, 2]: every fp32 sum is exact
        case["x"], case["kernel"], case["bias"] = vals(case["in_shape"], 1.0), vals(w_shape, 0.1), vals((co,), 1.0)
        case.update(in_q=(1.0, 0), out_q=(1.0, 0), k_scale=np.ones(1, np.float32), b_scale=np.ones(1, np.float32))
    return case


# the shapes of the issue's table: name -> keyword arguments of make()
SHAPES = {
    "a_unet_2x2s2": dict(n=2, h=5, w=7, c=32, co=32, k=(2, 2), stride=(2, 2)),                       # 70 phase pixels
    "b_4x4s2p1": dict(h=6, w=5, c=64, co=24, k=(4, 4), stride=(2, 2), pad=(1, 1, 1, 1)),                 # ragged channel tile
    "c_3x3s2p1_outpad": dict(h=4, w=4, c=32, co=40, k=(3, 3), stride=(2, 2), pad=(1, 1, 1, 1), out_pad=(1, 1)),
    "d_3x3s1p1": dict(h=5, w=5, c=32, co=32, k=(3, 3), stride=(1, 1), pad=(1, 1, 1, 1)),                 # one phase, nine taps
    "e_1x1s2_empty_phases": dict(h=3, w=3, c=32, co=32, k=(1, 1), stride=(2, 2), out_pad=(1, 1)),        # bias-only outputs
    "f_2x3_s21_p01": dict(h=4, w=6, c=32, co=36, k=(2, 3), stride=(2, 1), pad=(0, 1, 0, 1)),
    "g_4x4s2p1_deep": dict(h=3, w=3, c=96, co=70, k=(4, 4), stride=(2, 2), pad=(1, 1, 1, 1)),            # Co % 4 != 0
    "h_2x2_s32": dict(h=3, w=4, c=32, co=32, k=(2, 2), stride=(3, 2)),                                   # stride > kernel in y
}
GATHER_ONLY = {
    "i_c3_co5": dict(h=5, w=4, c=3, co=5, k=(4, 4), stride=(2, 2), pad=(1, 1, 1, 1)),
    "i_c20_co32": dict(h=4, w=5, c=20, co=32, k=(4, 4), stride=(2, 2), pad=(1, 1, 1, 1)),
}
DEPTHWISE = {
    "j_dw19_4x4": dict(dw=True, h=5, w=4, c=19, k=(4, 4), stride=(2, 2), pad=(1, 1, 1, 1)),
    "j_dw64_3x3_outpad": dict(dw=True, n=2, h=4, w=3, c=64, k=(3, 3), stride=(2, 2), pad=(1, 1, 1, 1), out_pad=(1, 1)),
}
IN_ZPS = (-128, 127, -5)


def deconv_cases():
    out = []

    def add(name, **kw):
        out.append(make(name, **kw))
    z = 0
    for dtype in ("int8", "f16"):
        for regime in (("exact", "general") if dtype == "int8" else ("exact",)):
            tag = "%s_%s" % (dtype, regime)
            for stem, kw in SHAPES.items():
                add("%s_%s_nhwc" % (stem, tag), dtype=dtype, regime=regime, in_zp=IN_ZPS[z % 3], **kw)
                z += 1
            for stem, kw in GATHER_ONLY.items():
                add("%s_%s_nhwc" % (stem, tag), dtype=dtype, regime=regime, in_zp=IN_ZPS[z % 3], **kw)
                z += 1
            for stem, kw in DEPTHWISE.items():
                for layout in ("NHWC", "NCHW"):
                    add("%s_%s_%s" % (stem, tag, layout.lower()), dtype=dtype, regime=regime, layout=layout, in_zp=IN_ZPS[z % 3], **kw)
                    z += 1
            for stem in ("a_unet_2x2s2", "c_3x3s2p1_outpad"):  # k: NCHW group 1
                add("k_%s_%s_nchw" % (stem, tag), dtype=dtype, regime=regime, layout="NCHW", in_zp=IN_ZPS[z % 3], **SHAPES[stem])
                z += 1
            add("k_i_c3_co5_%s_nchw" % tag, dtype=dtype, regime=regime, layout="NCHW", **GATHER_ONLY["i_c3_co5"])
            # l: folded activations, no bias tensor, per-channel kernel records where they are allowed
            add("l_a_relu_%s_nhwc" % tag, dtype=dtype, regime=regime, act=1, in_zp=127, **SHAPES["a_unet_2x2s2"])
            add("l_b_relu6_nobias_%s_nhwc" % tag, dtype=dtype, regime=regime, act=2, has_bias=False, **SHAPES["b_4x4s2p1"])
            add("l_j_relu_%s_nchw" % tag, dtype=dtype, regime=regime, act=1, layout="NCHW", **DEPTHWISE["j_dw19_4x4"])
            if dtype == "int8":
                add("l_a_perchannel_%s_nhwc" % tag, dtype=dtype, regime=regime, per_channel=True, **SHAPES["a_unet_2x2s2"])
                add("l_b_perchannel_relu_%s_nhwc" % tag, dtype=dtype, regime=regime, per_channel=True, act=1, in_zp=-128, **SHAPES["b_4x4s2p1"])
                add("l_j_perchannel_%s_nhwc" % tag, dtype=dtype, regime=regime, per_channel=True, **DEPTHWISE["j_dw64_3x3_outpad"])
                add("l_j_perchannel_nobias_%s_nchw" % tag, dtype=dtype, regime=regime, per_channel=True, has_bias=False, layout="NCHW",
                    **DEPTHWISE["j_dw19_4x4"])
    # binary16 with normally distributed values: the fp32 sums depend on the order, gated at the project's 1e-3 relative
    add("g_4x4s2p1_deep_f16_normal_nhwc", dtype="f16", normal=True, **SHAPES["g_4x4s2p1_deep"])
    return out


def phase_eligible(case):
    es = 1 if case["dtype"] == "int8" else 2
    return case["layout"] == "NHWC" and not case["dw"] and (case["c"] * es) % 32 == 0


def forms_of(case):
    return (PHASE, GATHER) if phase_eligible(case) else (GATHER,)


# ------------------------------------------------------------------------------------ numpy restatement
def _canonical(case):
    """input as [n, h, w, c]; weights as [kh, kw, ci, co] (group 1) or [kh, kw, c] (depthwise)"""
    nhwc = case["layout"] == "NHWC"
    x = case["x"] if nhwc else case["x"].transpose(0, 2, 3, 1)
    k = case["kernel"]
    if case["dw"]:
        wk = k[0] if nhwc else k[:, 0].transpose(1, 2, 0)
    else:
        wk = k.transpose(1, 2, 3, 0) if nhwc else k.transpose(2, 3, 0, 1)
    return np.ascontiguousarray(x), np.ascontiguousarray(wk)


def tables(case):
    """mult[oc] = fl(s_in s_k[oc]) and bias_f[oc] = fl((float)b s_b[oc]) as source/mi355x_opt builds them"""
    co = case["co"]
    if case["dtype"] == "int8":
        ks = np.broadcast_to(case["k_scale"], (co,)) if case["k_scale"].size == 1 else case["k_scale"]
        bs = np.broadcast_to(case["b_scale"], (co,)) if case["b_scale"].size == 1 else case["b_scale"]
        mult = (np.float32(case["in_q"][0]) * ks.astype(np.float32)).astype(np.float32)
        bias = (case["bias"].astype(np.float32) * bs.astype(np.float32)).astype(np.float32) if case["has_bias"] else np.zeros(co, np.float32)
    else:
        mult = np.ones(co, np.float32)
        bias = case["bias"].astype(np.float32) if case["has_bias"] else np.zeros(co, np.float32)
    return np.ascontiguousarray(mult), np.ascontiguousarray(bias)


def epilogue(acc, case):
    """acc: [n, ho, wo, co] exact integer sums (int8) or fp32 sums (binary16) -> the output tensor in the case's layout"""
    mult, bias = tables(case)
    s, zp = np.float32(case["out_q"][0]), np.float32(case["out_q"][1])
    with np.errstate(all="ignore"):
        if case["dtype"] == "int8":
            f = ((acc.astype(np.float32) * mult).astype(np.float32) + bias).astype(np.float32)
            q = np.clip(np.rint((f / s).astype(np.float32)) + zp, -128, 127)
            if case["act"]:
                v = ((q - zp) * s).astype(np.float32)
                v = np.maximum(v, np.float32(0))
                if case["act"] == 2:
                    v = np.minimum(v, np.float32(6))
                q = np.clip(np.rint((v / s).astype(np.float32)) + zp, -128, 127)
            out = q.astype(np.int8)
        else:
            f = (acc.astype(np.float32) + bias).astype(np.float32)
            if case["act"]:
                f = np.where(f > 0, f, np.float32(0))
                if case["act"] == 2:
                    f = np.minimum(f, np.float32(6))
            out = pool_cases.f32_to_f16_ref(f).view(np.float16)
    return np.ascontiguousarray(out if case["layout"] == "NHWC" else out.transpose(0, 3, 1, 2))


def scatter_sums(case):
    """the reference's scatter, in its order: (iy, ix, ic) outermost, then (ky, kx, oc)"""
    x, wk = _canonical(case)
    n, h, w, c = x.shape
    kh, kw, (sh, sw), (pt, pl) = case["kh"], case["kw"], case["stride"], case["pad"][:2]
    ho, wo, co, int8 = case["ho"], case["wo"], case["co"], case["dtype"] == "int8"
    if int8:
        xv, wv = x.astype(np.int64) - case["in_q"][1], wk.astype(np.int64)
        acc = np.zeros((n, ho, wo, co), np.int64)
    else:
        xv, wv = x.astype(np.float32), wk.astype(np.float32)
        acc = np.zeros((n, ho, wo, co), np.float32)
    for iy in range(h):
        oy0 = iy * sh - pt
        ky0, ky1 = max(0, -oy0), min(kh, ho - oy0)
        for ix in range(w):
            ox0 = ix * sw - pl
            kx0, kx1 = max(0, -ox0), min(kw, wo - ox0)
            if ky0 >= ky1 or kx0 >= kx1:
                continue
            dst = acc[:, oy0 + ky0:oy0 + ky1, ox0 + kx0:ox0 + kx1, :]
            if case["dw"]:
                dst += xv[:, iy, ix, None, None, :] * wv[None, ky0:ky1, kx0:kx1, :]
            elif int8:
                dst += np.einsum("nc,yxco->nyxo", xv[:, iy, ix, :], wv[ky0:ky1, kx0:kx1])
            else:
                for ic in range(c):  # one rounding per product (exact) and per addition, in the reference's order
                    dst += xv[:, iy, ix, ic, None, None, None] * wv[None, ky0:ky1, kx0:kx1, ic, :]
    return acc


def deconv_scatter(case):
    return epilogue(scatter_sums(case), case)


def _first(pad, s, p):
    return (p - pad) % s


def _count(o, s, o0):
    return (o - o0 + s - 1) // s if o0 < o else 0


def _taps(k, s, p):
    return (k - p + s - 1) // s if p < k else 0


def phase_table(case, batch=None):
    """[(py, px, taps y, taps x, rows, cols)] + the tiles of 32 pixels x 32 channels and the workgroups of the phase form"""
    (sh, sw), (pt, pl) = case["stride"], case["pad"][:2]
    rows, total, most = [], 0, 0
    ctiles = (case["co"] + 31) // 32
    n = case["n"] if batch is None else batch
    for py in range(sh):
        for px in range(sw):
            r, c = _count(case["ho"], sh, _first(pt, sh, py)), _count(case["wo"], sw, _first(pl, sw, px))
            rows.append((py, px, _taps(case["kh"], sh, py), _taps(case["kw"], sw, px), r, c))
            t = ((n * r * c + 31) // 32) * ctiles
            total, most = total + t, max(most, t)
    return rows, total, ((most + 3) // 4) * sh * sw


def phase_sums(case):
    """per phase an ordinary convolution: tap j reads iy = qy - j, positions outside the image read the pad value, the
    int8 accumulator starts at acc_init[phase][oc] = -zp_in sum over the phase's taps and ic of w.  Group 1 only."""
    x, wk = _canonical(case)
    n, h, w, c = x.shape
    (sh, sw), (pt, pl) = case["stride"], case["pad"][:2]
    ho, wo, co, int8 = case["ho"], case["wo"], case["co"], case["dtype"] == "int8"
    zp = case["in_q"][1] if int8 else 0
    acc = np.zeros((n, ho, wo, co), np.int64 if int8 else np.float32)
    rows, _, _ = phase_table(case)
    for py, px, ty, tx, nr, nc in rows:
        if nr == 0 or nc == 0:
            continue
        oy0, ox0 = _first(pt, sh, py), _first(pl, sw, px)
        qy = (oy0 + pt) // sh + np.arange(nr)
        qx = (ox0 + pl) // sw + np.arange(nc)
        if int8:
            part = np.zeros((n, nr, nc, co), np.int64)
            part += -zp * sum((wk[py + j * sh, px + i * sw].astype(np.int64).sum(axis=0) for j in range(ty) for i in range(tx)),
                              np.zeros(co, np.int64))
        else:
            part = np.zeros((n, nr, nc, co), np.float32)
        for j in range(ty):
            iy = qy - j
            for i in range(tx):
                ix = qx - i
                ok = ((iy >= 0) & (iy < h))[:, None] & ((ix >= 0) & (ix < w))[None, :]
                g = x[:, np.clip(iy, 0, h - 1)[:, None], np.clip(ix, 0, w - 1)[None, :], :]
                g = np.where(ok[None, :, :, None], g, np.array(zp, dtype=x.dtype))  # the pad page
                wt = wk[py + j * sh, px + i * sw]  # [ci, co]
                if int8:
                    part += np.einsum("nyxc,co->nyxo", g.astype(np.int64), wt.astype(np.int64))
                else:
                    gf, wf = g.astype(np.float32), wt.astype(np.float32)
                    for ic in range(c):
                        part += gf[..., ic, None] * wf[ic]
        acc[:, oy0::sh, ox0::sw, :] = part
    return acc


def deconv_phase(case):
    return epilogue(phase_sums(case), case)


def matches(got, want, dtype):
    """tests/test_resize_session.py's gate: int8 equal, binary16 within 1e-3 relative"""
    if dtype == "int8":
        return np.array_equal(got, want)
    g, w = got.astype(np.float32), want.astype(np.float32)
    return bool(np.all(np.abs(g - w) <= 1e-3 * np.maximum(np.abs(w), 1e-3)))


bits = pool_cases.bits
assert_same = pool_cases.assert_same


def golden():
    blob = np.load(os.path.join(HERE, "golden", "deconv_cases.npz"))
    return {k: blob[k] for k in blob.files}


# ------------------------------------------------------------------------------------ the routes
def deconv_desc(case, **override):
    d = pkg.ConvDesc()
    d.layout = pkg.SHL_NHWC if case["layout"] == "NHWC" else pkg.SHL_NCHW
    d.dtype = pkg.SHL_I8 if case["dtype"] == "int8" else pkg.SHL_F16
    d.act, d.batch = case["act"], case["n"]
    d.in_h, d.in_w, d.in_c, d.out_h, d.out_w, d.out_c = case["h"], case["w"], case["c"], case["ho"], case["wo"], case["co"]
    d.kernel_h, d.kernel_w = case["kh"], case["kw"]
    d.stride_h, d.stride_w = case["stride"]
    d.pad_top, d.pad_left = case["pad"][:2]
    d.dilation_h = d.dilation_w = 1
    d.group = case["group"]
    d.in_zp, d.out_zp, d.out_scale = case["in_q"][1], case["out_q"][1], case["out_q"][0]
    for key, v in override.items():
        setattr(d, key, v)
    return d


GUARD = 256  # bytes in front of and behind the output buffer, a multiple of 16


def cabi_run(hip, dev, case, batch=None):
    """plan + forward through the C ABI on device buffers with guard bands around the output.  Returns (output, kernel
    name, algo); batch: forward only that many images of the plan"""
    mult, bias = tables(case)
    plan = C.c_void_p()
    desc = deconv_desc(case)
    k = np.ascontiguousarray(case["kernel"])
    pkg.check(hip.shl_mi355x_deconv_plan_create(C.byref(desc), k.ctypes.data, mult.ctypes.data if case["dtype"] == "int8" else None,
                                                bias.ctypes.data if case["has_bias"] else None, None, C.byref(plan)), hip, "deconv_plan_create")
    try:
        name, algo = hip.shl_mi355x_conv_plan_kernel_name(plan).decode(), hip.shl_mi355x_conv_plan_algo(plan)
        n = case["n"] if batch is None else batch
        x = np.ascontiguousarray(case["x"][:n])
        out_shape = (n,) + tuple(case["out_shape"][1:])
        out_dt = np.int8 if case["dtype"] == "int8" else np.float16
        nbytes = int(np.prod(out_shape)) * np.dtype(out_dt).itemsize
        d_in, d_out = dev.alloc(x.nbytes), dev.alloc(nbytes + 2 * GUARD)
        dev.upload(d_in, x)
        dev.upload(d_out, np.full(nbytes + 2 * GUARD, 0xA5, np.uint8))
        pkg.check(hip.shl_mi355x_conv_forward(plan, d_in, d_out + GUARD, batch if batch is not None else 0, None), hip, "conv_forward")
        raw = dev.download(d_out, (nbytes + 2 * GUARD,), np.uint8)
        dev.free(d_in)
        dev.free(d_out)
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + nbytes:] == 0xA5).all(), "%s: the guard bands were written" % case["name"]
        return raw[GUARD:GUARD + nbytes].view(out_dt).reshape(out_shape).copy(), name, algo
    finally:
        hip.shl_mi355x_conv_plan_destroy(plan)


def csinn_tensors(fe, keep, sess, case, device=None, override=None):
    """(input, output, kernel, bias) tensors of a case, the device pointers of input / output, the host output array"""
    o = override or {}
    int8 = case["dtype"] == "int8"
    dt = o.get("dtype", pkg.DTYPE_INT8 if int8 else pkg.DTYPE_FLOAT16)
    nhwc = case["layout"] == "NHWC"
    act_l = pkg.LAYOUT_NHWC if nhwc else pkg.LAYOUT_NCHW
    if case["dw"]:
        w_l = pkg.LAYOUT_1HWO if nhwc else pkg.LAYOUT_O1HW
    else:
        w_l = pkg.LAYOUT_OHWI if nhwc else pkg.LAYOUT_IOHW
    out = np.zeros(case["out_shape"], dtype=np.int8 if int8 else np.float16)
    d_in = d_out = None
    if device is not None:
        d_in, d_out = device.alloc(case["x"].nbytes), device.alloc(out.nbytes)
        device.upload(d_in, case["x"])
    t_in = pkg.make_tensor(fe, keep, case["in_shape"], dt, act_l, data=case["x"], scales=o.get("in_scales", (case["in_q"][0],)),
                           zps=(case["in_q"][1],), name=b"input", sess=sess, device_ptr=d_in)
    t_out = pkg.make_tensor(fe, keep, case["out_shape"], o.get("out_dtype", dt), act_l, data=out, scales=(case["out_q"][0],),
                            zps=(case["out_q"][1],), name=b"output", sess=sess, device_ptr=d_out)
    kz = o.get("k_zps", (0,))
    t_w = pkg.make_tensor(fe, keep, case["w_shape"], dt, w_l, data=case["kernel"], scales=o.get("k_scales", tuple(case["k_scale"])),
                          zps=kz, is_const=1, name=b"kernel", sess=sess, **({"mtype": pkg.MEM_DMABUF} if o.get("kernel_dmabuf") else {}))
    if case["has_bias"]:
        t_b = pkg.make_tensor(fe, keep, (case["co"],), pkg.DTYPE_INT32 if int8 else dt, pkg.LAYOUT_O, data=case["bias"],
                              scales=o.get("b_scales", tuple(case["b_scale"])), zps=(0,), is_const=1, name=b"bias", sess=sess)
    else:
        t_b = pkg.make_tensor(fe, keep, (), pkg.DTYPE_INT32 if int8 else dt, pkg.LAYOUT_O, name=b"bias", sess=sess)
    return (t_in, t_out, t_w, t_b), (d_in, d_out), out


def csinn_run(fe, api, case, device=None, keep_params=None, status=False, **override):
    """layer mode through csinn_deconv2d (+ _init).  status: return (init status, exec status) instead of raising.  A case
    with a folded activation runs csinn_relu / csinn_relu6 behind the deconvolution (same record: what the fold computes)"""
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, api, keep)
    nhwc = case["layout"] == "NHWC"
    act_l = pkg.LAYOUT_NHWC if nhwc else pkg.LAYOUT_NCHW
    tensors, (d_in, d_out), out = csinn_tensors(fe, keep, sess, case, device, override)
    params = pkg.deconv_params(fe, keep, api, act_l, case["stride"], case["pad"], case["out_pad"], override.get("group", case["group"]),
                               override.get("dilation", (1, 1)), sess)
    rc_init = fe.csinn_deconv2d_init(*tensors, params)
    rc = fe.csinn_deconv2d(*tensors, params) if rc_init == pkg.CSINN_TRUE else rc_init
    if rc == pkg.CSINN_TRUE and case["act"] and not status:
        kind = "relu" if case["act"] == 1 else "relu6"
        rp = pkg.siso_params(fe, keep, api, kind, act_l, 1, sess)
        assert getattr(fe, "csinn_%s_init" % kind)(tensors[1], tensors[1], rp) == pkg.CSINN_TRUE
        rc = getattr(fe, "csinn_" + kind)(tensors[1], tensors[1], rp)
    if device is not None:
        out = device.download(d_out, out.shape, out.dtype)
        device.free(d_in)
        device.free(d_out)
    if keep_params is not None:
        keep_params.append((params, keep))
    if status:
        return rc_init, rc
    if rc != pkg.CSINN_TRUE:
        raise pkg.MI355XError("csinn_deconv2d returned %d" % rc)
    return out


def reference_run(fe, case):
    """the genuine library's answer (CSINN_REF, layer mode)"""
    return csinn_run(fe, pkg.API_REF, case)


# ------------------------------------------------------------------------------------ a small decoder
class DecoderNet:
    """data (16 ch, 8 x 8) -> conv 3x3 + relu (E1, 32 ch) -> maxpool 2x2 (4 x 4) -> conv 3x3 + relu (32 ch) -> deconv 2x2 s2
    (32 ch, 8 x 8) -> relu (its own layer, same record: folds) -> concat with E1 (64 ch) -> conv 3x3 (32 ch) -> deconv 4x4 s2
    p1 (16 ch, 16 x 16) -> sigmoid; int8 NHWC or fp16 NCHW through the csinn session API in graph mode: one level of a U-Net."""

    def __init__(self, dtype="int8", layout="NHWC", seed=85):
        self.dtype, self.layout = dtype, layout
        int8 = dtype == "int8"
        rng = np.random.default_rng(seed)
        q1 = lambda s, z: (float(s), int(z)) if int8 else (1.0, 0)
        self.q_in = q1(2.0 ** -4, -5)
        q = self.q = dict(e1=q1(2.0 ** -3, -100), p1=q1(2.0 ** -3, -100), e2=q1(2.0 ** -2, -90), up=q1(2.0 ** -1, -80), cat=q1(2.0 ** -1, -60),
                          d1=q1(2.0 ** -1, 3), up2=q1(2.0 ** -3, 5))
        self.q_out = q1(1.0 / 256, -128)

        def conv(cin, cout, hin, q_prev, out_q, act, k_log2=-7):
            case = cases.make_case(int(rng.integers(1 << 30)), layout=layout, dtype=dtype, n=1, h=hin, w=hin, c=cin, co=cout, k=(3, 3),
                                   stride=(1, 1), pad=(1, 1, 1, 1), act=act)
            if int8:
                case["in_scale"], case["in_zp"] = q_prev
                case["k_scale"] = np.array([2.0 ** k_log2], dtype=np.float32)
                case["b_scale"] = (np.float32(case["in_scale"]) * case["k_scale"]).astype(np.float32)
                case["bias"] = rng.integers(-2000, 2001, (case["co"],), dtype=np.int32)
                case["out_scale"], case["out_zp"] = out_q
            return case

        def deconv(name, cin, cout, hin, k, pad, q_prev, out_q, act, w_sd=0.1, b_sd=1.0):
            case = make("decoder_%s_%s_%s" % (name, dtype, layout), dtype=dtype, layout=layout, n=1, h=hin, w=hin, c=cin, co=cout, k=(k, k),
                        stride=(2, 2), pad=(pad,) * 4, act=act)
            if int8:
                case["in_q"], case["out_q"] = q_prev, out_q
                case["k_scale"] = np.array([2.0 ** -7], dtype=np.float32)
                case["b_scale"] = (np.float32(q_prev[0]) * case["k_scale"]).astype(np.float32)
                case["kernel"] = rng.integers(-32, 32, case["w_shape"], dtype=np.int8)
                case["bias"] = rng.integers(-2000, 2001, (cout,), dtype=np.int32)
            else:
                # (small enough that the last layer's sums stay within +-2: the sigmoid behind it turns an ABSOLUTE error of
                # its input into a RELATIVE one of its output, which the 1e-3 gate of the binary16 chain could not hold at |x| = 10)
                case["kernel"] = (w_sd * rng.standard_normal(case["w_shape"])).astype(np.float16)
                case["bias"] = (b_sd * rng.standard_normal((cout,))).astype(np.float16)
            return case
        self.cv = dict(e1=conv(16, 32, 8, self.q_in, q["e1"], 1), e2=conv(32, 32, 4, q["p1"], q["e2"], 1),
                       d1=conv(64, 32, 8, q["cat"], q["d1"], 0, k_log2=-8))
        self.dc = dict(up=deconv("up", 32, 32, 4, 2, 0, q["e2"], q["up"], 1), up2=deconv("up2", 32, 16, 8, 4, 1, q["d1"], q["up2"], 0, w_sd=0.004, b_sd=0.25))

    def _shape(self, c, h):
        return (1, h, h, c) if self.layout == "NHWC" else (1, c, h, h)

    @property
    def c_axis(self):
        return 3 if self.layout == "NHWC" else 1

    def input(self, k):
        rng = np.random.default_rng(300 + k)
        shape = self._shape(16, 8)
        return rng.integers(-100, 100, shape, dtype=np.int8) if self.dtype == "int8" else rng.standard_normal(shape).astype(np.float16)

    # -- oracle chain: convolutions through the C oracle, everything else through the numpy restatements
    def oracle(self, x):
        form = "ref" if self.dtype == "int8" else "f16"
        q, cv, dc = self.q, self.cv, self.dc

        def run_conv(name, cur):
            case = dict(cv[name])
            case["input"] = np.ascontiguousarray(cur)
            return cases.oracle_run(case, form)

        def run_deconv(name, cur):
            return deconv_scatter(dict(dc[name], x=np.ascontiguousarray(cur)))
        e1 = run_conv("e1", x)
        p1 = pool_cases.pool_numpy(dict(kind="max", dtype=self.dtype, layout=self.layout, x=e1, kernel=(2, 2), stride=(2, 2), pad=(0, 0, 0, 0),
                                        cip=0, ho=4, wo=4, in_q=q["e1"], out_q=q["p1"]))
        up = run_deconv("up", run_conv("e2", p1))  # (the relu layer behind it: the case's act)
        cat = concat_cases.concat_numpy(dict(axis=self.c_axis, dtype=self.dtype, xs=[up, e1], in_qs=[q["up"], q["e1"]], out_q=q["cat"],
                                             out_shape=self._shape(64, 8)))
        up2 = run_deconv("up2", run_conv("d1", cat))
        return eltwise_cases.eltwise_numpy(dict(op="sigmoid", dtype=self.dtype, x=up2, in_q=q["up2"], out_q=self.q_out, n=0.0))

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
        q, cv, dc = self.q, self.cv, self.dc

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

        def deconv(name, t_in, c_out, h, rec):
            case = dc[name]
            bname = name.encode()
            t_w = T(case["w_shape"], None, bname + b"_w", case["kernel"], 1, pkg.LAYOUT_OHWI if nhwc else pkg.LAYOUT_IOHW,
                    scales=tuple(case["k_scale"]))
            t_b = T((case["co"],), None, bname + b"_b", case["bias"], 1, pkg.LAYOUT_O, pkg.DTYPE_INT32 if int8 else dt,
                    scales=tuple(case["b_scale"]))
            p = pkg.deconv_params(fe, keep, api, act_l, case["stride"], case["pad"], (0, 0), 1, (1, 1), sess, bname)
            t_out = T(self._shape(c_out, h), rec, bname + b"_out")
            ops.append(("csinn_deconv2d", (t_in, t_out, t_w, t_b, p)))
            return t_out

        def siso(stem, kind, name, t_in, shape, rec, params=None):
            t_out = T(shape, rec, name + b"_out")
            ops.append((stem, (t_in, t_out, params if params is not None else pkg.siso_params(fe, keep, api, kind, act_l, self.c_axis, sess, name))))
            return t_out
        t_in = T(self._shape(16, 8), self.q_in, b"data")
        e1 = conv("e1", t_in, 32, 8, q["e1"], stem="csinn_conv2d_relu")
        p1 = siso("csinn_maxpool2d", None, b"pool", e1, self._shape(32, 4), q["p1"],
                  pkg.pool_params(fe, keep, api, act_l, (2, 2), (2, 2), (0, 0, 0, 0), 0, False, sess, b"pool"))
        e2 = conv("e2", p1, 32, 4, q["e2"], stem="csinn_conv2d_relu")
        up_raw = deconv("up", e2, 32, 8, q["up"])
        up = siso("csinn_relu", "relu", b"up_relu", up_raw, self._shape(32, 8), q["up"])
        t_cat = T(self._shape(64, 8), q["cat"], b"cat_out")
        ops.append(("csinn_concat", (pkg.tensor_array(keep, [up, e1]), t_cat, pkg.concat_params(fe, keep, api, act_l, 2, self.c_axis, sess, b"cat"))))
        d1 = conv("d1", t_cat, 32, 8, q["d1"])
        up2 = deconv("up2", d1, 16, 16, q["up2"])
        prob = siso("csinn_sigmoid", "sigmoid", b"sigmoid", up2, self._shape(16, 16), self.q_out)
        for stem, args in ops:
            assert getattr(fe, stem + "_init")(*args) == pkg.CSINN_TRUE, stem
        fe.csinn_set_tensor_entry(t_in, sess)
        fe.csinn_set_input(0, t_in, sess)
        for stem, args in ops:
            assert getattr(fe, stem)(*args) == pkg.CSINN_TRUE, stem
        fe.csinn_set_output(0, prob, sess)
        rc = fe.csinn_session_setup(sess)
        assert rc == pkg.CSINN_TRUE or getattr(fe, "kind", "") == "reference"
        self._keep, self._sess, self._out_shape, self._in_q = keep, sess, self._shape(16, 16), self.q_in
        self.layer_count = len(ops)
        return sess

    run = tail.MiniNet.run
    close = tail.MiniNet.close

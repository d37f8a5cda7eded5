"""Shared helpers for the fused attention core with an additive bias or mask on the scores (shl_mi355x_attention_bias):
scores = Q K^T, [scores * a one-element constant], + bias, softmax over the keys, P V as one launch.

  all_cases()    deterministic problems, seeded by crc32(name) through attention_cases._add, all on 2 x 3 batches (both batch
                 indices of the bias move): query rows 1, 31, 32, 33, 65 (one ragged tile, a full one, a second one) crossed
                 with keys 1, 63, 64, 65, 129, 257 (int8: the per-row table), 1024 (the cap) and the bias shapes GEOMETRIES;
                 d = 64, so Q K^T is matmul's mfma form, and where t < 64 a dv wide enough that 6 s dv > 65536 gives P V the
                 mfma form as well; with and without the multiply, the bias as the add's first and second input, the bias
                 pointer one element off the 16-byte grid.  int8: a mask record under which -128 saturates the sum, and a
                 bias record on the far side of add_step.h's div_by_scale condition (a scale of 2^54: the sum's bound exceeds
                 2^60, so the hardware's division is taken).  binary16: -inf columns, a fully -inf row, +inf, -0, and NaNs
                 against the NaN scores of attention_cases' special row, in both operand orders
  index_map      where [batches][s][t] finds its bias element, by numpy's broadcast_to
  add_desc       the add's own descriptor (struct shl_mi355x_mul_desc): a the scores, b the bias
  bias_desc      struct shl_mi355x_attention_bias_desc through shl_mi355x_attention_bias_geometry
  run_both       (-m gpu) the fused launch and the four or five unfused calls on the same device buffers
"""
import ctypes as C

import numpy as np

import attention_cases as ac
import eltwise_cases
from cases import pkg
from pool_cases import _q

B0, B1 = 2, 3  # the scores are [2, 3, s, t]
GEOMETRIES = {"h_s_t": lambda s, t: (1, B1, s, t), "b_t": lambda s, t: (B0, 1, 1, t), "b_s_t": lambda s, t: (B0, 1, s, t),
              "s_t4": lambda s, t: (1, 1, s, t), "s_t": lambda s, t: (s, t), "t": lambda s, t: (t,), "h_t": lambda s, t: (1, B1, 1, t),
              "one": lambda s, t: (1, 1, 1, 1), "same": lambda s, t: (B0, B1, s, t)}
NEG_INF, POS_INF, NEG_ZERO = 0xFC00, 0x7C00, 0x8000
FAR_SCALE = 2.0 ** 54  # a bias record whose sums leave div_by_scale's proven range


def fma_div(c):
    """add_step.h:add_rec restated: is the sum's bound inside the range in which one fused multiply-add is the division"""
    (sa, za), (sb, zb), (so, _) = x_record(c), c["b_q"], c["sb_q"]
    bound = (128.0 + abs(za)) * abs(sa) + (128.0 + abs(zb)) * abs(sb)
    return 2.0 ** -40 <= so <= 2.0 ** 40 and bound <= 2.0 ** 60


def x_record(c):
    """the record of the add's full operand: the scaled scores', else the scores'"""
    return c["sc_q"] if c["has_scale"] else c["s_q"]


def _bias_add(out, name, dtype, geom, s, t, dv=64, bias_first=False, bias_off=False, kind="plain", **kw):
    """kind: plain; int8 mask (0 / -128 under a record that saturates the sum), far (a record beyond div_by_scale's range:
    elements at the zero point leave the score alone, the others saturate the sum); binary16 special"""
    cases = []
    ac._add(cases, "bias_" + name, dtype, s=s, t=t, d=64, dv=dv, batches=B0 * B1, special=kind == "special", **kw)
    c = cases[0]
    rng = ac._rng("attention bias " + c["name"])
    shape = GEOMETRIES[geom](s, t)
    c.update(geom=geom, bias_shape=shape, bias_first=bias_first, bias_off=bias_off, kind=kind)
    if dtype == "int8":
        xs, xz = x_record(c)
        conv = c["regime"] == "conv"
        if kind == "mask":  # masked keys: -128 under four times the scores' scale is -512 LSB of the sum
            c["bias"] = np.where(rng.random(shape) < 0.3, -128, 0).astype(np.int8)
            c["b_q"], c["sb_q"] = _q(xs * 4.0, 0), _q(xs, xz)
        elif kind == "far":
            c["bias"] = np.where(rng.random(shape) < 0.25, rng.integers(-128, 128, shape), 7).astype(np.int8)
            c["b_q"], c["sb_q"] = _q(FAR_SCALE, 7), _q(xs * 1.25, -3)
        else:  # the bias spreads over about as many LSB of the sum as the scores do
            c["bias"] = rng.integers(-128, 128, shape, dtype=np.int8)
            c["b_q"] = _q(xs * (0.43 if conv else 0.5), 3)
            c["sb_q"] = _q(xs * (1.31 if conv else 1.0), -5)
    else:
        c["bias"] = (rng.integers(-16, 17, shape) / 16.0).astype(np.float16)
        c["b_q"] = c["sb_q"] = _q(1.0, 0)
        if kind == "special":
            assert geom == "h_s_t" and s > 8 and t > 12
            u = c["bias"].view(np.uint16)
            u[0, :, :, 5] = NEG_INF               # a masked key in every row
            u[0, 1, :, 9] = NEG_INF               # ... and one in one head only
            u[0, 1, 4, :] = NEG_INF               # a row with nothing left
            u[0, 0, 2, 11] = POS_INF
            u[0, 2, 6, 0:4] = NEG_ZERO
            # against the NaN scores of attention_cases' special row (batch 0 of the attention: i0 = 0, i1 = 0), NaNs of
            # either sign and of other payloads, next to ordinary elements; and against its infinite scores an opposite infinity
            nan_row, inf_row = ac.SPECIAL_ROWS[1], ac.SPECIAL_ROWS[0]
            u[0, 0, nan_row, 0], u[0, 0, nan_row, 1], u[0, 0, nan_row, 2] = 0x7E01, 0xFE02, 0xFD55
            u[0, 0, inf_row, [0, 2, 4, 6]] = NEG_INF
            u[0, 0, inf_row, [1, 3, 7, 8]] = POS_INF
    out.append(c)


def _both(out, name, *args, **kw):
    for dtype in ("int8", "f16"):
        _bias_add(out, name, dtype, *args, **kw)


def all_cases():
    out = []
    #            name                geometry  s   t
    _both(out, "h_s_t_s33_t65", "h_s_t", 33, 65)
    _both(out, "b_t_s1_t64", "b_t", 1, 64, bias_first=True, regime="conv")
    _both(out, "b_s_t_s31_t129", "b_s_t", 31, 129, has_scale=False, bias_off=True)
    _both(out, "s_t4_s32_t257", "s_t4", 32, 257, bias_first=True, scale_first=True)
    _both(out, "s_t_s65_t63", "s_t", 65, 63, dv=176, has_scale=False, bias_first=True, regime="conv")
    _both(out, "h_s_t_s33_t1", "h_s_t", 33, 1, dv=336, bias_off=True)
    _both(out, "h_t_s32_cap", "h_t", 32, ac.CAP)
    _both(out, "one_s33_t65", "one", 33, 65, bias_off=True, regime="conv")
    _both(out, "same_s33_t64", "same", 33, 64, has_scale=False)
    _both(out, "same_first_s31_t65", "same", 31, 65, bias_first=True, bias_off=True)
    _both(out, "t_s65_t129", "t", 65, 129, bias_first=True, bias_off=True)
    _both(out, "b_t_s32_t257_no_mul", "b_t", 32, 257, has_scale=False, regime="conv")
    _bias_add(out, "mask_saturates", "int8", "b_t", 33, 65, kind="mask")
    _bias_add(out, "mask_saturates_s_t4", "int8", "s_t4", 65, 129, kind="mask", bias_first=True, regime="conv")
    _bias_add(out, "far_record", "int8", "h_s_t", 33, 65, kind="far")
    _bias_add(out, "far_record_no_mul", "int8", "b_s_t", 32, 257, kind="far", has_scale=False, bias_first=True, bias_off=True)
    _bias_add(out, "specials", "f16", "h_s_t", 33, 65, kind="special")
    _bias_add(out, "specials_first", "f16", "h_s_t", 33, 65, kind="special", bias_first=True, bias_off=True)
    _bias_add(out, "specials_no_mul", "f16", "h_s_t", 33, 65, kind="special", has_scale=False, bias_first=True)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def case_id(case):
    return case["name"]


def index_map(c):
    """[batches][s][t] -> the bias element's index, by numpy's own broadcasting"""
    idx = np.arange(int(np.prod(c["bias_shape"])), dtype=np.int64).reshape(c["bias_shape"])
    return np.broadcast_to(idx, (B0, B1, c["s"], c["t"])).reshape(B0 * B1, c["s"], c["t"])


def desc_index_map(bd, batches, s, t):
    """the same map by the descriptor's formula (include/shl_mi355x.h)"""
    bi = np.arange(batches, dtype=np.int64)
    i0, i1 = bi // bd.b_ext1, bi % bd.b_ext1
    s0 = bd.b_stride[0] if batches // bd.b_ext1 > 1 else 0
    s1 = bd.b_stride[1] if bd.b_ext1 > 1 else 0
    rs, ks = (bd.row_stride if s > 1 else 0), (bd.key_stride if t > 1 else 0)
    return (i0 * s0 + i1 * s1)[:, None, None] + (np.arange(s, dtype=np.int64) * rs)[None, :, None] + \
        (np.arange(t, dtype=np.int64) * ks)[None, None, :]


def add_desc(c):
    """the unfused add's descriptor: a the (scaled) scores [2, 3, s, t], b the bias"""
    return eltwise_cases.mul_desc(dict(dtype=c["dtype"], in_q=x_record(c), in1_q=c["b_q"], out_q=c["sb_q"], small_first=c["bias_first"]),
                                  (B0, B1, c["s"], c["t"]), c["bias_shape"])


def bias_desc(hip, c):
    bd = pkg.AttentionBiasDesc()
    md = add_desc(c)
    pkg.check(hip.shl_mi355x_attention_bias_geometry(C.byref(md), c["batches"], c["s"], c["t"], C.byref(bd)), hip,
              "shl_mi355x_attention_bias_geometry")
    bd.bias_is_first = int(c["bias_first"])
    (bd.b_scale, bd.b_zp), (bd.sb_scale, bd.sb_zp) = c["b_q"], c["sb_q"]
    return bd


POISON, GUARD, SLACK = ac.POISON, ac.GUARD, ac.SLACK


def run_both(hip, dev, c):
    """(the fused launch's output, the unfused calls' output, their sum -- the softmax's input --, their add's input, their
    probabilities), all from the device; the bytes around the fused output are poisoned and must stay.  bias_off moves the bias
    one element off the allocator's grid, for the fused launch and the unfused add alike"""
    b, s, t, dv = c["batches"], c["s"], c["t"], c["dv"]
    es = c["q"].itemsize
    dt = pkg.SHL_I8 if c["dtype"] == "int8" else pkg.SHL_F16
    room, bufs = [], {}

    def alloc(nbytes):
        room.append(dev.alloc(nbytes + SLACK))
        return room[-1]
    for key in ("q", "k", "v", "bias") + (("c",) if c["has_scale"] else ()):
        bufs[key] = alloc(c[key].nbytes) + (es if key == "bias" and c["bias_off"] else 0)
        dev.upload(bufs[key], c[key])
    for key in ("s", "x", "sum", "p"):
        bufs[key] = alloc(b * s * t * es)
    out_bytes = b * s * dv * es
    frame = np.full(out_bytes + 2 * GUARD, POISON, np.uint8)
    for key in ("chain", "fused"):
        bufs[key] = alloc(frame.nbytes)
        dev.upload(bufs[key], frame)
    p_chain, p_fused = bufs["chain"] + GUARD, bufs["fused"] + GUARD
    qk, mul, pv = ac.unfused_descs(c)
    assert hip.shl_mi355x_matmul_kernel_name(bufs["q"], bufs["k"], bufs["s"], C.byref(qk)).decode() == pkg.MATMUL_MFMA
    assert hip.shl_mi355x_matmul_kernel_name(bufs["p"], bufs["v"], p_chain, C.byref(pv)).decode() == pkg.MATMUL_MFMA
    pkg.check(hip.shl_mi355x_matmul(bufs["q"], bufs["k"], bufs["s"], C.byref(qk), None), hip, "shl_mi355x_matmul (q k^T)")
    x = bufs["s"]
    if c["has_scale"]:
        pkg.check(hip.shl_mi355x_mul(bufs["s"], bufs["c"], bufs["x"], C.byref(mul), None), hip, "shl_mi355x_mul")
        x = bufs["x"]
    md = add_desc(c)
    pkg.check(hip.shl_mi355x_add_bcast(x, bufs["bias"], bufs["sum"], C.byref(md), None), hip, "shl_mi355x_add_bcast")
    pkg.check(hip.shl_mi355x_softmax(bufs["sum"], bufs["p"], dt, b * s, t, 1, c["sb_q"][0], c["sb_q"][1], c["p_q"][0], c["p_q"][1], None),
              hip, "shl_mi355x_softmax")
    pkg.check(hip.shl_mi355x_matmul(bufs["p"], bufs["v"], p_chain, C.byref(pv), None), hip, "shl_mi355x_matmul (p v)")
    d, bd = ac.desc(c), bias_desc(hip, c)
    args = (bufs["q"], bufs["k"], bufs["v"], bufs["bias"], p_fused, C.byref(d), C.byref(bd))
    assert hip.shl_mi355x_attention_bias_kernel_name(*args).decode() == pkg.ATTENTION_BIAS_MFMA
    pkg.check(hip.shl_mi355x_attention_bias(*args, None), hip, "shl_mi355x_attention_bias")
    got = dev.download(bufs["fused"], frame.shape, np.uint8)
    assert np.all(got[:GUARD] == POISON) and np.all(got[GUARD + out_bytes:] == POISON), "wrote outside the output"
    view = lambda raw, shape: raw.view(c["q"].dtype)[:int(np.prod(shape))].reshape(shape)
    fused = view(got[GUARD:GUARD + out_bytes].copy(), (b, s, dv))
    chain = view(dev.download(bufs["chain"], frame.shape, np.uint8)[GUARD:GUARD + out_bytes].copy(), (b, s, dv))
    total = dev.download(bufs["sum"], (b, s, t), c["q"].dtype)
    x_in = dev.download(x, (b, s, t), c["q"].dtype)
    p = dev.download(bufs["p"], (b, s, t), c["q"].dtype)
    for ptr in room:
        dev.free(ptr)
    return fused, chain, total, x_in, p

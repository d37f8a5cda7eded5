"""Shared helpers for the attention core on operands where the projections left them (shl_mi355x_attention_layout): q, k and v
read out of [B, S, H D] tensors by strides, the output written into one, instead of a reshape and a transpose(0,2,1,3) in
front of each operand and behind the output.

  all_cases()   deterministic problems on attention_cases._add's data and records (a case's dense q, k, v are the operands the
                movers would produce; its SOURCES are those arrays permuted back on the host), the smallest shapes that reach
                each path:
                  c1      B=2 H=3 S=33 T=70 d=64 dv=72: both parts of the batch index, a ragged second row tile, a ragged key
                          pass; int8: dv is no multiple of 16 bytes, so v and the output go by elements, q and k by 16-byte loads
                  c2      B=16 H=4 S=T=49 d=dv=32 (Swin windows: k < 64 on more than 65536 outputs) with a bias [1,H,S,T]
                  c3      B=1 H=2 S=T=80 d=dv=64, the session net's shape: plain, and with a padding mask [B,1,1,T] with and
                          without the multiply
                  c4      d=dv=68: row strides off the 16-byte grid; the pattern without a reshape
                  c1_off  c1 with every operand 1, 2 and 4 elements into its allocation
                  packed  q, k and v inside one [B,S,3,H,D] projection
                  k0231   K's strides derived as ONNX exports it -- transpose(0,2,3,1) and the last two dims read the other way
                          round --; the reference's dense K is made by the ordinary transpose, so at the kernel this is the
                          derivation's test (the product without trans_b itself: tests/test_attention_layout_session.py)
                  rank3   [S,H,D] -> transpose(1,0,2)
                  gaps    an output whose rows are further apart than H dv: the gaps keep their poison
                  specials (binary16) +-inf, NaNs of both signs and other payloads, subnormals in q, k and v: moved set, against
                          the movers; moved clear, against the dense kernel on a host-permuted copy
  view          an operand's {outer, head, row} through shl_mi355x_attention_layout_strides, and numpy's own strides for it
  run_both      (-m gpu) the layout launch, and the reference: shl_mi355x_move / shl_mi355x_transpose, shl_mi355x_attention[_bias],
                shl_mi355x_transpose [/ shl_mi355x_move] back, on the same device buffers; whole frames with 64-byte guards
"""
import ctypes as C

import numpy as np

import attention_bias_cases as abc
import attention_cases as ac
from cases import pkg
from pool_cases import _q

POISON, GUARD = ac.POISON, ac.GUARD
MOVED_ALL = 15
MAX_DIM = 8
SPECIAL_BITS = (0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7D55, 0xFC01, 0x0001, 0x83FF, 0x8000)
SUBNORMAL_BITS = (0x0001, 0x83FF, 0x8000)  # (and -0)


def _case(out, name, dtype, B, H, s, t, d, dv, pattern="reshape", bias=None, offset=0, gap=0, moved=MOVED_ALL, special=False, **kw):
    cs = []
    ac._add(cs, "layout_" + name, dtype, s=s, t=t, d=d, dv=dv, batches=B * H, **kw)
    c = cs[0]
    c.update(B=B, H=H, pattern=pattern, bias_geom=bias, offset=offset, gap=gap, moved=moved, special_bits=special)
    rng = ac._rng("attention layout " + c["name"])
    if bias:
        shape = (1, H, s, t) if bias == "h_s_t" else (B, 1, 1, t)
        if dtype == "int8":
            xs, _ = abc.x_record(c)
            c["bias"] = rng.integers(-128, 128, shape, dtype=np.int8)
            c["b_q"], c["sb_q"] = _q(xs * 0.5, 3), _q(xs, -5)
        else:
            c["bias"] = (rng.integers(-16, 17, shape) / 16.0).astype(np.float16)
            if bias == "b_t":  # a padding mask: the last keys of every batch
                c["bias"][..., t - 7:] = -np.inf
            c["b_q"] = c["sb_q"] = _q(1.0, 0)
    if special:
        assert dtype == "f16"
        # A NaN or an infinity in q takes its query row, one in k every row of its batch, one in v a column of its batch: batch 0
        # holds only subnormals and -0 (ordinary outputs), batch 1 the specials of q, batch 2 those of k, batch 3 those of v
        for key, batch in (("q", 1), ("k", 2), ("v", 3)):
            u = c[key].view(np.uint16)
            for i, bits in enumerate(SPECIAL_BITS):
                u[batch, 3 + 2 * i, (5 + 7 * i) % u.shape[2]] = bits
                if bits in SUBNORMAL_BITS:
                    u[0, 2 + 3 * i, (1 + 5 * i) % u.shape[2]] = bits
    out.append(c)


def all_cases():
    out = []
    for dtype in ("int8", "f16"):
        _case(out, "c1", dtype, 2, 3, 33, 70, 64, 72)
        _case(out, "c2_bias", dtype, 16, 4, 49, 49, 32, 32, bias="h_s_t", regime="conv")
        _case(out, "c3", dtype, 1, 2, 80, 80, 64, 64)
        _case(out, "c3_mask", dtype, 1, 2, 80, 80, 64, 64, bias="b_t")
        _case(out, "c3_mask_no_mul", dtype, 1, 2, 80, 80, 64, 64, bias="b_t", has_scale=False, regime="conv")
        _case(out, "c4_d68", dtype, 2, 2, 33, 65, 68, 68, pattern="bshd")
        for off in (1, 2, 4):
            _case(out, "c1_off%d" % off, dtype, 2, 3, 33, 70, 64, 72, offset=off)
        _case(out, "packed", dtype, 2, 2, 70, 70, 64, 64, pattern="packed")
        _case(out, "k0231", dtype, 2, 2, 33, 70, 64, 64, pattern="k0231", regime="conv")
        _case(out, "rank3", dtype, 1, 3, 33, 70, 64, 64, pattern="rank3")
        _case(out, "gaps", dtype, 2, 3, 33, 70, 64, 72, gap=8)
    _case(out, "specials_moved", "f16", 2, 2, 33, 70, 64, 64, special=True)
    out.append(dict(out[-1], name="layout_specials_raw_f16", moved=0))  # the same bits, read raw
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def case_id(c):
    return c["name"]


# ------------------------------------------------------------------------------------ the views
def chain_of(c, rows, inner, key):
    """(the source's dims, the steps [("reshape", dims) | ("transpose", perm)], swap_last2) that make operand `key`'s
    [B H][rows][inner] view; for "out" the destination's dims and the chain behind the core inverted"""
    B, H, pat = c["B"], c["H"], c["pattern"]
    if pat == "rank3":
        return (rows, H, inner), [("transpose", (1, 0, 2))], 0
    if pat == "k0231" and key == "k":
        return (B, rows, H, inner), [("transpose", (0, 2, 3, 1))], 1
    if pat == "bshd":
        return (B, rows, H, inner), [("transpose", (0, 2, 1, 3))], 0
    return (B, rows, H * inner), [("reshape", (B, rows, H, inner)), ("transpose", (0, 2, 1, 3))], 0


def numpy_view(src_dims, steps, swap):
    """(batches, rows, cols, element offsets [batches][rows][cols]) by numpy's own reshape and transpose"""
    idx = np.arange(int(np.prod(src_dims)), dtype=np.int64).reshape(src_dims)
    for kind, v in steps:
        idx = idx.reshape(v) if kind == "reshape" else idx.transpose(v)
    if swap:
        idx = idx.swapaxes(-1, -2)
    rows, cols = idx.shape[-2:]
    return idx.reshape(-1, rows, cols)


def derive(hip, src_dims, steps, swap):
    """(status, batches, rows, cols, heads, [outer, head, row]) through shl_mi355x_attention_layout_strides"""
    i32 = C.c_int32
    n = len(steps)
    dims = (i32 * len(src_dims))(*src_dims)
    is_t = (i32 * max(n, 1))(*[int(kind == "transpose") for kind, _ in steps])
    rank = (i32 * max(n, 1))(*[len(v) for _, v in steps])
    flat = (i32 * (MAX_DIM * max(n, 1)))()
    for i, (_, v) in enumerate(steps):
        for j, x in enumerate(v):
            flat[i * MAX_DIM + j] = x
    b, r, cl, h, st = i32(), i32(), i32(), i32(), (i32 * 3)()
    rc = hip.shl_mi355x_attention_layout_strides(dims, len(src_dims), n, is_t, rank, flat, swap, C.byref(b), C.byref(r), C.byref(cl),
                                                 C.byref(h), st)
    return rc, b.value, r.value, cl.value, h.value, list(st)


def strides_index(batches, rows, cols, heads, st):
    """[batches][rows][cols] -> element offset, by the layout descriptor's formula (include/shl_mi355x.h)"""
    bi = np.arange(batches, dtype=np.int64)
    return ((bi // heads) * st[0] + (bi % heads) * st[1])[:, None, None] + (np.arange(rows, dtype=np.int64) * st[2])[None, :, None] + \
        np.arange(cols, dtype=np.int64)[None, None, :]


def operands(c):
    """key -> (rows, inner) of q, k, v, out"""
    return dict(q=(c["s"], c["d"]), k=(c["t"], c["d"]), v=(c["t"], c["dv"]), out=(c["s"], c["dv"]))


def layout_desc(hip, c):
    ld = pkg.AttentionLayoutDesc()
    ld.moved = c["moved"]
    for key, (rows, inner) in operands(c).items():
        if c["pattern"] == "packed" and key != "out":  # a slice of [B, S, 3, H, D]: the strides of its [B, H, S, D] view
            heads, st = c["H"], [rows * 3 * c["H"] * inner, inner, 3 * c["H"] * inner]
        else:
            rc, b, r, cl, heads, st = derive(hip, *chain_of(c, rows, inner, key))
            assert rc == 0 and (b, r, cl) == (c["batches"], rows, inner), (key, rc, b, r, cl)
        if key == "out" and c["gap"]:  # rows further apart than the heads need
            row = st[2] + c["gap"]
            st = [rows * row, st[1], row]
        if key == "q":
            ld.heads = heads
        assert heads == ld.heads, (key, heads)
        getattr(ld, key + "_stride")[:] = st
    return ld


def bias_desc(c):
    """the bias descriptor of a [1,H,S,T] bias or a [B,1,1,T] mask over the batches B H"""
    bd = pkg.AttentionBiasDesc()
    s, t = c["s"], c["t"]
    bd.b_ext1 = c["H"]
    if c["bias_geom"] == "h_s_t":
        bd.b_stride[0], bd.b_stride[1], bd.row_stride, bd.key_stride = 0, s * t, t, 1
    else:
        bd.b_stride[0], bd.b_stride[1], bd.row_stride, bd.key_stride = t, 0, 0, 1
    (bd.b_scale, bd.b_zp), (bd.sb_scale, bd.sb_zp) = c["b_q"], c["sb_q"]
    return bd


def source_of(c, key):
    """the array the projection left: the dense operand permuted back on the host, [B, rows, H, inner] (rank3: [rows, H, inner])"""
    B, H = c["B"], c["H"]
    a = c[key]
    if c["pattern"] == "rank3":
        return np.ascontiguousarray(a.transpose(1, 0, 2))
    return np.ascontiguousarray(a.reshape(B, H, a.shape[1], a.shape[2]).transpose(0, 2, 1, 3))


# ------------------------------------------------------------------------------------ on the device
def _tdesc(c, dims, perm, rec):
    d = pkg.TransposeDesc()
    d.dtype = pkg.SHL_I8 if c["dtype"] == "int8" else pkg.SHL_F16
    d.rank = len(dims)
    d.dim[:len(dims)], d.perm[:len(perm)] = dims, perm
    (d.in_scale, d.in_zp), (d.out_scale, d.out_zp) = rec, rec
    return d


def _mdesc(c, rec):
    d = pkg.MoveDesc()
    d.dtype = pkg.SHL_I8 if c["dtype"] == "int8" else pkg.SHL_F16
    (d.in_scale, d.in_zp), (d.out_scale, d.out_zp) = rec, rec
    return d


def run_both(hip, dev, c):
    """(the layout launch's whole output frame, the frame the reference gives: poison but where its movers' output lands), as bytes"""
    B, H, s, dv, es = c["B"], c["H"], c["s"], c["dv"], c["q"].itemsize
    np_dt = c["q"].dtype
    off = c["offset"] * es
    ops = operands(c)
    room, src, dense = [], {}, {}

    def alloc(nbytes):
        room.append(dev.alloc(nbytes + 64))
        return room[-1]
    # the sources, where the projections left them
    if c["pattern"] == "packed":
        packed = np.ascontiguousarray(np.stack([source_of(c, key) for key in ("q", "k", "v")], axis=2))  # [B, S, 3, H, D]
        base = alloc(packed.nbytes) + off
        dev.upload(base, packed)
        for i, key in enumerate(("q", "k", "v")):
            src[key] = base + i * H * c["d"] * es
    else:
        for key in ("q", "k", "v"):
            a = source_of(c, key)
            src[key] = alloc(a.nbytes) + off
            dev.upload(src[key], a)
    bias = None
    if c["bias_geom"]:
        bias = alloc(c["bias"].nbytes)
        dev.upload(bias, c["bias"])
    # the reference's dense operands
    for key in ("q", "k", "v"):
        rows, inner = ops[key]
        if c["pattern"] == "packed" and c["moved"] and key != "q":
            continue  # (q's transpose has made all three)
        dense[key] = alloc(c[key].nbytes)
        if c["moved"] == 0:  # read raw: the dense kernel on a host-permuted copy
            dev.upload(dense[key], c[key])
            continue
        rec = c[key + "_q"]
        if c["pattern"] == "packed":
            whole = alloc(3 * c["q"].nbytes)
            td = _tdesc(c, (B, rows, 3, H, inner), (2, 0, 3, 1, 4), rec)
            pkg.check(hip.shl_mi355x_transpose(src["q"], whole, C.byref(td), None), hip, "shl_mi355x_transpose (packed)")
            for i, k2 in enumerate(("q", "k", "v")):
                dense[k2] = whole + i * c["q"].nbytes
            continue
        at = src[key]
        if c["pattern"] == "reshape":
            tmp = alloc(c[key].nbytes)
            pkg.check(hip.shl_mi355x_move(at, tmp, c[key].size, C.byref(_mdesc(c, rec)), None), hip, "shl_mi355x_move")
            at = tmp
        td = _tdesc(c, (rows, H, inner), (1, 0, 2), rec) if c["pattern"] == "rank3" else _tdesc(c, (B, rows, H, inner), (0, 2, 1, 3), rec)
        pkg.check(hip.shl_mi355x_transpose(at, dense[key], C.byref(td), None), hip, "shl_mi355x_transpose")
    d = ac.desc(c)
    bd = bias_desc(c) if bias else None
    bref = C.byref(bd) if bias else None
    out_dense = alloc(B * H * s * dv * es)
    if bias:
        assert hip.shl_mi355x_attention_bias_kernel_name(dense["q"], dense["k"], dense["v"], bias, out_dense, C.byref(d), bref).decode() == \
            pkg.ATTENTION_BIAS_MFMA, "both products must be the mfma form's"
        pkg.check(hip.shl_mi355x_attention_bias(dense["q"], dense["k"], dense["v"], bias, out_dense, C.byref(d), bref, None), hip,
                  "shl_mi355x_attention_bias")
    else:
        assert hip.shl_mi355x_attention_kernel_name(dense["q"], dense["k"], dense["v"], out_dense, C.byref(d)).decode() == pkg.ATTENTION_MFMA, \
            "both products must be the mfma form's"
        pkg.check(hip.shl_mi355x_attention(dense["q"], dense["k"], dense["v"], out_dense, C.byref(d), None), hip, "shl_mi355x_attention")
    if c["moved"] == 0:
        o = dev.download(out_dense, (B * H, s, dv), np_dt)
        merged = np.ascontiguousarray(o.transpose(1, 0, 2) if c["pattern"] == "rank3" else o.reshape(B, H, s, dv).transpose(0, 2, 1, 3))
    else:
        back = alloc(B * H * s * dv * es)
        rec = c["out_q"]
        td = _tdesc(c, (H, s, dv), (1, 0, 2), rec) if c["pattern"] == "rank3" else _tdesc(c, (B, H, s, dv), (0, 2, 1, 3), rec)
        pkg.check(hip.shl_mi355x_transpose(out_dense, back, C.byref(td), None), hip, "shl_mi355x_transpose (back)")
        if c["pattern"] == "reshape":
            back2 = alloc(B * H * s * dv * es)
            pkg.check(hip.shl_mi355x_move(back, back2, B * H * s * dv, C.byref(_mdesc(c, rec)), None), hip, "shl_mi355x_move (back)")
            back = back2
        merged = dev.download(back, (s, H, dv) if c["pattern"] == "rank3" else (B, s, H, dv), np_dt)
    # the layout launch into a poisoned frame
    ld = layout_desc(hip, c)
    ost = list(ld.out_stride)
    index = strides_index(B * H, s, dv, ld.heads, ost)
    span = int(index.max()) + 1
    frame = np.full(2 * GUARD + span * es, POISON, np.uint8)
    p_frame = alloc(frame.nbytes + 16) + off
    dev.upload(p_frame, frame)
    p_out = p_frame + GUARD
    args = (src["q"], src["k"], src["v"], bias, p_out, C.byref(d), bref, C.byref(ld))
    want_name = pkg.ATTENTION_BIAS_LAYOUT_MFMA if bias else pkg.ATTENTION_LAYOUT_MFMA
    assert hip.shl_mi355x_attention_layout_kernel_name(*args).decode() == want_name, hip.shl_mi355x_last_error()
    pkg.check(hip.shl_mi355x_attention_layout(*args, None), hip, "shl_mi355x_attention_layout")
    got = dev.download(p_frame, frame.shape, np.uint8)
    want = frame.copy()
    body = want[GUARD:GUARD + span * es].view(np_dt)
    # the movers' output [B, S, H, dv] lands at (b, h, row, col) of the view
    m = merged.transpose(1, 0, 2) if c["pattern"] == "rank3" else merged.transpose(0, 2, 1, 3).reshape(B * H, s, dv)
    body[index] = m
    for ptr in room:
        dev.free(ptr)
    return got, want

"""Shared helpers for the reductions: mean, sum, max, min (CSINN_OP_MEAN .. the stride family), reduce_mean, reduce_sum,
reduce_max, reduce_min (the axis family) and global_maxpool2d.

  all_cases()                       deterministic single-op problems, seeded by crc32(name): the smallest shapes at which each
                                    kernel form, a staging window's edge, a ragged head or tail, a merged or dropped group
                                    can still go wrong, and crafted rows whose float32 sum depends on its order
  descriptor(case)                  (kind, init, out groups, inner groups): what the nine ops become
  reduce_numpy                      plain numpy restatement of the reference (source/reference/mean.c, sum.c, max.c, min.c,
                                    reduce_*.c, global_maxpool.c behind shl_ref_siso_callback_base): dequantise with the
                                    input's record, ONE sequential float32 loop over the inner index, requantise with the
                                    output's; reverse=True walks the inner index backwards
  layer_run                         csinn_<op>_init + csinn_<op> through a front-end (layer mode)
  cabi_desc                         the C ABI's descriptor of a case
  expected_form                     the documented canonicalisation and form rule, restated
  ReduceNet, se_block(), cbam_block(), reid_tail()   small networks through the csinn session API (graph mode) with an
                                    oracle replay
The genuine library's outputs for the cases live in tests/golden/reduce_cases.npz (make_reduce_golden.py).
"""
import ctypes as C
import os
import zlib

import numpy as np

import cases
import concat_cases
import eltwise_cases
import move_cases
import pool_cases
import tail
from cases import pkg
from pool_cases import FLT_MAX, Q_CONV, Q_F16, _q, assert_same, bits  # noqa: F401

STRIDE_OPS = ("mean", "sum", "max", "min")
AXIS_OPS = ("reduce_mean", "reduce_sum", "reduce_max", "reduce_min")
OPS = STRIDE_OPS + AXIS_OPS + ("global_maxpool2d",)
KIND = {"sum": pkg.REDUCE_SUM, "mean": pkg.REDUCE_MEAN, "max": pkg.REDUCE_MAX, "min": pkg.REDUCE_MIN}
CHUNK = {"int8": pkg.REDUCE_CHUNK_BYTES, "f16": pkg.REDUCE_CHUNK_BYTES // 2}  # elements of the rows form's staging chunk
# inner sizes: the fixed list, and around the staging chunk of either dtype (below, equal, above, two chunks plus 3)
INNER_SIZES = sorted({1, 2, 63, 64, 65, 255, 256, 257} | {c + d for c in CHUNK.values() for d in (-1, 0, 1)} |
                     {2 * c + 3 for c in CHUNK.values()})
OUT_COUNTS = (1, 3, 63, 64, 65, 257)
NAN_P, NAN_N, INF_P, INF_N = 0x7E00, 0xFE00, 0x7C00, 0xFC00


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def kind_of(op):
    return op.split("_")[-1] if op != "global_maxpool2d" else "max"


def _data(name, dtype, shape):
    rng = _rng(name)
    if dtype == "int8":
        return rng.integers(-128, 128, shape, dtype=np.int8)
    return (3.0 * rng.standard_normal(shape)).astype(np.float16)


def out_record(kind, inner, in_q, name):
    """an int8 output record under which the outputs of random data spread over the int8 range instead of saturating: the
    scale follows the spread of the result (no power of two), the zero point is seeded"""
    s = np.float32(in_q[0])
    spread = {"sum": 74.0 * np.sqrt(inner) / 40.0, "mean": 74.0 / np.sqrt(inner) / 40.0, "max": 1.1, "min": 1.1}[kind]
    zp = 0 if kind in ("max", "min") else int(_rng("zp " + name).integers(-20, 21))
    return _q(s * np.float32(spread), zp)


# ------------------------------------------------------------------------------------ cases
def _out_shape(x, op, **kw):
    if op in STRIDE_OPS:
        keep = [x.shape[k] for k in range(x.ndim) if k not in kw["axes"]]
        return tuple(keep) or (1,)
    if op in AXIS_OPS:
        if kw["axis"] == -1:
            return (1,)
        return tuple(x.shape[k] for k in range(x.ndim) if k != kw["axis"]) or (1,)
    return (x.shape[0], x.shape[1], 1, 1) if kw["layout"] == "NCHW" else (x.shape[0], 1, 1, x.shape[3])


def _inner_of(x, op, **kw):
    if op in STRIDE_OPS:
        return int(np.prod([x.shape[k] for k in kw["axes"]]))
    if op in AXIS_OPS:
        return x.size if kw["axis"] == -1 else x.shape[kw["axis"]]
    return x.shape[2] * x.shape[3] if kw["layout"] == "NCHW" else x.shape[1] * x.shape[2]


def _add(out, op, name, dtype, x, in_q=None, out_q=None, **kw):
    full = "%s_%s" % (name, "f16" if dtype == "f16" else "i8")
    if dtype == "f16":
        in_q, out_q = Q_F16
    else:
        in_q = in_q or Q_CONV[0]
        out_q = out_q or out_record(kind_of(op), _inner_of(x, op, **kw), in_q, op + full)
    layout = kw.pop("layout", "NCHW")
    c = dict(op=op, name=full, dtype=dtype, in_q=in_q, out_q=out_q, x=np.ascontiguousarray(x), layout=layout, **kw)
    c["out_shape"] = _out_shape(x, op, layout=layout, **kw)
    out.append(c)


def _both(out, op, name, shape, x=None, **kw):
    for dtype in ("f16", "int8"):
        _add(out, op, name, dtype, _data("%s %s %s" % (op, name, dtype), dtype, shape) if x is None else x[dtype], **kw)


def size_cases():
    """every kind, both dtypes: each inner size as a row (reduced dim innermost: rows) and as a column (reduced dim outermost:
    cols); each output count likewise"""
    out = []
    for op in STRIDE_OPS:
        for n in INNER_SIZES:
            _both(out, op, "row_3x%d" % n, (3, n), axes=(1,))
            _both(out, op, "col_%dx3" % n, (n, 3), axes=(0,))
        for o in OUT_COUNTS:
            _both(out, op, "rows_%dx5" % o, (o, 5), axes=(1,))
            _both(out, op, "cols_5x%d" % o, (5, o), axes=(0,))
    return out


def group_cases():
    out = []
    for op in STRIDE_OPS:
        _both(out, op, "nchw_over_n_h", (2, 3, 4, 5), axes=(0, 2))           # two inner groups that do not merge
        _both(out, op, "three_outer_groups", (2, 3, 4, 5, 6), axes=(1, 3))
        _both(out, op, "nchw_over_hw", (2, 5, 7, 7), axes=(2, 3))            # 49-element rows off the 16-byte grid
        _both(out, op, "nhwc_over_hw", (2, 7, 7, 5), axes=(1, 2))
        _both(out, op, "channel_nchw", (1, 6, 5, 9), axes=(1,))              # CBAM's channel max / mean
        _both(out, op, "channel_nhwc", (1, 5, 9, 6), axes=(3,))
        _both(out, op, "rows_of_two_runs", (3, 4, 2, 9), axes=(1, 3))        # rows: several runs per output
        _both(out, op, "unit_dims", (1, 4, 1, 6), axes=(0, 3))
        _both(out, op, "everything", (3, 4, 5), axes=(0, 1, 2))
        _both(out, op, "nothing", (3, 4), axes=())                           # inner size 1 through no inner group at all
        _both(out, op, "strided_generic", (4, 3, 4), axes=(1,), generic=True)
    for op in AXIS_OPS:
        _both(out, op, "whole_tensor", (2, 3, 5), axis=-1)
        for axis in range(4):
            _both(out, op, "rank4_axis%d" % axis, (2, 3, 4, 5), axis=axis)
        _both(out, op, "last_axis_257", (3, 257), axis=1)
        _both(out, op, "first_axis_130", (130, 5), axis=0)
    for layout in ("NCHW", "NHWC"):
        for h, w in ((1, 1), (7, 7), (5, 9)):
            shape = (2, 5, h, w) if layout == "NCHW" else (2, h, w, 5)
            _both(out, "global_maxpool2d", "%dx%d_%s" % (h, w, layout.lower()), shape, layout=layout)
    return out


def long_row_cases():
    """one row of 2^16 elements: a single lane's chain"""
    out = []
    _both(out, "sum", "long_row", (1, 1 << 16), axes=(1,))
    _both(out, "reduce_max", "long_row", (1, 1 << 16), axis=-1)
    return out


ORDER_TERMS = 4096


def _cancelling_i8(name, rows):
    """rows of ORDER_TERMS int8 values whose exact sum is zero: a random half and its negation in another order, so what
    a float32 chain is left with is its own rounding -- which depends on the order"""
    rng = _rng(name)
    half = rng.integers(-127, 128, (rows, ORDER_TERMS // 2), dtype=np.int8)
    x = np.concatenate([half, -half], axis=1)
    for r in range(rows):
        x[r] = x[r, rng.permutation(ORDER_TERMS)]
    return x


def _f16_sum_rows():
    """crafted binary16 rows of ORDER_TERMS values each"""
    rng = _rng("f16 crafted sums")
    n = ORDER_TERMS
    rows = []
    tiny = (2.0 ** -14 * (1.0 + rng.random(n))).astype(np.float16)
    r = tiny.copy()                                    # 65504, many values near 2^-14, -65504
    r[0], r[-1] = 65504.0, -65504.0
    rows.append(r)
    r = tiny.copy()                                    # the same with values ahead of the large one and behind its negation
    r[70], r[-300] = 65504.0, -65504.0
    rows.append(r)
    big = (rng.choice([-1.0, 1.0], n // 4) * rng.uniform(1000.0, 60000.0, n // 4)).astype(np.float16)
    small = rng.uniform(-1.0, 1.0, n // 4).astype(np.float16)
    r = np.empty(n, np.float16)                        # alternating large and small magnitudes whose exact sum is zero
    r[0::2] = np.concatenate([big, -big])[rng.permutation(n // 2)]
    r[1::2] = np.concatenate([small, -small])[rng.permutation(n // 2)]
    rows.append(r)
    r = (3.0 * rng.standard_normal(n)).astype(np.float16)
    r.view(np.uint16)[n // 2] = INF_P                  # reaches inf midway and stays there
    rows.append(r)
    r = r.copy()
    r.view(np.uint16)[n // 2 + 9] = INF_N              # inf + -inf
    rows.append(r)
    r = np.zeros(n, np.float16)                        # a subnormal total: 2^-24 * 37 behind values that cancel exactly
    half = np.resize(big, n // 2 - 1) / np.float16(64)
    r[:n - 2] = np.concatenate([half, -half])[rng.permutation(n - 2)]
    r.view(np.uint16)[n - 1] = 37
    rows.append(r)
    for first, second in ((NAN_P, NAN_N), (NAN_N, NAN_P)):  # NaNs of both signs: the first one met keeps its sign
        r = (3.0 * rng.standard_normal(n)).astype(np.float16)
        r.view(np.uint16)[11], r.view(np.uint16)[n - 7] = first, second
        rows.append(r)
    r = (3.0 * rng.standard_normal(n)).astype(np.float16)   # a NaN behind inf + -inf
    r.view(np.uint16)[[3, 4, 5]] = [INF_P, INF_N, NAN_P]
    rows.append(r)
    return np.stack(rows)


def order_cases():
    """sum / mean whose float32 chain depends on its order: int8 with a scale that is no power of two (0.1f), mixed signs and an
    exact total of zero; crafted binary16 rows.  test_reduce_cpu.py asserts that the reverse order changes an output"""
    out = []
    q_in = _q(0.1, 0)
    xi = _cancelling_i8("int8 order rows", 8)
    xf = _f16_sum_rows()
    for op in ("sum", "mean"):
        # the total is rounding noise of some 1e-4 (sum) and 1 / 4096 of that (mean): records that resolve it
        q_out = _q(2.3e-5, 3) if op == "sum" else _q(2.3e-5 / ORDER_TERMS, 3)
        _add(out, op, "order_rows", "int8", xi, in_q=q_in, out_q=q_out, axes=(1,), order=True)
        _add(out, op, "order_cols", "int8", np.ascontiguousarray(xi.T), in_q=q_in, out_q=q_out, axes=(0,), order=True)
        _add(out, op, "order_rows", "f16", xf, axes=(1,), order=True)
        _add(out, op, "order_cols", "f16", np.ascontiguousarray(xf.T), axes=(0,), order=True)
    _add(out, "reduce_sum", "order_last_axis", "int8", xi, in_q=q_in, out_q=_q(2.3e-5, 3), axis=1, order=True)
    _add(out, "reduce_mean", "order_whole", "int8", xi[:1], in_q=q_in, out_q=_q(2.3e-5 / ORDER_TERMS, 3), axis=-1, order=True)
    _add(out, "reduce_sum", "order_last_axis", "f16", xf, axis=1, order=True)
    _add(out, "reduce_mean", "order_first_axis", "f16", np.ascontiguousarray(xf.T), axis=0, order=True)
    return out


def _f16_extreme_rows():
    """binary16 rows for max / min: +-0 mixes, NaN first / middle / last / everywhere, all -inf, all +inf, 65504 next to inf"""
    n = 9
    u = lambda *v: np.array(v, np.uint16)
    rows = [
        u(0x0000, 0x8000, 0x0000, 0x8000, 0x8000, 0x0000, 0x8000, 0x0000, 0x8000),   # +0 / -0: the later one of a tie stays
        u(0x8000, 0x0000, 0x8000, 0x0000, 0x0000, 0x8000, 0x0000, 0x8000, 0x0000),
        u(0x8000, 0x8000, 0x8000, 0x8000, 0x8000, 0x8000, 0x8000, 0x8000, 0x8000),
        u(NAN_P, 0x3C00, 0xC000, 0x4200, 0x0000, 0x8000, 0x3800, 0xB800, 0x4000),    # NaN first
        u(NAN_N, 0x3C00, 0xC000, 0x4200, 0x0000, 0x8000, 0x3800, 0xB800, 0x4000),
        u(0x3C00, 0xC000, 0x4200, 0x0000, NAN_P, 0x8000, 0x3800, 0xB800, 0x4000),    # NaN in the middle
        u(0x3C00, 0xC000, 0x4200, 0x0000, 0x8000, 0x3800, 0xB800, 0x4000, NAN_N),    # NaN last
        u(*([NAN_P] * n)),                                                           # NaN everywhere
        u(*([NAN_N] * n)),
        u(NAN_N, NAN_P, NAN_N, NAN_P, NAN_N, NAN_P, NAN_N, NAN_P, NAN_P),
        u(NAN_P, NAN_N, NAN_N, NAN_P, NAN_N, NAN_P, NAN_N, NAN_P, NAN_N),
        u(*([INF_N] * n)),                                                           # all -inf / all +inf
        u(*([INF_P] * n)),
        u(0x7BFF, INF_P, 0x7BFF, 0xFBFF, INF_N, 0xFBFF, 0x0000, 0x3C00, 0xBC00),     # 65504 next to inf
        u(0x7BFF, 0x7BFF, 0x3C00, 0xFBFF, 0xFBFF, 0x0000, 0x0001, 0x8001, 0x03FF),   # 65504 without it; subnormals
        u(0x0001, 0x8001, 0x0000, 0x8000, 0x0001, 0x8001, 0x8000, 0x0000, 0x8001),
    ]
    return np.stack(rows).view(np.float16)


def extreme_cases():
    out = []
    xf = _f16_extreme_rows()
    for kind in ("max", "min"):
        _add(out, kind, "special_rows", "f16", xf, axes=(1,))
        _add(out, kind, "special_cols", "f16", np.ascontiguousarray(xf.T), axes=(0,))
        _add(out, "reduce_" + kind, "special_last_axis", "f16", xf, axis=1)
        _add(out, "reduce_" + kind, "special_first_axis", "f16", np.ascontiguousarray(xf.T), axis=0)
        _add(out, "reduce_" + kind, "special_whole_nan_first", "f16", xf[3:4], axis=-1)
        _add(out, "reduce_" + kind, "special_whole_all_nan", "f16", xf[9:10], axis=-1)
    _add(out, "global_maxpool2d", "special_nchw", "f16", xf.reshape(2, 8, 3, 3), layout="NCHW")
    _add(out, "global_maxpool2d", "special_nhwc", "f16", np.ascontiguousarray(xf.reshape(2, 8, 3, 3).transpose(0, 2, 3, 1)), layout="NHWC")
    # extreme int8 records: zero points -128 and 127 on each side, an output scale that saturates both ends, one outside
    # div_by_scale's range (the hardware's division; the input scale keeps |x / s_out| below 2^20)
    recs = {"zp_in_lo": (_q(0.0473, -128), None), "zp_in_hi": (_q(0.0473, 127), None),
            "zp_out_lo": (_q(0.0473, -9), "lo"), "zp_out_hi": (_q(0.0473, -9), "hi"),
            "saturates": (_q(0.0473, -9), "sat"), "hw_division": (_q(5e-15, 3), "div")}
    for op in STRIDE_OPS + ("reduce_sum", "reduce_max"):
        for rname, (in_q, how) in recs.items():
            for shape, kw in (((5, 67), dict(axes=(1,))), ((67, 5), dict(axes=(0,)))):
                if op in AXIS_OPS:
                    kw = dict(axis=kw["axes"][0])
                x = _data("%s %s %s" % (op, rname, shape), "int8", shape)
                base = out_record(kind_of(op), 67, in_q, op + rname)
                out_q = {None: base, "lo": (base[0], -128), "hi": (base[0], 127), "sat": _q(base[0] / 16.0, 0),
                         "div": _q(base[0] * 0.55, -7)}[how]
                assert how != "div" or out_q[0] < 2.0 ** -40
                _add(out, op, "%s_%dx%d" % (rname, shape[0], shape[1]), "int8", x, in_q=in_q, out_q=out_q, **kw)
    return out


def all_cases():
    out = size_cases() + group_cases() + long_row_cases() + order_cases() + extreme_cases()
    names = [golden_key(c) for c in out]
    assert len(set(names)) == len(names)
    return out


def case_id(case):
    return "%s-%s" % (case["op"], case["name"])


def golden_key(case):
    return "%s.%s" % (case["op"], case["name"])


def golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reduce_cases.npz")
    blob = np.load(path)
    return {k: blob[k] for k in blob.files}


# ------------------------------------------------------------------------------------ what the nine ops become
def descriptor(case):
    """dict(kind, init, groups=(out_extents, out_strides, inner_extents, inner_strides)) in input elements"""
    op, shape = case["op"], case["x"].shape
    kind = KIND[kind_of(op)]
    if op in STRIDE_OPS:
        groups = pkg.reduce_groups(shape, case["axes"])
        if case.get("generic"):  # the same layer through a view of every other element of the last dim: no stride is 1
            oe, os_, ie, is_ = groups
            oe, os_ = list(oe), list(os_)
            oe[-1], os_[-1] = (shape[-1] + 1) // 2, 2
            groups = (oe, os_, ie, is_)
        return dict(kind=kind, init=pkg.REDUCE_INIT_FLT_MAX, groups=groups)
    if op in AXIS_OPS:
        if case["axis"] == -1:
            return dict(kind=kind, init=pkg.REDUCE_INIT_FIRST, groups=([], [], [case["x"].size], [1]))
        a = case["axis"]
        outer, cnt, inner = int(np.prod(shape[:a], dtype=np.int64)), shape[a], int(np.prod(shape[a + 1:], dtype=np.int64))
        return dict(kind=kind, init=pkg.REDUCE_INIT_FIRST, groups=([outer, inner], [cnt * inner, 1], [cnt], [inner]))
    n, c, h, w = shape if case["layout"] == "NCHW" else (shape[0], shape[3], shape[1], shape[2])
    if case["layout"] == "NCHW":
        return dict(kind=kind, init=pkg.REDUCE_INIT_FLT_MAX, groups=([n, c], [c * h * w, h * w], [h, w], [w, 1]))
    return dict(kind=kind, init=pkg.REDUCE_INIT_FLT_MAX, groups=([n, c], [c * h * w, 1], [h, w], [w * c, c]))


def out_shape_of(case):
    d = descriptor(case)
    if case.get("generic"):
        return tuple(d["groups"][0]) or (1,)
    return case["out_shape"]


def _indices(ext, strides):
    """shl_ref_get_reduction_index for every k: the first group is the outermost digit"""
    at = np.zeros(1, np.int64)
    for e, s in zip(ext, strides):
        at = (at[:, None] + np.arange(e, dtype=np.int64)[None, :] * s).reshape(-1)
    return at


def _fmax(acc, v):
    """fmax(acc, v) of the C library the reference is built against: a NaN operand loses, of two NaNs the first stays, of two
    equal operands (+0 and -0) the second is returned"""
    return np.where(np.isnan(v), acc, np.where(np.isnan(acc), v, np.where(acc > v, acc, v)))


def _fmin(acc, v):
    return np.where(np.isnan(v), acc, np.where(np.isnan(acc), v, np.where(acc < v, acc, v)))


_DEFAULT_NAN = np.array([0xFFC00000], np.uint32).view(np.float32)[0]


def _add_x86(acc, v):
    """acc += v as the reference's build computes it: acc's NaN is handed on, else v's; inf + -inf makes the default NaN, whose
    sign bit is set.  (float32_to_float16_base keeps a NaN's sign.)"""
    r = acc + v
    bad = np.isnan(r)
    if bad.any():
        r = np.where(bad, np.where(np.isnan(acc), acc, np.where(np.isnan(v), v, _DEFAULT_NAN)), r)
    return r


def _requantise(v, dtype, q):
    if dtype == "int8":
        return pool_cases.requantise(v, dtype, q)
    h = pool_cases.f32_to_f16_ref(v)
    nan = np.isnan(v)  # a NaN keeps its sign and nothing else
    h = np.where(nan, np.where(np.signbit(v), 0xFFFF, 0x7FFF), h).astype(np.uint16)
    return h.view(np.float16)


def reduce_numpy(case, x=None, reverse=False):
    x = case["x"] if x is None else x
    d = descriptor(case)
    oe, os_, ie, is_ = d["groups"]
    with np.errstate(all="ignore"):
        f = np.ascontiguousarray(pool_cases.dequantise(x, case["dtype"], case["in_q"]), dtype=np.float32).reshape(-1)
        base, off = _indices(oe, os_), _indices(ie, is_)
        if reverse:
            off = off[::-1]
        if d["kind"] in (pkg.REDUCE_SUM, pkg.REDUCE_MEAN):
            acc = np.zeros(base.size, np.float32)
            for o in off:  # the chain: one float32 addition per inner index, in order
                acc = _add_x86(acc, f[base + o])
            if d["kind"] == pkg.REDUCE_MEAN:
                nan = np.isnan(acc)
                acc = np.where(nan, acc, acc / np.float32(off.size))
        else:
            step = _fmax if d["kind"] == pkg.REDUCE_MAX else _fmin
            if d["init"] == pkg.REDUCE_INIT_FIRST:
                acc, rest = f[base + off[0]], off[1:]
            else:
                acc = np.full(base.size, -FLT_MAX if d["kind"] == pkg.REDUCE_MAX else FLT_MAX, np.float32)
                rest = off
            for o in rest:
                acc = step(acc, f[base + o])
        out = _requantise(np.ascontiguousarray(acc, dtype=np.float32), case["dtype"], case["out_q"])
    return np.ascontiguousarray(out).reshape(out_shape_of(case))


# ------------------------------------------------------------------------------------ the documented rules, restated
def canonical(ext, strides):
    """[(extent, stride)]: extent-1 groups dropped, a group merged into the one before it when that one's stride is this one's
    extent times its stride"""
    groups = []
    for e, s in zip(ext, strides):
        if e == 1:
            continue
        if groups and groups[-1][1] == e * s:
            groups[-1] = (groups[-1][0] * e, s)
        else:
            groups.append((e, s))
    return groups


def expected_form(case, force=None):
    oe, os_, ie, is_ = descriptor(case)["groups"]
    outer, inner = canonical(oe, os_), canonical(ie, is_)
    if force == "generic":
        return "reduce_generic"
    if inner and inner[-1][1] == 1:
        return "reduce_rows"
    if outer and outer[-1][1] == 1:
        return "reduce_cols"
    return "reduce_generic"


def cabi_desc(case, **override):
    d = pkg.ReduceDesc()
    info = descriptor(case)
    info.update(override)
    oe, os_, ie, is_ = info["groups"]
    d.dtype = pkg.SHL_I8 if case["dtype"] == "int8" else pkg.SHL_F16
    d.kind, d.init = info["kind"], info["init"]
    d.n_out, d.n_inner = len(oe), len(ie)
    for k in range(len(oe)):
        d.out_extent[k], d.out_stride[k] = oe[k], os_[k]
    for k in range(len(ie)):
        d.inner_extent[k], d.inner_stride[k] = ie[k], is_[k]
    d.in_elems = info.get("in_elems", case["x"].size)
    d.in_scale, d.in_zp = case["in_q"]
    d.out_scale, d.out_zp = case["out_q"]
    return d


# ------------------------------------------------------------------------------------ through csinn_*
def _layout(case):
    return pkg.LAYOUT_NHWC if case["layout"] == "NHWC" else pkg.LAYOUT_NCHW


def op_params(fe, keep, api, case, sess, layout=None, **kw):
    """the params block of a case; kw overrides fields (refusal tests): groups, axis, axis_count"""
    layout = _layout(case) if layout is None else layout
    op = case["op"]
    if op in STRIDE_OPS:
        return pkg.reduce_params(fe, keep, api, layout, groups=kw.get("groups", descriptor(case)["groups"]), sess=sess)
    if op in AXIS_OPS:
        return pkg.reduce_params(fe, keep, api, layout, axis=kw.get("axis", [case["axis"]]), sess=sess, axis_count=kw.get("axis_count"))
    return pkg.pool_params(fe, keep, api, layout, sess=sess)


def layer_run(fe, api, case, device=None, poison=None, out_shape=None, perf=None, **kw):
    """layer mode through csinn_<op> (+ _init).  device: a cases.HipDevice -- both tensors then are DMABUF tensors in HBM.
    Returns the output, or (status, output) when `poison` (a byte the output is pre-filled with) is given.  perf: a callable
    (callback block, input, output, params) run between init and exec."""
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, api, keep)
    dt = pkg.DTYPE_INT8 if case["dtype"] == "int8" else pkg.DTYPE_FLOAT16
    lay = _layout(case)
    x = case["x"]
    o = np.zeros(out_shape or out_shape_of(case), dtype=x.dtype)
    o.view(np.uint8)[...] = poison if poison is not None else 0
    allocs = []

    def place(arr):
        if device is None:
            return None
        p = device.alloc(arr.nbytes)
        device.upload(p, arr)
        allocs.append(p)
        return p
    t_in = pkg.make_tensor(fe, keep, x.shape, dt, lay, data=x, scales=(case["in_q"][0],), zps=(case["in_q"][1],), name=b"in",
                           sess=sess, device_ptr=place(x))
    p_out = place(o)
    t_out = pkg.make_tensor(fe, keep, o.shape, dt, lay, data=o, scales=(case["out_q"][0],), zps=(case["out_q"][1],), name=b"out",
                            sess=sess, device_ptr=p_out)
    params = op_params(fe, keep, api, case, sess, **kw)
    stem = "csinn_" + case["op"]
    args = (t_in, t_out, params)
    rc = getattr(fe, stem + "_init")(*args)
    if rc == pkg.CSINN_TRUE and perf is not None:
        perf(C.cast(params, C.POINTER(pkg.ParamsBase)).contents.cb, *args)
    if rc == pkg.CSINN_TRUE:
        rc = getattr(fe, stem)(*args)
    if device is not None:
        o = device.download(p_out, o.shape, o.dtype)
        for p in allocs:
            device.free(p)
    if poison is not None:
        return rc, o
    if rc != pkg.CSINN_TRUE:
        raise pkg.MI355XError("%s returned %d" % (stem, rc))
    return o


# ------------------------------------------------------------------------------------ networks around the reductions
class ReduceNet:
    """A small network given as a list of layers over named tensors, run two ways: through the csinn session API in graph
    mode, and as an oracle chain -- convolutions and fullyconnected through the C oracle (cases.oracle_run), relu, add and
    global_avgpool2d through the C oracle's restatements, everything else through the numpy restatements.  cut=True builds THE
    SAME GRAPH WITHOUT ITS REDUCTION LAYERS: each one's input becomes a graph output and its output a graph input, so that the
    fusion planner's counts can be compared (that graph is built, never run).

    tensors: name -> (shape, record).  layers: (kind, name, input or tuple of inputs, output, info) with kind conv (info: act,
    k, k_log2), fc, relu, gap, sigmoid, hard_sigmoid, add, mul, concat (info: axis), flatten, and the reductions: mean / max
    (info: axes), reduce_max (info: axis), gmp."""
    REDUCTIONS = ("mean", "sum", "max", "min", "reduce_mean", "reduce_sum", "reduce_max", "reduce_min", "gmp")

    def __init__(self, dtype, layout, seed, in_name, tensors, layers, outputs, cut=False):
        self.dtype, self.layout, self.cut = dtype, layout, cut
        self.in_name, self.tensors, self.layers, self.outputs = in_name, tensors, layers, list(outputs)
        int8 = dtype == "int8"
        nhwc = layout == "NHWC"
        rng = np.random.default_rng(seed)
        self.cv = {}
        for kind, name, src, dst, info in layers:
            if kind not in ("conv", "fc"):
                continue
            ishape, q_prev = tensors[src]
            oshape, out_q = tensors[dst]
            if kind == "fc":
                case = cases.make_case(int(rng.integers(1 << 30)), dtype=dtype, fc=True, n=ishape[0], c=ishape[1], co=oshape[1])
            else:
                cin, hin = (ishape[3], ishape[1]) if nhwc else (ishape[1], ishape[2])
                cout = oshape[3] if nhwc else oshape[1]
                k = info.get("k", 1)
                case = cases.make_case(int(rng.integers(1 << 30)), layout=layout, dtype=dtype, n=1, h=hin, w=hin, c=cin, co=cout,
                                       k=(k, k), pad=(k // 2,) * 4, act=info.get("act", 0))
                assert tuple(case["out_shape"]) == tuple(oshape), (name, case["out_shape"], oshape)
            if int8:
                case["in_scale"], case["in_zp"] = q_prev
                case["k_scale"] = np.array([2.0 ** info.get("k_log2", -7)], dtype=np.float32)
                case["b_scale"] = (np.float32(case["in_scale"]) * case["k_scale"]).astype(np.float32)
                case["bias"] = rng.integers(-2000, 2001, (case["co"],), dtype=np.int32)
                case["out_scale"], case["out_zp"] = out_q
            self.cv[name] = case

    def rec(self, name):
        return self.tensors[name][1] if self.dtype == "int8" else _q(1.0, 0)

    def shape(self, name):
        return tuple(self.tensors[name][0])

    def input(self, k):
        rng = np.random.default_rng(1100 + k)
        shape = self.shape(self.in_name)
        return rng.integers(-100, 100, shape, dtype=np.int8) if self.dtype == "int8" else rng.standard_normal(shape).astype(np.float16)

    def _reduce_case(self, kind, src, dst, info, x=None):
        op = "global_maxpool2d" if kind == "gmp" else kind
        x = np.zeros(self.shape(src), np.int8 if self.dtype == "int8" else np.float16) if x is None else x
        return dict(op=op, dtype=self.dtype, in_q=self.rec(src), out_q=self.rec(dst), x=x, out_shape=self.shape(dst),
                    axes=info.get("axes"), axis=info.get("axis"), layout=self.layout)

    # -- the oracle chain: every named tensor
    def oracle(self, x):
        env = {self.in_name: x}
        form = "ref" if self.dtype == "int8" else "f16"
        for kind, name, src, dst, info in self.layers:
            srcs = src if isinstance(src, tuple) else (src,)
            a = env[srcs[0]]
            if kind in ("conv", "fc"):
                case = dict(self.cv[name])
                case["input"] = np.ascontiguousarray(a).reshape(case["in_shape"])
                env[dst] = cases.oracle_run(case, form).reshape(self.shape(dst))
            elif kind in self.REDUCTIONS:
                env[dst] = reduce_numpy(self._reduce_case(kind, src, dst, info, a)).reshape(self.shape(dst))
            elif kind == "flatten":
                env[dst] = move_cases.move_numpy(dict(op="flatten", dtype=self.dtype, in_q=self.rec(src), out_q=self.rec(dst), x=a,
                                                      out_shape=self.shape(dst)))
            elif kind in ("sigmoid", "hard_sigmoid"):
                env[dst] = eltwise_cases.eltwise_numpy(dict(op=kind, x=a, dtype=self.dtype, in_q=self.rec(src), out_q=self.rec(dst), n=0.0))
            elif kind == "mul":
                env[dst] = eltwise_cases.eltwise_numpy(dict(op="mul", dtype=self.dtype, x=a, y=env[srcs[1]], in_q=self.rec(srcs[0]),
                                                            in1_q=self.rec(srcs[1]), out_q=self.rec(dst)))
            elif kind == "add":
                env[dst] = tail.siso_oracle(dict(kind="add", x=a, y=env[srcs[1]], dtype=self.dtype, layout=self.layout, axis=1,
                                                 in_q=self.rec(srcs[0]), in1_q=self.rec(srcs[1]), out_q=self.rec(dst)))
            elif kind == "concat":
                env[dst] = concat_cases.concat_numpy(dict(axis=info["axis"], out_shape=self.shape(dst), dtype=self.dtype,
                                                          xs=[env[s] for s in srcs], in_qs=[self.rec(s) for s in srcs],
                                                          out_q=self.rec(dst)))
            else:
                what = {"relu": "relu", "gap": "pool"}[kind]
                env[dst] = tail.siso_oracle(dict(kind=what, x=a, dtype=self.dtype, layout=self.layout, axis=1,
                                                 in_q=self.rec(src), out_q=self.rec(dst)))
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

        def A(name):  # an activation tensor: 2-d ones (around fullyconnected) are N C
            shape = self.shape(name)
            lay = {4: act_l, 2: pkg.LAYOUT_NC, 1: pkg.LAYOUT_N}.get(len(shape), act_l)
            return T(shape, self.rec(name), name.encode(), layout=lay)
        env = {self.in_name: A(self.in_name)}
        ops, inputs, outputs = [], [env[self.in_name]], []
        cut_away = set()
        for kind, name, src, dst, info in self.layers:
            srcs = src if isinstance(src, tuple) else (src,)
            env[dst] = A(dst)
            nm = name.encode()
            if kind in self.REDUCTIONS and self.cut:
                if srcs[0] not in cut_away and all(env[srcs[0]] is not t for t in outputs):
                    outputs.append(env[srcs[0]])
                inputs.append(env[dst])
                cut_away.add(dst)
            elif kind == "conv":
                case = self.cv[name]
                t_w = T(case["w_shape"], None, nm + b"_w", case["kernel"], 1, pkg.LAYOUT_OHWI if nhwc else pkg.LAYOUT_OIHW,
                        scales=tuple(case["k_scale"]))
                t_b = T((case["co"],), None, nm + b"_b", case["bias"], 1, pkg.LAYOUT_O, pkg.DTYPE_INT32 if int8 else dt,
                        scales=tuple(case["b_scale"]))
                p = pkg.conv_params(fe, keep, api, act_l, case["stride"], case["pad"], case["dilation"], case["group"], 0, sess, nm)
                ops.append(("csinn_conv2d" + ("_relu" if case["act"] else ""), (env[src], env[dst], t_w, t_b, p)))
            elif kind == "fc":
                case = self.cv[name]
                t_w = T((case["co"], case["c"]), None, nm + b"_w", case["kernel"], 1, pkg.LAYOUT_OI, scales=tuple(case["k_scale"]))
                t_b = T((case["co"],), None, nm + b"_b", case["bias"], 1, pkg.LAYOUT_O, pkg.DTYPE_INT32 if int8 else dt,
                        scales=tuple(case["b_scale"]))
                ops.append(("csinn_fullyconnected", (env[src], env[dst], t_w, t_b, pkg.fc_params(fe, keep, api, case["co"], 0, sess, nm))))
            elif kind in self.REDUCTIONS:
                case = self._reduce_case(kind, src, dst, info)
                ops.append(("csinn_" + case["op"], (env[src], env[dst], op_params(fe, keep, api, case, sess, layout=act_l))))
            elif kind == "flatten":
                ops.append(("csinn_flatten", (env[src], env[dst], pkg.flatten_params(fe, keep, api, act_l, 1, sess))))
            elif kind in ("add", "mul"):
                ops.append(("csinn_" + kind, (env[srcs[0]], env[srcs[1]], env[dst], pkg.siso_params(fe, keep, api, kind, act_l, 1, sess, nm))))
            elif kind == "concat":
                p = pkg.concat_params(fe, keep, api, act_l, len(srcs), info["axis"], sess, nm)
                ops.append(("csinn_concat", (pkg.tensor_array(keep, [env[s] for s in srcs]), env[dst], p)))
            else:
                what = {"relu": "relu", "gap": "pool", "sigmoid": "sigmoid", "hard_sigmoid": "hard_sigmoid"}[kind]
                stem = {"gap": "csinn_global_avgpool2d"}.get(kind, "csinn_" + kind)
                ops.append((stem, (env[src], env[dst], pkg.siso_params(fe, keep, api, what, act_l, 1, sess, nm))))
        outputs.extend(env[o] for o in self.outputs if o not in cut_away and all(env[o] is not t for t in outputs))
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

    run = move_cases.MoveNet.run
    close = tail.MiniNet.close


def _act(layout, c, h):
    return (1, h, h, c) if layout == "NHWC" else (1, c, h, h)


def se_block(dtype="int8", layout="NHWC", cut=False):
    """a TensorFlow-style squeeze-and-excite block: 8x8x16 -> conv3x3 + relu (32) -> MEAN over H and W -> 1x1 (8) + a relu
    LAYER (which a session folds) -> 1x1 (32) -> hard_sigmoid -> broadcast mul with the feature map"""
    q = lambda s, z: _q(2.0 ** s, z)
    hw = (1, 2) if layout == "NHWC" else (2, 3)
    t = {"data": (_act(layout, 16, 8), q(-4, -5)), "c0": (_act(layout, 32, 8), q(-3, -100)), "sq": (_act(layout, 32, 1), q(-5, -128)),
         "fc1c": (_act(layout, 8, 1), q(-4, -100)), "fc1": (_act(layout, 8, 1), q(-4, -100)), "fc2": (_act(layout, 32, 1), q(-4, 3)),
         "gate": (_act(layout, 32, 1), _q(1.0 / 256, -128)), "se": (_act(layout, 32, 8), q(-3, -100))}
    L = [("conv", "c0", "data", "c0", dict(act=1, k=3)),
         ("mean", "squeeze", "c0", "sq", dict(axes=hw)),
         ("conv", "fc1", "sq", "fc1c", dict(act=0, k_log2=-5)),
         ("relu", "fc1_relu", "fc1c", "fc1", {}),
         ("conv", "fc2", "fc1", "fc2", dict(act=0, k_log2=-5)),
         ("hard_sigmoid", "gate", "fc2", "gate", {}),
         ("mul", "excite", ("c0", "gate"), "se", {})]
    return ReduceNet(dtype, layout, 61, "data", t, L, ["se"], cut=cut)


def cbam_block(dtype="int8", layout="NHWC", cut=False):
    """a CBAM block on 8x8x16: channel attention -- global_maxpool2d and global_avgpool2d, each through a 1x1 pair (8, 16) with
    a relu LAYER between, add -> sigmoid -> mul; then spatial attention -- MAX and MEAN over the channel axis -> concat -> 3x3
    conv to one channel -> sigmoid -> mul"""
    q = lambda s, z: _q(2.0 ** s, z)
    nhwc = layout == "NHWC"
    c_axis = 3 if nhwc else 1
    one = _act(layout, 1, 8)
    t = {"data": (_act(layout, 16, 8), q(-4, -5)), "f": (_act(layout, 16, 8), q(-3, -100)),
         "mx": (_act(layout, 16, 1), q(-3, -100)), "av": (_act(layout, 16, 1), q(-5, -128)),
         "m1c": (_act(layout, 8, 1), q(-3, -100)), "m1": (_act(layout, 8, 1), q(-3, -100)), "m2": (_act(layout, 16, 1), q(-3, 3)),
         "a1c": (_act(layout, 8, 1), q(-4, -100)), "a1": (_act(layout, 8, 1), q(-4, -100)), "a2": (_act(layout, 16, 1), q(-4, 3)),
         "both": (_act(layout, 16, 1), q(-2, 5)), "cgate": (_act(layout, 16, 1), _q(1.0 / 256, -128)),
         "fc": (_act(layout, 16, 8), q(-3, -100)),
         "smax": (one, q(-3, -100)), "smean": (one, q(-4, -110)), "cat": (_act(layout, 2, 8), q(-3, -100)),
         "sconv": (one, q(-3, 7)), "sgate": (one, _q(1.0 / 256, -128)), "out": (_act(layout, 16, 8), q(-3, -100))}
    L = [("conv", "c0", "data", "f", dict(act=1, k=3)),
         ("gmp", "gmp", "f", "mx", {}),
         ("gap", "gap", "f", "av", {}),
         ("conv", "m1", "mx", "m1c", dict(act=0, k_log2=-5)),
         ("relu", "m1_relu", "m1c", "m1", {}),
         ("conv", "m2", "m1", "m2", dict(act=0, k_log2=-5)),
         ("conv", "a1", "av", "a1c", dict(act=0, k_log2=-5)),
         ("relu", "a1_relu", "a1c", "a1", {}),
         ("conv", "a2", "a1", "a2", dict(act=0, k_log2=-5)),
         ("add", "both", ("m2", "a2"), "both", {}),
         ("sigmoid", "cgate", "both", "cgate", {}),
         ("mul", "channel", ("f", "cgate"), "fc", {}),
         ("max", "smax", "fc", "smax", dict(axes=(c_axis,))),
         ("mean", "smean", "fc", "smean", dict(axes=(c_axis,))),
         ("concat", "cat", ("smax", "smean"), "cat", dict(axis=c_axis)),
         ("conv", "sconv", "cat", "sconv", dict(act=0, k=3, k_log2=-5)),
         ("sigmoid", "sgate", "sconv", "sgate", {}),
         ("mul", "spatial", ("fc", "sgate"), "out", {})]
    return ReduceNet(dtype, layout, 63, "data", t, L, ["out"], cut=cut)


def reid_tail(dtype="int8", layout="NHWC", cut=False, classes=24):
    """a ReID tail: 8x8x16 -> conv1x1 (32) + a relu LAYER -> global_maxpool2d -> flatten -> fullyconnected, with reduce_max over
    the class axis as a second graph output"""
    q = lambda s, z: _q(2.0 ** s, z)
    t = {"data": (_act(layout, 16, 8), q(-4, -5)), "c1c": (_act(layout, 32, 8), q(-3, -100)), "c1": (_act(layout, 32, 8), q(-3, -100)),
         "gmp": (_act(layout, 32, 1), q(-3, -100)), "flat": ((1, 32), q(-4, -120)), "fc": ((1, classes), q(-3, -11)),
         "best": ((1,), q(-3, -20))}
    L = [("conv", "c1", "data", "c1c", dict(act=0)),
         ("relu", "c1_relu", "c1c", "c1", {}),
         ("gmp", "gmp", "c1", "gmp", {}),
         ("flatten", "flat", "gmp", "flat", {}),
         ("fc", "fc", "flat", "fc", dict(k_log2=-8)),
         ("reduce_max", "best", "fc", "best", dict(axis=1))]
    return ReduceNet(dtype, layout, 67, "data", t, L, ["fc", "best"], cut=cut)


NETS = {"se_block": se_block, "cbam_block": cbam_block, "reid_tail": reid_tail}
CUT_LAYERS = {"se_block": 1, "cbam_block": 3, "reid_tail": 2}

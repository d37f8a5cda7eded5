"""Shared helpers for the operators that only change a tensor's order or shape: transpose (CSINN_OP_TRANSPOSE), pad
(CSINN_OP_PAD), reshape (CSINN_OP_RESHAPE) and flatten (CSINN_OP_FLATTEN).

  transpose_cases() / pad_cases() / flat_cases()   deterministic single-op problems, seeded by crc32(name): the smallest
                                    shapes at which each kernel form, an edge tile, a ragged extent, a merged or dropped dim
                                    can still go wrong
  move_numpy                        plain numpy restatement of the reference (source/reference/transpose.c, pad.c, reshape.c,
                                    flatten.c behind shl_ref_siso_callback_base): dequantise with the input's record, move,
                                    requantise with the output's
  layer_run                         csinn_<op>_init + csinn_<op> through a front-end (layer mode)
  cabi_args                         what the C ABI takes, from a case
  canonical / expected_form         the documented canonicalisation and form rules, restated
  MoveNet, classifier_tail(), tf_stride2_block(), detection_head()   small networks through the csinn session API (graph
                                    mode) with an oracle replay: convolutions and fullyconnected through the C oracle
                                    (cases.oracle_run), the rest through the numpy restatements
The genuine library's outputs for the cases live in tests/golden/move_cases.npz (make_move_golden.py).
"""
import ctypes as C
import os
import zlib

import numpy as np

import cases
import eltwise_cases
import pool_cases
import tail
from cases import pkg
from pool_cases import Q_CONV, Q_F16, Q_SAME, _q, assert_same, bits  # noqa: F401

# (input record, output record): equal; the scale alone differs; the zero point alone; both (converter scales: no power of
# two); both with an output scale below 2^-40, which div_by_scale does not admit: the hardware's division
RECORDS = {
    "eq": (Q_SAME, Q_SAME),
    "scale": (_q(2.0 ** -4, -5), _q(2.0 ** -3, -5)),
    "zp": (_q(2.0 ** -4, -5), _q(2.0 ** -4, 9)),
    "both": (Q_CONV[1], Q_CONV[0]),
    "div": (_q(5e-13, 3), _q(3e-13, -7)),
}
REC_ORDER = ["both", "eq", "scale", "zp", "div"]
# +-inf, quiet and signalling NaNs of both signs, the smallest and largest subnormals of both signs, +-0
F16_SPECIALS = np.array([0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFFFF, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0000, 0x8000], np.uint16)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _data(name, dtype, shape):
    rng = _rng(name)
    if dtype == "int8":
        return rng.integers(-128, 128, shape, dtype=np.int8)
    x = (3.0 * rng.standard_normal(shape)).astype(np.float16)
    flat = x.reshape(-1).view(np.uint16)
    at = rng.permutation(flat.size)[:F16_SPECIALS.size]  # as many specials as the tensor has room for
    flat[at] = F16_SPECIALS[:at.size]
    return x


# ------------------------------------------------------------------------------------ cases
TRANSPOSES = [
    # (name, shape, permutation, int8 records beyond the rotating one)
    ("3x5", (3, 5), (1, 0), ()),
    ("64x64", (64, 64), (1, 0), ()),
    ("65x67", (65, 67), (1, 0), REC_ORDER),                      # edge tiles both ways
    ("128x4", (128, 4), (1, 0), ()),
    ("4x128", (4, 128), (1, 0), ()),
    ("2x3x5x7_to_nhwc", (2, 3, 5, 7), (0, 2, 3, 1), REC_ORDER),
    ("2x3x5x7_to_nchw", (2, 3, 5, 7), (0, 3, 1, 2), ()),
    ("1x64x8x8_to_nhwc", (1, 64, 8, 8), (0, 2, 3, 1), ("eq",)),   # aligned everywhere
    ("1x8x8x64_to_nchw", (1, 8, 8, 64), (0, 3, 1, 2), ()),
    ("2x16x7x7_to_nhwc", (2, 16, 7, 7), (0, 2, 3, 1), ()),       # 49-byte planes
    ("yolo_1x3x8x4x4", (1, 3, 8, 4, 4), (0, 1, 3, 4, 2), ("eq",)),
    ("heads_2x5x4x16", (2, 5, 4, 16), (0, 2, 1, 3), REC_ORDER),   # the rows form at 16-byte runs ...
    ("heads_2x5x4x6", (2, 5, 4, 6), (0, 2, 1, 3), ()),            # ... and at none (binary16: 4-byte pieces)
    ("heads_2x5x4x4", (2, 5, 4, 4), (0, 2, 1, 3), ()),            # int8: 4-byte pieces
    ("2x3x4x5_reversed", (2, 3, 4, 5), (3, 2, 1, 0), ()),
    ("2x3x4x5_2031", (2, 3, 4, 5), (2, 0, 3, 1), ()),
    ("1x1x7x3_unit_dims", (1, 1, 7, 3), (3, 1, 2, 0), ()),
    ("identity_2x3x4x5", (2, 3, 4, 5), (0, 1, 2, 3), ("eq",)),
    ("identity_17", (17,), (0,), ()),
    ("rank6", (2, 2, 3, 2, 2, 3), (0, 3, 1, 4, 2, 5), ()),
    ("rank8_reversed", (2,) * 8, (7, 6, 5, 4, 3, 2, 1, 0), ()),
    ("rank8_pairs", (2,) * 8, (0, 2, 1, 3, 5, 4, 7, 6), ()),
    ("3x130x70", (3, 130, 70), (0, 2, 1), ()),                    # several tiles each way and a batch dim
    ("5x8", (5, 8), (1, 0), ()),                                  # one ragged side: dword loads, element stores ...
    ("8x5", (8, 5), (1, 0), ()),                                  # ... and element loads, dword stores
    ("2x67x132", (2, 67, 132), (0, 2, 1), ("eq",)),               # the same over several tiles
    ("2x132x67", (2, 132, 67), (0, 2, 1), ("eq",)),
]


def _add(out, op, name, dtype, rec, x, out_shape, **kw):
    in_q, out_q = Q_F16 if dtype == "f16" else RECORDS[rec]
    out.append(dict(op=op, name="%s_%s" % (name, "f16" if dtype == "f16" else "i8_" + rec), dtype=dtype, in_q=in_q, out_q=out_q,
                    x=np.ascontiguousarray(x), out_shape=tuple(out_shape), layout=kw.pop("layout", "NHWC"), **kw))


def transpose_cases():
    out = []
    for i, (name, shape, perm, extra) in enumerate(TRANSPOSES):
        oshape = tuple(shape[p] for p in perm)
        _add(out, "transpose", name, "f16", None, _data(name + " f16", "f16", shape), oshape, perm=tuple(perm))
        for rec in dict.fromkeys((REC_ORDER[i % len(REC_ORDER)],) + tuple(extra)):
            _add(out, "transpose", name, "int8", rec, _data(name + " i8", "int8", shape), oshape, perm=tuple(perm))
    return out


def _mem(layout, shape_nhwc, pads_nhwc):
    """shape and (before, after) per dim in memory order, from N, H, W, C order"""
    order = (0, 1, 2, 3) if layout == "NHWC" else (0, 3, 1, 2)
    return tuple(shape_nhwc[k] for k in order), [pads_nhwc[k][0] for k in order], [pads_nhwc[k][1] for k in order]


PADS = [
    # (name, shape as N H W C, pads as ((before, after) for N, H, W, C), value, int8 records beyond the rotating one)
    ("same_01", (1, 5, 5, 3), ((0, 0), (0, 1), (0, 1), (0, 0)), 0.0, ("eq",)),       # TensorFlow's SAME in front of stride 2
    ("hw_11", (1, 5, 5, 3), ((0, 0), (1, 1), (1, 1), (0, 0)), -1.5, REC_ORDER),
    ("hw_23", (1, 5, 5, 3), ((0, 0), (2, 3), (2, 3), (0, 0)), 0.0, ()),
    ("channels_3_to_8", (1, 5, 5, 3), ((0, 0), (0, 0), (0, 0), (2, 3)), -1.5, ()),
    ("batch", (1, 5, 5, 3), ((1, 2), (0, 0), (0, 0), (0, 0)), 0.0, ()),
    ("every_pad_zero", (1, 5, 5, 3), ((0, 0),) * 4, 0.0, ("eq",)),
    ("vec_2x4x4x16_hw_11", (2, 4, 4, 16), ((0, 0), (1, 1), (1, 1), (0, 0)), -1.5, REC_ORDER),
    ("vec_1x4x4x16_w_01_c_0_16", (1, 4, 4, 16), ((0, 0), (0, 0), (0, 1), (0, 16)), 0.0, ("eq",)),
    ("all_dims", (2, 3, 4, 5), ((1, 0), (0, 2), (1, 1), (3, 0)), 0.5, ()),
    ("saturates_up", (1, 5, 5, 3), ((0, 0), (1, 1), (1, 1), (0, 0)), 1000.0, ("eq",)),
    ("saturates_down", (1, 5, 5, 3), ((0, 0), (1, 1), (1, 1), (0, 0)), -1000.0, ("eq",)),
]
F16_PAD_VALUES = [("minus_inf", -np.inf), ("plus_inf", np.inf), ("beyond_range", 70000.0), ("subnormal", 1e-7)]


def pad_cases():
    out = []
    i = 0
    for layout in ("NHWC", "NCHW"):
        for name, shape, pads, value, extra in PADS:
            mshape, before, after = _mem(layout, shape, pads)
            oshape = tuple(s + b + a for s, b, a in zip(mshape, before, after))
            nm = "%s_%s" % (name, layout.lower())
            kw = dict(before=before, after=after, value=float(value), layout=layout)
            _add(out, "pad", nm, "f16", None, _data(nm + " f16", "f16", mshape), oshape, **kw)
            for rec in dict.fromkeys((REC_ORDER[i % len(REC_ORDER)],) + tuple(extra)):
                if rec == "div" and value != 0.0:
                    continue  # |v / s_out| must stay below 2^20: the reference's own float-to-int conversion is defined
                _add(out, "pad", nm, "int8", rec, _data(nm + " i8", "int8", mshape), oshape, **kw)
            i += 1
        for vname, value in F16_PAD_VALUES:
            mshape, before, after = _mem(layout, (1, 5, 5, 3), ((0, 0), (1, 1), (1, 1), (0, 0)))
            oshape = tuple(s + b + a for s, b, a in zip(mshape, before, after))
            nm = "value_%s_%s" % (vname, layout.lower())
            _add(out, "pad", nm, "f16", None, _data(nm, "f16", mshape), oshape, before=before, after=after, value=float(value),
                 layout=layout)
    return out


FLATS = [("1", (1,), (1, 1)), ("15", (3, 5), (15,)), ("16", (2, 8), (1, 16)), ("17", (17,), (1, 17)), ("4099", (1, 4099), (4099,)),
         ("2x1x1x24", (2, 1, 1, 24), (2, 24)), ("1x24x4x4", (1, 24, 4, 4), (1, 3, 8, 4, 4))]


def flat_cases():
    out = []
    for i, (name, shape, oshape) in enumerate(FLATS):
        for op in ("reshape", "flatten"):
            _add(out, op, name, "f16", None, _data(op + name + " f16", "f16", shape), oshape)
            for rec in dict.fromkeys((REC_ORDER[(i + (op == "flatten")) % len(REC_ORDER)], "eq")):
                _add(out, op, name, "int8", rec, _data(op + name + " i8", "int8", shape), oshape)
    return out


def all_cases():
    out = transpose_cases() + pad_cases() + flat_cases()
    names = [c["op"] + "." + c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def case_id(case):
    return "%s-%s" % (case["op"], case["name"])


# ------------------------------------------------------------------------------------ numpy restatement
def move_numpy(case, x=None):
    x = case["x"] if x is None else x
    dt = case["dtype"]
    with np.errstate(all="ignore"):
        f = pool_cases.dequantise(x, dt, case["in_q"])
        if case["op"] == "transpose":
            f = np.transpose(f, case["perm"])
        elif case["op"] == "pad":
            f = np.pad(f, list(zip(case["before"], case["after"])), constant_values=np.float32(case["value"]))
        else:
            f = f.reshape(case["out_shape"])
        return np.ascontiguousarray(pool_cases.requantise(np.ascontiguousarray(f, dtype=np.float32), dt, case["out_q"]))


def golden_key(case):
    return "%s.%s" % (case["op"], case["name"])


def golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "move_cases.npz")
    blob = np.load(path)
    return {k: blob[k] for k in blob.files}


def _layout(case):
    return pkg.LAYOUT_NHWC if case["layout"] == "NHWC" else pkg.LAYOUT_NCHW


# ------------------------------------------------------------------------------------ through csinn_*
def op_params(fe, keep, api, case, sess, layout=None, **kw):
    """the params block of a case; kw overrides fields (refusal tests): perm, permute_num, before, after, pad_num, mode,
    value"""
    layout = _layout(case) if layout is None else layout
    op = case["op"]
    if op == "transpose":
        return pkg.transpose_params(fe, keep, api, layout, list(kw.get("perm", case["perm"])), sess,
                                    permute_num=kw.get("permute_num"))
    if op == "pad":
        return pkg.pad_params(fe, keep, api, layout, list(kw.get("before", case["before"])), list(kw.get("after", case["after"])),
                              kw.get("value", case["value"]), kw.get("mode", pkg.PAD_CONSTANT), sess, pad_num=kw.get("pad_num"))
    if op == "reshape":
        return pkg.reshape_params(fe, keep, api, layout, list(case["out_shape"]), sess)
    return pkg.flatten_params(fe, keep, api, layout, 1, sess)


def layer_run(fe, api, case, device=None, poison=None, out_shape=None, in_scales=None, out_dt=None, perf=None, layout=None, **kw):
    """layer mode through csinn_<op> (+ _init).  device: a cases.HipDevice -- both tensors then are DMABUF tensors in HBM.
    Returns the output, or (status, output) when `poison` (a byte the output is pre-filled with) is given.  out_shape /
    in_scales / out_dt / layout / kw override what the case says (refusal tests).  perf: a callable (callback block, input,
    output, params) run between init and exec."""
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, api, keep)
    dt = pkg.DTYPE_INT8 if case["dtype"] == "int8" else pkg.DTYPE_FLOAT16
    lay = _layout(case) if layout is None else layout
    x = case["x"]
    o = np.zeros(out_shape or case["out_shape"], dtype=x.dtype)
    o.view(np.uint8)[...] = poison if poison is not None else 0
    allocs = []

    def place(arr):
        if device is None:
            return None
        p = device.alloc(arr.nbytes)
        device.upload(p, arr)
        allocs.append(p)
        return p
    t_in = pkg.make_tensor(fe, keep, x.shape, dt, lay, data=x, scales=in_scales or (case["in_q"][0],), zps=(case["in_q"][1],),
                           name=b"in", sess=sess, device_ptr=place(x))
    p_out = place(o)
    t_out = pkg.make_tensor(fe, keep, o.shape, out_dt or dt, lay, data=o, scales=(case["out_q"][0],), zps=(case["out_q"][1],),
                            name=b"out", sess=sess, device_ptr=p_out)
    params = op_params(fe, keep, api, case, sess, layout=lay, **kw)
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


class CabiArgs:
    """the descriptor the C ABI takes for a case, and the call"""

    def __init__(self, case):
        self.op = case["op"]
        x = case["x"]
        dtype = pkg.SHL_I8 if case["dtype"] == "int8" else pkg.SHL_F16
        if self.op == "transpose":
            d = pkg.TransposeDesc()
            d.rank = x.ndim
            for k in range(x.ndim):
                d.dim[k], d.perm[k] = x.shape[k], case["perm"][k]
        elif self.op == "pad":
            d = pkg.PadDesc()
            for k in range(4):
                d.dim[k], d.before[k], d.after[k] = x.shape[k], case["before"][k], case["after"][k]
            d.pad_value = case["value"]
        else:
            d = pkg.MoveDesc()
            self.elems = x.size
        d.dtype = dtype
        d.in_scale, d.in_zp = case["in_q"]
        d.out_scale, d.out_zp = case["out_q"]
        self.desc = d

    def name(self, hip, in_ptr, out_ptr):
        if self.op == "transpose":
            return hip.shl_mi355x_transpose_kernel_name(in_ptr, out_ptr, C.byref(self.desc)).decode()
        if self.op == "pad":
            return hip.shl_mi355x_pad_kernel_name(in_ptr, out_ptr, C.byref(self.desc)).decode()
        return hip.shl_mi355x_move_kernel_name(in_ptr, out_ptr, self.elems, C.byref(self.desc)).decode()

    def run(self, hip, in_ptr, out_ptr, stream=None):
        if self.op == "transpose":
            return hip.shl_mi355x_transpose(in_ptr, out_ptr, C.byref(self.desc), stream)
        if self.op == "pad":
            return hip.shl_mi355x_pad(in_ptr, out_ptr, C.byref(self.desc), stream)
        return hip.shl_mi355x_move(in_ptr, out_ptr, self.elems, C.byref(self.desc), stream)


def cabi_args(case):
    return CabiArgs(case)


# ------------------------------------------------------------------------------------ the documented rules, restated
FORM_ENV = {"transpose": "SHL_MI355X_TRANSPOSE_FORM", "reshape": "SHL_MI355X_TRANSPOSE_FORM", "flatten": "SHL_MI355X_TRANSPOSE_FORM",
            "pad": "SHL_MI355X_PAD_FORM"}
FORCES = {"transpose": ["generic", "tile", "rows"], "reshape": ["generic", "tile", "rows"], "flatten": ["generic", "tile", "rows"],
          "pad": ["generic"]}


def canonical(shape, perm):
    """[(extent, stride in the input)] in output order: dims of extent 1 dropped, dims that follow each other in the output
    and are contiguous in the input merged"""
    stride = [int(np.prod(shape[j + 1:], dtype=np.int64)) for j in range(len(shape))]
    dims = []
    for j in perm:
        if shape[j] == 1:
            continue
        if dims and dims[-1][1] == shape[j] * stride[j]:
            dims[-1] = (dims[-1][0] * shape[j], stride[j])
        else:
            dims.append((shape[j], stride[j]))
    return dims or [(1, 1)]


def expected_form(case, force=None, align=16, align_in=None, align_out=None):
    """the form the documented rules give a case whose buffers are `align`-byte aligned (align_in / align_out: that one of
    them only), under a value of the switch"""
    align_in, align_out = align_in or align, align_out or align
    align = min(align_in, align_out)
    es = 1 if case["dtype"] == "int8" else 2
    x = case["x"]
    if case["op"] == "pad":
        if force == "generic" or align < 16:
            return "pad_generic"
        j = max([k for k in range(1, 4) if case["before"][k] or case["after"][k]], default=0)
        unit = es * int(np.prod(x.shape[j + 1:], dtype=np.int64))
        ok = all(v * unit % 16 == 0 for v in (case["before"][j], x.shape[j], case["after"][j]))
        return "pad_vec" if ok else "pad_generic"
    dims = canonical(x.shape, case["perm"]) if case["op"] == "transpose" else [(x.size, 1)]
    if force == "generic":
        return "transpose_generic"
    if force is None and len(dims) == 1 and align >= 16:
        return "transpose_flat"
    if dims[-1][1] == 1:
        run = dims[-1][0] * es
        w = 16 if run % 16 == 0 and align >= 16 else 4 if run % 4 == 0 and align >= 4 else 0
        return "transpose_rows_%d" % w if w and force != "tile" else "transpose_generic"
    if force == "rows":
        return "transpose_generic"
    eb = next(e for e, s in dims[:-1] if s == 1)
    vin, vout = eb * es % 4 == 0 and align_in >= 4, dims[-1][0] * es % 4 == 0 and align_out >= 4  # the width of each side
    return "transpose_tile_" + {(1, 1): "4", (1, 0): "4_1", (0, 1): "1_4", (0, 0): "1"}[(int(vin), int(vout))]


# ------------------------------------------------------------------------------------ networks around the four ops
class MoveNet:
    """A small network given as a list of layers over named tensors, run two ways: through the csinn session API in graph
    mode, and as an oracle chain -- convolutions and fullyconnected through the C oracle (cases.oracle_run), everything else
    through the numpy restatements.  cut=True builds THE SAME GRAPH WITHOUT ITS TRANSPOSE / RESHAPE / FLATTEN / PAD LAYERS:
    each one's input becomes a graph output and its output a graph input, so that the fusion planner's counts can be compared
    (that graph is built, never run).

    tensors: name -> (shape, record).  layers: (kind, name, input, output, info) with kind conv (info: act, k, stride, pad,
    depthwise, k_log2), fc, relu, gap, sigmoid, flatten, reshape, pad (info: before, after), transpose (info: perm)."""
    MOVES = ("transpose", "reshape", "flatten", "pad")

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
                                       k=(k, k), stride=(info.get("stride", 1),) * 2, pad=(info.get("pad", k // 2),) * 4,
                                       act=info.get("act", 0), depthwise=info.get("depthwise", False))
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
        rng = np.random.default_rng(900 + k)
        shape = self.shape(self.in_name)
        return rng.integers(-100, 100, shape, dtype=np.int8) if self.dtype == "int8" else rng.standard_normal(shape).astype(np.float16)

    def _move_case(self, kind, src, dst, info, x=None):
        return dict(op=kind, dtype=self.dtype, in_q=self.rec(src), out_q=self.rec(dst), x=x, out_shape=self.shape(dst),
                    perm=info.get("perm"), before=info.get("before"), after=info.get("after"), value=info.get("value", 0.0),
                    layout=self.layout)

    # -- the oracle chain: every named tensor
    def oracle(self, x):
        env = {self.in_name: x}
        form = "ref" if self.dtype == "int8" else "f16"
        for kind, name, src, dst, info in self.layers:
            a = env[src]
            if kind in ("conv", "fc"):
                case = dict(self.cv[name])
                case["input"] = np.ascontiguousarray(a).reshape(case["in_shape"])
                env[dst] = cases.oracle_run(case, form).reshape(self.shape(dst))
            elif kind in self.MOVES:
                env[dst] = move_numpy(self._move_case(kind, src, dst, info, a))
            elif kind == "sigmoid":
                env[dst] = eltwise_cases.eltwise_numpy(dict(op="sigmoid", x=a, dtype=self.dtype, in_q=self.rec(src),
                                                            out_q=self.rec(dst), n=0.0))
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
            return T(shape, self.rec(name), name.encode(), layout=pkg.LAYOUT_NC if len(shape) == 2 else act_l)
        env = {self.in_name: A(self.in_name)}
        ops, inputs, outputs = [], [env[self.in_name]], []
        for kind, name, src, dst, info in self.layers:
            env[dst] = A(dst)
            nm = name.encode()
            if kind in self.MOVES and self.cut:
                outputs.append(env[src])
                inputs.append(env[dst])
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
                stem = "csinn_depthwise_conv2d" if case["depthwise"] else "csinn_conv2d"
                ops.append((stem + ("_relu" if case["act"] else ""), (env[src], env[dst], t_w, t_b, p)))
            elif kind == "fc":
                case = self.cv[name]
                t_w = T((case["co"], case["c"]), None, nm + b"_w", case["kernel"], 1, pkg.LAYOUT_OI, scales=tuple(case["k_scale"]))
                t_b = T((case["co"],), None, nm + b"_b", case["bias"], 1, pkg.LAYOUT_O, pkg.DTYPE_INT32 if int8 else dt,
                        scales=tuple(case["b_scale"]))
                ops.append(("csinn_fullyconnected", (env[src], env[dst], t_w, t_b, pkg.fc_params(fe, keep, api, case["co"], 0, sess, nm))))
            elif kind in self.MOVES:
                p = op_params(fe, keep, api, self._move_case(kind, src, dst, info), sess, layout=act_l)
                ops.append(("csinn_" + kind, (env[src], env[dst], p)))
            else:
                what = {"relu": "relu", "gap": "pool", "sigmoid": "sigmoid"}[kind]
                stem = {"relu": "csinn_relu", "gap": "csinn_global_avgpool2d", "sigmoid": "csinn_sigmoid"}[kind]
                ops.append((stem, (env[src], env[dst], pkg.siso_params(fe, keep, api, what, act_l, 1, sess, nm))))
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


def _act(layout, c, h):
    return (1, h, h, c) if layout == "NHWC" else (1, c, h, h)


def classifier_tail(dtype="int8", layout="NHWC", cut=False, reshape=False, classes=24):
    """8x8x16 -> conv1x1 (32) + a relu LAYER (which a session folds) -> global_avgpool2d -> flatten (or reshape) to [1, 32]
    -> fullyconnected: the tail of a converted ResNet / MobileNet"""
    q = lambda s, z: _q(2.0 ** s, z)
    t = {"data": (_act(layout, 16, 8), q(-4, -5)), "c1c": (_act(layout, 32, 8), q(-3, -100)), "c1": (_act(layout, 32, 8), q(-3, -100)),
         "gap": (_act(layout, 32, 1), q(-5, -128)), "flat": ((1, 32), q(-4, -120)),  # the flatten requantises
         "fc": ((1, classes), q(-3, -11))}
    L = [("conv", "c1", "data", "c1c", dict(act=0)),
         ("relu", "c1_relu", "c1c", "c1", {}),
         ("gap", "gap", "c1", "gap", {}),
         ("reshape" if reshape else "flatten", "flat", "gap", "flat", {}),
         ("fc", "fc", "flat", "fc", dict(k_log2=-8))]
    return MoveNet(dtype, layout, 51, "data", t, L, ["fc"], cut=cut)


def tf_stride2_block(dtype="int8", layout="NHWC", cut=False):
    """8x8x16 -> conv1x1 + a relu LAYER -> pad (0 before, 1 after on H and W: TensorFlow's SAME) -> depthwise 3x3 stride 2
    without padding (4x4) -> conv1x1 + relu (32): a stride-2 block of a TF-exported MobileNet"""
    q = lambda s, z: _q(2.0 ** s, z)
    nhwc = layout == "NHWC"
    t = {"data": (_act(layout, 16, 8), q(-4, -5)), "pwc": (_act(layout, 16, 8), q(-3, -100)), "pw": (_act(layout, 16, 8), q(-3, -100)),
         "padded": (_act(layout, 16, 9), q(-3, -100)), "dw": (_act(layout, 16, 4), q(-3, -10)), "out": (_act(layout, 32, 4), q(-3, -90))}
    hw = dict(before=[0, 0, 0, 0], after=[0, 1, 1, 0] if nhwc else [0, 0, 1, 1], value=0.0)
    L = [("conv", "pw0", "data", "pwc", dict(act=0)),
         ("relu", "pw0_relu", "pwc", "pw", {}),
         ("pad", "pad", "pw", "padded", hw),
         ("conv", "dw", "padded", "dw", dict(k=3, stride=2, pad=0, depthwise=True, k_log2=-5)),
         ("conv", "pw1", "dw", "out", dict(act=1))]
    return MoveNet(dtype, layout, 53, "data", t, L, ["out"], cut=cut)


def detection_head(dtype="int8", layout="NHWC", cut=False):
    """4x4x16 -> conv1x1 + a relu LAYER -> conv1x1 to 24 channels -> reshape to anchors x values -> transpose so that the
    values are innermost -> sigmoid: a YOLO head.  NCHW: [1, 24, 4, 4] -> [1, 3, 8, 4, 4] -> (0, 1, 3, 4, 2); NHWC, the
    equivalent: [1, 4, 4, 24] -> [1, 16, 3, 8] -> (0, 2, 1, 3).  The transposed tensor is a graph output too."""
    q = lambda s, z: _q(2.0 ** s, z)
    nhwc = layout == "NHWC"
    split, perm = ((1, 16, 3, 8), (0, 2, 1, 3)) if nhwc else ((1, 3, 8, 4, 4), (0, 1, 3, 4, 2))
    t = {"data": (_act(layout, 16, 4), q(-4, -5)), "c0c": (_act(layout, 16, 4), q(-3, -100)), "c0": (_act(layout, 16, 4), q(-3, -100)),
         "head": (_act(layout, 24, 4), q(-4, 3)), "split": (split, q(-4, 3)),
         "moved": (tuple(split[p] for p in perm), q(-3, 10)),  # the transpose requantises
         "prob": (tuple(split[p] for p in perm), _q(1.0 / 256, -128))}
    L = [("conv", "c0", "data", "c0c", dict(act=0)),
         ("relu", "c0_relu", "c0c", "c0", {}),
         ("conv", "head", "c0", "head", dict(act=0, k_log2=-6)),
         ("reshape", "split", "head", "split", {}),
         ("transpose", "moved", "split", "moved", dict(perm=perm)),
         ("sigmoid", "prob", "moved", "prob", {})]
    return MoveNet(dtype, layout, 57, "data", t, L, ["prob", "moved"], cut=cut)


NETS = {"classifier_flatten": lambda d, l, **kw: classifier_tail(d, l, **kw),
        "classifier_reshape": lambda d, l, **kw: classifier_tail(d, l, reshape=True, **kw),
        "tf_stride2": lambda d, l, **kw: tf_stride2_block(d, l, **kw),
        "detection_head": lambda d, l, **kw: detection_head(d, l, **kw)}
CUT_LAYERS = {"classifier_flatten": 1, "classifier_reshape": 1, "tf_stride2": 1, "detection_head": 2}

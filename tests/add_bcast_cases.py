"""Shared helpers for the broadcasting add (CSINN_OP_ADD with operands of different shapes).

  add_cases()               deterministic single-op problems: every pair of int8 operands with b broadcast along rows, every
                            binary16 pattern plus a broadcast scalar, every pair of the binary16 specials (NaNs and infinities
                            of both signs in either position), the bias shapes of a linear layer, the smallest shapes at which
                            each kernel form (add_vec, add_row, add_generic) can still go wrong, either operand order, a
                            constant operand second and first, one case per dtype with more than one workgroup
  add_numpy(case)           plain numpy restatement of the reference (source/reference/add.c:21-41 inside
                            shl_ref_diso_callback_base, the broadcast of shl_ref_broadcast_to_shape): dequantise, broadcast,
                            one float32 sum, requantise
  add_run(fe, api, case)    csinn_add_init + csinn_add through a front-end (layer mode), host or DMABUF tensors
  add_desc(case)            the case's struct shl_mi355x_mul_desc (the descriptor is mul's)
The genuine library's outputs for add_cases() live in tests/golden/add_bcast_cases.npz (make_add_bcast_golden.py).
A case is a dict with mul's keys (eltwise_cases): x has the output's shape, y is broadcast to it; small_first: y is the
layer's FIRST input; b_const: y is a constant tensor.
"""
import os

import numpy as np

import eltwise_cases
import pool_cases
from cases import pkg
from eltwise_cases import F16_SCALARS, RECORD_TRIPLES, _data, _nan_like, _rng
from pool_cases import Q_F16, assert_same, bits  # noqa: F401

# binary16 values whose sums need care: quiet and signalling NaNs of both signs, both infinities, the largest finite
# values (their sum saturates), signed zeros, subnormals.  Sixteen of them: one 16-byte piece times two
F16_SPECIALS = (0x7E00, 0xFE00, 0x7C01, 0xFFFF, 0x7C00, 0xFC00, 0x7BFF, 0xFBFF, 0x0000, 0x8000, 0x0001, 0x8001, 0x3C00, 0xBC00,
                0x3555, 0x7BFE)


def add_cases():
    out = []

    def add(name, dtype, a_shape, b_shape, q=None, layout="NHWC", small_first=False, b_const=False, x=None, y=None):
        """x has a_shape (the output's), y has b_shape; small_first: y is given as the FIRST input"""
        rng = _rng(name)
        x = _data(rng, dtype, a_shape) if x is None else x
        y = _data(rng, dtype, b_shape) if y is None else y
        qa, qb, qo = q if dtype == "int8" else (Q_F16[0],) * 3
        out.append(dict(name=name, op="add", dtype=dtype, x=np.ascontiguousarray(x), y=np.ascontiguousarray(y), in_q=qa, in1_q=qb,
                        out_q=qo, layout=layout, small_first=small_first, b_const=b_const))

    every = np.arange(-128, 128, dtype=np.int16).astype(np.int8)
    patterns = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    # ---- int8: the 256 x 256 grid of all operand pairs, b broadcast along the rows ---------------------------------------
    for key, q in RECORD_TRIPLES.items():
        add("add_i8_grid_" + key, "int8", (256, 256), (256,), q, layout="NC", x=np.repeat(every, 256).reshape(256, 256), y=every)
    # ---- binary16: all patterns plus a broadcast scalar; every pair of the specials, in either operand position ----------
    for key, h in F16_SCALARS.items():
        add("add_f16_all_by_" + key, "f16", (65536,), (1,), layout="N", x=patterns, y=np.array([h], np.uint16).view(np.float16))
    specials = np.array(F16_SPECIALS, np.uint16).view(np.float16)
    for first in (False, True):
        add("add_f16_specials" + ("_small_first" if first else ""), "f16", (16, 16), (16,), layout="NC", small_first=first,
            x=np.repeat(specials, 16).reshape(16, 16), y=specials)
    # ---- geometry, both dtypes ------------------------------------------------------------------------------------------
    conv = RECORD_TRIPLES["conv"]
    for dtype in ("int8", "f16"):
        d = "i8" if dtype == "int8" else "f16"
        # the bias of a linear layer, a positional embedding, an attention bias
        add("add_%s_bias_n16" % d, dtype, (2, 3, 5, 16), (16,), conv)                        # vec
        add("add_%s_bias_n20" % d, dtype, (2, 3, 5, 20), (20,), conv)                        # generic: 20 % 16, 20 % 8
        add("add_%s_bias_2x17x64" % d, dtype, (2, 17, 64), (64,), conv, layout="N")
        add("add_%s_posemb_2x17x64" % d, dtype, (2, 17, 64), (1, 17, 64), conv, layout="N")
        add("add_%s_attn_bias_2x2x17x17" % d, dtype, (2, 2, 17, 17), (1, 2, 17, 17), conv, layout="NCHW")  # 17 17 is odd: pieces straddle
        # the other patterns
        add("add_%s_nhwc_gate_c16" % d, dtype, (2, 3, 5, 16), (2, 1, 1, 16), conv)           # vec, b along N and C
        add("add_%s_scalar" % d, dtype, (2, 3, 5, 16), (1,), conv)                           # vec, scalar
        add("add_%s_scalar_tail" % d, dtype, (3, 7, 5), (1,), conv, layout="N")              # 105 elements: pieces + tail
        add("add_%s_nchw_channels" % d, dtype, (2, 3, 4, 5), (1, 3, 1, 1), conv, layout="NCHW")  # row
        add("add_%s_nchw_gate" % d, dtype, (2, 3, 4, 5), (2, 3, 1, 1), conv, layout="NCHW")
        for hw in ((1, 1), (2, 2), (1, 37)):                                                 # row-form tails: H W = 1, 4, 37
            add("add_%s_nchw_hw%d" % (d, hw[0] * hw[1]), dtype, (2, 3) + hw, (2, 3, 1, 1), conv, layout="NCHW")
        add("add_%s_nchw_middle" % d, dtype, (2, 3, 4, 5), (1, 1, 4, 1), conv, layout="NCHW")  # row: b varies along H only
        # the broadcast operand first; a constant operand second and first
        add("add_%s_small_first_nhwc" % d, dtype, (2, 3, 5, 16), (16,), conv, small_first=True)
        add("add_%s_small_first_nchw" % d, dtype, (2, 3, 4, 5), (1, 3, 1, 1), conv, layout="NCHW", small_first=True)
        add("add_%s_const_bias" % d, dtype, (2, 3, 5, 16), (16,), conv, b_const=True)
        add("add_%s_const_nchw" % d, dtype, (2, 3, 4, 5), (1, 3, 1, 1), conv, layout="NCHW", b_const=True)
        add("add_%s_const_first_bias" % d, dtype, (2, 3, 5, 16), (16,), conv, small_first=True, b_const=True)
        add("add_%s_const_first_nchw" % d, dtype, (2, 3, 4, 5), (1, 3, 1, 1), conv, layout="NCHW", small_first=True, b_const=True)

    # ---- more than one workgroup (a block of 4 096 random values over and over: the golden file stays small) --------------
    def tiled(dtype, shape):
        block = _data(_rng("big " + dtype), dtype, (4096,))
        return np.resize(block, int(np.prod(shape))).reshape(shape)
    add("add_i8_2x56x56x64_bias", "int8", (2, 56, 56, 64), (64,), RECORD_TRIPLES["pow2"], x=tiled("int8", (2, 56, 56, 64)))
    add("add_f16_2x64x28x28_channels", "f16", (2, 64, 28, 28), (1, 64, 1, 1), layout="NCHW", x=tiled("f16", (2, 64, 28, 28)))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


# ------------------------------------------------------------------------------------ numpy restatement
def add_f32(a, b):
    """one float32 sum of the layer's first input a and second input b.  NaNs as the reference's x86 build hands them on: an
    operand's NaN keeps its sign (the SECOND input's when both are NaNs: add.c:23 compiles to src1 + src0, as mul.c:23 does;
    the genuine library's outputs on every pair of specials decide), inf + -inf gives the default NaN, whose sign bit is set"""
    with np.errstate(all="ignore"):
        r = (a + b).astype(np.float32)
    made = np.isnan(r) & ~np.isnan(a) & ~np.isnan(b)
    r = np.where(np.isnan(b), _nan_like(b), np.where(np.isnan(a), _nan_like(a), r))
    return np.where(made, np.float32(np.uint32(0xFFC00000).view(np.float32)), r)


def add_numpy(case):
    dt = case["dtype"]
    x = pool_cases.dequantise(case["x"], dt, case["in_q"])
    y = np.broadcast_to(pool_cases.dequantise(case["y"], dt, case["in1_q"]), x.shape)
    r = add_f32(y, x) if case.get("small_first") else add_f32(x, y)
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(pool_cases.requantise(r, dt, case["out_q"])).reshape(case["x"].shape)


def golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "add_bcast_cases.npz")
    blob = np.load(path)
    return {k: blob[k] for k in blob.files}


add_desc = eltwise_cases.mul_desc  # (the case's keys are mul's, and so is the descriptor)


# ------------------------------------------------------------------------------------ through csinn_add
def add_run(fe, api, case, device=None, poison=None, in_skew=0, **override):
    """layer mode through csinn_add_init + csinn_add.  device: a cases.HipDevice -- every non-constant tensor then lives in HBM
    as a DMABUF tensor, the full operand `in_skew` ELEMENTS into its allocation.  override: out_shape / out_dtype / in1_dtype /
    scales / out_q for the refusal tests.  Returns the output, or (status, output buffer) when `poison` (a byte the output is
    pre-filled with) is given."""
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, api, keep)
    np_dt = {"int8": np.int8, "f16": np.float16}
    code = {"int8": pkg.DTYPE_INT8, "f16": pkg.DTYPE_FLOAT16}
    dt = case["dtype"]
    layout = eltwise_cases._LAYOUTS[case["layout"]]
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
    y = case["y"] if "in1_dtype" not in override else case["y"].astype(np_dt[override["in1_dtype"]])
    t_y, _ = tensor(y, case["in1_q"], b"in1", dtype=override.get("in1_dtype", dt), const=1 if case["b_const"] else 0)
    params = pkg.siso_params(fe, keep, api, "add", layout, 1, sess, b"add")
    args = (t_y, t_x, t_out, params) if case["small_first"] else (t_x, t_y, t_out, params)
    rc = fe.csinn_add_init(*args)
    if rc == pkg.CSINN_TRUE:
        rc = fe.csinn_add(*args)
    if dev_out is not None:
        out = device.download(dev_out, out.shape, out.dtype)
    for p in allocs:
        device.free(p)
    if poison is not None:
        return rc, out
    if rc != pkg.CSINN_TRUE:
        raise pkg.MI355XError("csinn_add returned %d" % rc)
    return out

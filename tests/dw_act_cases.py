"""Cases of an int8 table activation folded into the DEPTHWISE launch -- depthwise conv2d [+ folded relu / relu6] -> sigmoid |
hard_sigmoid | silu | leaky_relu, or the gate of a swish / hard-swish (shl_mi355x_dwconv_lut_forward) -- on each of the three
kernels that carry the post-op, with the oracle chain and the two ways to run them on the device, and the small networks of the
session tests.  Tables, their builders and the oracle's side of them are act_fuse_cases.py's.

  all_cases()       (shape, table) pairs for the dot4 kernel (3x3, the default at these sizes) and the generic kernel (any
                    other kernel size): the smallest shapes at which each can still go wrong
  child_cases()     the matrix-core kernel: `python dw_act_cases.py` runs them under SHL_MI355X_DWMFMA=1 (the switch is read
                    once per process)
  mbv3_block(), effnet_block() and the nets that must NOT fuse
"""
import os
import sys

import numpy as np

import act_fuse_cases as ac
import cases
import residual_cases as rc
from act_fuse_cases import ActNet, q
from cases import pkg

POISON, GUARD = ac.POISON, ac.GUARD
DW = dict(depthwise=True)
# name -> (kernel, make_case arguments, seed, output zero point or None for make_case's)
SHAPES = {
    # ---- dot4: blockIdx.x = output row, 256 lanes of (pixel, channel group) per block in y
    "dot4_c4_3x5": ("dot4", dict(DW, h=3, w=5, c=4), 1, None),                       # one partial wave, 5 busy lanes
    "dot4_c8_9x9_s2_asym": ("dot4", dict(DW, h=9, w=9, c=8, stride=(2, 2), pad=(0, 1, 1, 2)), 2, None),
    "dot4_c32_2x33": ("dot4", dict(DW, h=2, w=33, c=32), 3, None),                   # 264 per row: a second block with 8 busy lanes
    "dot4_dilation2": ("dot4", dict(DW, h=7, w=7, c=8, dilation=(2, 2), pad=(2, 2, 2, 2)), 4, None),
    "dot4_batch2": ("dot4", dict(DW, n=2, h=4, w=6, c=12), 5, None),
    "dot4_relu6": ("dot4", dict(DW, h=5, w=7, c=16, act=2), 6, None),                # the convolution folds its own relu6
    "dot4_converter_scales": ("dot4", dict(DW, h=5, w=7, c=16, exact=False), 7, None),
    "dot4_out_zp_min": ("dot4", dict(DW, h=5, w=7, c=8, exact=False), 8, -128),
    "dot4_out_zp_max": ("dot4", dict(DW, h=5, w=7, c=8), 9, 127),
    # ---- generic: any kernel size, grid-stride loop
    "nhwc_5x5_7x7": ("nhwc", dict(DW, h=7, w=7, c=8, k=(5, 5), pad=(2, 2, 2, 2)), 10, None),
    "nhwc_5x5_s2_9x11": ("nhwc", dict(DW, h=9, w=11, c=12, k=(5, 5), stride=(2, 2), pad=(2, 2, 2, 2), exact=False), 11, None),
    "nhwc_3x5": ("nhwc", dict(DW, h=6, w=7, c=8, k=(3, 5), pad=(1, 2, 1, 2), act=1), 12, None),
    "nhwc_batch2": ("nhwc", dict(DW, n=2, h=5, w=5, c=16, k=(5, 5), pad=(2, 2, 2, 2)), 13, None),
}
# ---- mfma: workgroups of 8 x 4 pixel tiles by min(C, 128) channels, waves of 32 channels
CHILD_SHAPES = {
    "mfma_c32_5x7": ("mfma", dict(DW, h=5, w=7, c=32), 20, None),                    # one ragged tile
    "mfma_c64_9x9_s2": ("mfma", dict(DW, h=9, w=9, c=64, stride=(2, 2), exact=False), 21, None),
    "mfma_c96_6x10": ("mfma", dict(DW, h=6, w=10, c=96, act=2), 22, None),           # three channel blocks of 32
    "mfma_c128_9x17": ("mfma", dict(DW, h=9, w=17, c=128), 23, None),                # two tiles in x, ragged in both directions
    "mfma_batch2": ("mfma", dict(DW, n=2, h=5, w=9, c=32), 24, 127),
}
FULL_TABLE_SHAPES = ("dot4_c32_2x33", "nhwc_5x5_s2_9x11", "mfma_c128_9x17")  # every table of act_fuse_cases.TABLES, one shape per kernel
KERNEL_NAME = {"dot4": "dwconv_dot4+lut", "nhwc": "dwconv_nhwc+lut", "mfma": "dwconv_mfma+lut"}


def conv_of(shape):
    """the shape's depthwise problem, made once -- and made known to act_fuse_cases, whose tables take the convolution's output
    record from its own list of problems"""
    if shape not in ac._CONVS:
        kernel, kw, seed, out_zp = SHAPES.get(shape) or CHILD_SHAPES[shape]
        c = cases.make_case(9400 + seed, **kw)
        if out_zp is not None:
            c["out_zp"] = out_zp
        ac._CONVS[shape] = c
    return ac._CONVS[shape]


def _case(shape, table):
    return dict(name=shape + "-" + table, shape=shape, kernel=(SHAPES.get(shape) or CHILD_SHAPES[shape])[0], table=table)


def _cases_of(shapes):
    out = []
    acts = ("silu", "gate", "leaky_relu", "sigmoid", "hard_sigmoid", "silu_zp_min", "leaky_zp_max")
    i = 0
    for shape in shapes:
        if shape in FULL_TABLE_SHAPES:
            out += [_case(shape, t) for t in ac.TABLES]
        else:  # the table that tells every byte and every byte lane apart, and one activation or the gate
            out += [_case(shape, "permutation"), _case(shape, acts[i % len(acts)])]
            i += 1
    return out


def all_cases():
    return _cases_of(SHAPES)


def child_cases():
    return _cases_of(CHILD_SHAPES)


_ORACLE = {}


def oracle_chain(case):
    """conv (oracle formulation X, once per shape), then the reference's layers on the stored bytes"""
    if case["shape"] not in _ORACLE:
        conv = cases.oracle_run(conv_of(case["shape"]), "exact")
        conv.setflags(write=False)
        _ORACLE[case["shape"]] = conv
    conv = _ORACLE[case["shape"]]
    return ac.oracle_table(case)[conv.astype(np.int16) + 128]


def run_both(hip, opt, dev, case):
    """(fused output, unfused output, the guard bytes around the fused output, the fused launch's kernel name), on one set of
    buffers: the fused launch into a poisoned output with guard bands, then conv_forward, then unary_lut_i8"""
    c = conv_of(case["shape"])
    n = int(np.prod(c["out_shape"]))
    plan = rc.make_plan(hip, c)
    table = ac.device_table(opt, case)
    d_in, d_conv, d_un, d_guarded = dev.alloc(c["input"].nbytes), dev.alloc(n), dev.alloc(n), dev.alloc(n + 2 * GUARD)
    try:
        dev.upload(d_in, c["input"])
        dev.upload(d_guarded, np.full(n + 2 * GUARD, POISON, np.uint8))
        name = hip.shl_mi355x_dwconv_lut_kernel_name(plan, 0).decode()
        pkg.check(hip.shl_mi355x_dwconv_lut_forward(plan, d_in, d_guarded + GUARD, 0, table.ctypes.data, None), hip, "dwconv_lut_forward")
        pkg.check(hip.shl_mi355x_conv_forward(plan, d_in, d_conv, 0, None), hip, "conv_forward")
        pkg.check(hip.shl_mi355x_unary_lut_i8(d_conv, d_un, n, table.ctypes.data, None), hip, "unary_lut_i8")
        unfused = dev.download(d_un, c["out_shape"], np.int8)
        whole = dev.download(d_guarded, (n + 2 * GUARD,), np.uint8)
        fused = whole[GUARD:GUARD + n].view(np.int8).reshape(c["out_shape"])
        return fused, unfused, np.concatenate([whole[:GUARD], whole[GUARD + n:]]), name
    finally:
        for p in (d_in, d_conv, d_un, d_guarded):
            dev.free(p)
        hip.shl_mi355x_conv_plan_destroy(plan)


def check_case(hip, opt, dev, case):
    want = oracle_chain(case)
    fused, unfused, guards, name = run_both(hip, opt, dev, case)
    assert name == KERNEL_NAME[case["kernel"]], (case["name"], name)
    assert (guards == POISON).all(), case["name"] + ": the fused launch wrote outside its output"
    for what, got in (("unfused", unfused), ("fused", fused)):
        bad, worst = cases.mismatch_report(got, want)
        assert bad == 0, "%s: %s differs from the oracle chain on %d of %d outputs (max %d)" % (case["name"], what, bad, got.size, worst)
    assert np.array_equal(fused, unfused)


# ------------------------------------------------------------------------------------------ networks
DWK = dict(depthwise=True, k_log2=-5)


def mbv3_block():
    """MobileNetV3: 1x1 expand -> hard_sigmoid -> mul -> depthwise 3x3 -> hard_sigmoid -> mul(gate, dw) -> 1x1 project -> add(skip)"""
    t = {"x": (16, 8, q(-4, -5)), "e": (48, 8, q(-4, 7)), "g1": (48, 8, q(-8, -128)), "h1": (48, 8, q(-4, -100)), "d": (48, 8, q(-3, -20)),
         "g2": (48, 8, q(-8, -128)), "h2": (48, 8, q(-3, -90)), "p": (16, 8, q(-4, 9)), "out": (16, 8, q(-3, -7))}
    L = [("conv", "expand", ["x"], ["e"], {}), ("hard_sigmoid", "hsig1", ["e"], ["g1"], {}), ("mul", "hswish1", ["e", "g1"], ["h1"], {}),
         ("conv", "dw", ["h1"], ["d"], dict(DWK, k=3)), ("hard_sigmoid", "hsig2", ["d"], ["g2"], {}), ("mul", "hswish2", ["g2", "d"], ["h2"], {}),
         ("conv", "project", ["h2"], ["p"], {}), ("add", "add", ["p", "x"], ["out"], {})]
    return ActNet("int8", "NHWC", 81, "x", t, L, ["out"])


def effnet_block():
    """EfficientNet: 1x1 -> silu -> depthwise 5x5 stride 2 -> silu -> 1x1"""
    t = {"x": (16, 9, q(-4, -5)), "e": (32, 9, q(-3, 3)), "a1": (32, 9, q(-4, -90)), "d": (32, 5, q(-2, -9)), "a2": (32, 5, q(-3, -100)),
         "out": (24, 5, q(-3, 11))}
    L = [("conv", "expand", ["x"], ["e"], {}), ("silu", "silu1", ["e"], ["a1"], {}), ("conv", "dw", ["a1"], ["d"], dict(DWK, k=5, stride=2)),
         ("silu", "silu2", ["d"], ["a2"], {}), ("conv", "project", ["a2"], ["out"], {})]
    return ActNet("int8", "NHWC", 82, "x", t, L, ["out"])


def exported_dw():
    """depthwise -> silu, the depthwise output a graph output too"""
    t = {"x": (16, 8, q(-4, -5)), "d": (16, 8, q(-2, 3)), "out": (16, 8, q(-3, -90))}
    L = [("conv", "dw", ["x"], ["d"], dict(DWK, k=3)), ("silu", "silu", ["d"], ["out"], {})]
    return ActNet("int8", "NHWC", 83, "x", t, L, ["out", "d"])


def third_reader_dw():
    """depthwise -> hard_sigmoid -> mul(dw, gate), and a relu that reads the depthwise output as well"""
    t = {"x": (16, 8, q(-4, -5)), "d": (16, 8, q(-2, 7)), "g": (16, 8, q(-8, -128)), "out": (16, 8, q(-2, -100)), "r": (16, 8, q(-2, -128))}
    L = [("conv", "dw", ["x"], ["d"], dict(DWK, k=3)), ("hard_sigmoid", "hsig", ["d"], ["g"], {}), ("mul", "hswish", ["d", "g"], ["out"], {}),
         ("relu", "relu", ["d"], ["r"], {})]
    return ActNet("int8", "NHWC", 84, "x", t, L, ["out", "r"])


def broadcast_gate_dw():
    """a squeeze-and-excite gate behind the depthwise layer: dw -> global_avgpool -> hard_sigmoid -> mul(dw, gate [1, 1, 1, C])"""
    t = {"x": (16, 8, q(-4, -5)), "d": (16, 8, q(-2, 7)), "s": (16, 1, q(-3, 0)), "g": (16, 1, q(-8, -128)), "out": (16, 8, q(-2, -100))}
    L = [("conv", "dw", ["x"], ["d"], dict(DWK, k=3)), ("gap", "squeeze", ["d"], ["s"], {}), ("hard_sigmoid", "hsig", ["s"], ["g"], {}),
         ("mul", "excite", ["d", "g"], ["out"], {})]
    return ActNet("int8", "NHWC", 85, "x", t, L, ["out"])


def paired_dw():
    """1x1 (relu6 folded) -> depthwise 3x3 -> silu: the depthwise layer is the second half of the pw -> dw pair, which comes first"""
    t = {"x": (32, 14, q(-4, -5)), "e": (32, 14, q(-5, -128)), "d": (32, 14, q(-2, 3)), "out": (32, 14, q(-3, -90))}
    L = [("conv", "expand", ["x"], ["e"], dict(act=2)), ("conv", "dw", ["e"], ["d"], dict(DWK, k=3)), ("silu", "silu", ["d"], ["out"], {})]
    return ActNet("int8", "NHWC", 86, "x", t, L, ["out"])


# name -> (net, fused activations under SHL_MI355X_ACT_FUSE=1, of which on implicit-GEMM steps alone)
FUSING = {"mbv3_block": (mbv3_block, 2, 1), "effnet_block": (effnet_block, 2, 1)}
APART = {"exported_dw": exported_dw, "third_reader_dw": third_reader_dw, "broadcast_gate_dw": broadcast_gate_dw}


if __name__ == "__main__":  # the child of tests/test_dw_act_fuse.py: the matrix-core kernel, chosen through the environment
    assert os.environ.get("SHL_MI355X_DWMFMA") == "1"
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    device = cases.HipDevice(hip)
    for cs in child_cases():
        check_case(hip, opt, device, cs)
        print("ok", cs["name"])
    print("child ok", len(child_cases()))
    sys.exit(0)

"""Cases of the fused residual tail -- conv2d [+ folded activation] -> add(conv_out, skip) -> [relu | relu6] in the convolution's
launch (shl_mi355x_conv_add_forward) -- with the oracle chain and the two ways to run them on the device.

Shapes are the smallest at which each store path of the two carrying kernel families can go wrong (M = N Ho Wo):
  wave   ragged pixel and channel tiles with dword stores, the element-store path (Co % 4 != 0), the split-K tail (K rows of
         256 bytes on few tiles), 3x3 at stride 1 and 2
  tile   the second ragged tile of the 128 x 128 flavour through the staged stores (Co % 16 == 0) and through the element
         stores, 256 x 64; 256 x 128 and 256 x 256 and the flavours without producer waves in a child process (the switches
         are read once per process): `python residual_cases.py` runs child_cases() under the caller's environment
Records vary per case: the convolution's byte as either operand, no activation / relu / relu6, a convolution with its own
folded relu6, converter scales, zero points -128 / 0 / 127, a sum scale outside the range of the multiply-and-correct division
(add_rec gives fma_div == 0 there, 1 everywhere else), skip tensors of all -128 and all 127.
"""
import ctypes as C
import os
import sys

import numpy as np

import cases
import tail
from cases import pkg

POISON = 0x5A
GUARD = 256


def _case(name, form, conv, conv_first=1, act=0, skip_q=(2.0 ** -4, 3), sum_q=(2.0 ** -3, -7), out_q=(2.0 ** -3, 5), skip_fill=None,
          seed=0, rel=False):
    """rel: the skip's and the sum's scales are given in units of the convolution's output scale"""
    c = cases.make_case(9100 + seed, **conv)
    if rel:
        skip_q, sum_q = (skip_q[0] * c["out_scale"], skip_q[1]), (sum_q[0] * c["out_scale"], sum_q[1])
    rng = np.random.default_rng(9200 + seed)
    skip = rng.integers(-128, 128, c["out_shape"], dtype=np.int8)
    if skip_fill is not None:
        skip[...] = skip_fill
    return dict(name=name, form=form, conv=c, conv_first=conv_first, act=act, skip_q=(float(np.float32(skip_q[0])), skip_q[1]),
                sum_q=(float(np.float32(sum_q[0])), sum_q[1]), out_q=(float(np.float32(out_q[0])), out_q[1]), skip=skip)


PW = dict(k=(1, 1), pad=(0, 0, 0, 0))


def all_cases():
    out = []
    # ---- wave
    out.append(_case("wave_1x1_m33_co36", "wave", dict(PW, h=3, w=11, c=16, co=36), conv_first=1, act=1, seed=1))
    out.append(_case("wave_1x1_m33_co30_elements", "wave", dict(PW, h=3, w=11, c=16, co=30, exact=False), conv_first=0, act=0,
                     skip_q=(0.0437, -128), sum_q=(0.0713, 127), seed=2))
    out.append(_case("wave_1x1_c256_splitk", "wave", dict(PW, h=8, w=8, c=256, co=32, act=2), conv_first=0, act=2,
                     skip_q=(0.0291, 127), sum_q=(0.0517, 0), out_q=(0.0333, -128), seed=3))
    out.append(_case("wave_3x3_5x7", "wave", dict(h=5, w=7, c=16, co=32, exact=False), conv_first=1, act=2,
                     skip_q=(0.0611, 0), sum_q=(0.0939, -128), out_q=(0.0471, -20), seed=4))
    # (an activation's output under zero point 127 saturates wherever the sum is positive: the record is legal, the output flat)
    out.append(_case("wave_out_zp_127", "wave", dict(PW, h=3, w=11, c=16, co=36), conv_first=1, act=1, sum_q=(0.0939, 0),
                     out_q=(0.0471, 127), seed=14))
    out.append(_case("wave_3x3_s2_9x9", "wave", dict(h=9, w=9, c=16, co=32, stride=(2, 2)), conv_first=0, act=1,
                     sum_q=(2.0 ** 41, 9), out_q=(2.0 ** -3, 11), seed=5))  # add_rec: fma_div == 0
    # (a skip tensor at one end of its range under the convolution's own scale: half of the sums saturate, the others spread)
    out.append(_case("wave_skip_all_min", "wave", dict(PW, h=3, w=11, c=16, co=36), act=0, skip_q=(1.0, 0), sum_q=(1.0, 0),
                     skip_fill=-128, seed=6, rel=True))
    out.append(_case("wave_skip_all_max", "wave", dict(PW, h=3, w=11, c=16, co=36), conv_first=0, act=1, skip_q=(1.0, 0),
                     sum_q=(1.0, 0), out_q=(0.09, -100), skip_fill=127, seed=7, rel=True))
    # ---- tile
    out.append(_case("tile_m129_co144_staged", "tile", dict(PW, h=3, w=43, c=64, co=144, exact=False), conv_first=1, act=1,
                     skip_q=(0.0437, 127), sum_q=(0.0713, -128), out_q=(0.0519, 0), seed=8))
    out.append(_case("tile_m129_co130_elements", "tile", dict(PW, h=3, w=43, c=16, co=130), conv_first=0, act=2, seed=9))
    out.append(_case("tile_m257_co64_256x64", "tile", dict(PW, h=1, w=257, c=64, co=64, act=2), conv_first=1, act=0,
                     skip_q=(0.0377, -128), sum_q=(0.0893, -128), seed=10))
    out.append(_case("tile_3x3_m130_co32", "tile", dict(h=10, w=13, c=16, co=32), conv_first=0, act=1, seed=11))
    out.append(_case("tile_skip_all_min", "tile", dict(PW, h=3, w=43, c=64, co=144), act=0, skip_q=(1.0, 0), sum_q=(1.0, 0),
                     skip_fill=-128, seed=12, rel=True))
    out.append(_case("tile_skip_all_max", "tile", dict(PW, h=3, w=43, c=64, co=144), conv_first=0, act=2, skip_q=(1.0, 0), sum_q=(1.0, 0),
                     out_q=(0.05, -128), skip_fill=127, seed=13, rel=True))
    return out


def child_cases():
    """the large tile flavours need uniform-tap addressing (C % 64 == 0); one ragged tile in each direction"""
    return [_case("tile_m257_co144_c64", "tile", dict(PW, h=1, w=257, c=64, co=144, exact=False), conv_first=1, act=2,
                  skip_q=(0.0437, 5), sum_q=(0.0713, -9), out_q=(0.0519, -128), seed=20),
            _case("tile_m257_co272_c64", "tile", dict(PW, h=1, w=257, c=64, co=272), conv_first=0, act=1, seed=21),
            _case("tile_3x3_m260_co130_c64", "tile", dict(h=10, w=26, c=64, co=130), conv_first=1, act=0, seed=22)]


# (environment of the child, what it is for)
CHILD_ENVS = [dict(SHL_MI355X_TILE="256x128"), dict(SHL_MI355X_TILE="256x128", SHL_MI355X_PIPE="6"), dict(SHL_MI355X_TILE="256x256"),
              dict(SHL_MI355X_TILE="128", SHL_MI355X_PIPE="0"), dict(SHL_MI355X_TILE="128", SHL_MI355X_PIPE="4"),
              dict(SHL_MI355X_TILE="256x64", SHL_MI355X_PIPE="4")]


def flat_by_record(case):
    """records that map (nearly) every sum to one byte, so that the expected output cannot spread"""
    return case["sum_q"][0] > 1e6 or (case["act"] != 0 and case["out_q"][1] == 127)


def fma_div_of(case):
    """csrc/add_step.h:add_rec restated: the multiply-and-correct division is exact for a sum scale in [2^-40, 2^40]"""
    return int(2.0 ** -40 <= case["sum_q"][0] <= 2.0 ** 40)


# ------------------------------------------------------------------------------------------ the oracle chain
def oracle_chain(case):
    """conv (oracle formulation X: what the device computes bit for bit in both scale regimes), then the reference's add and
    relu on the stored bytes"""
    c = case["conv"]
    conv = cases.oracle_run(c, "exact")
    conv_q, skip = (float(np.float32(c["out_scale"])), c["out_zp"]), case["skip"]
    a, b, qa, qb = (conv, skip, conv_q, case["skip_q"]) if case["conv_first"] else (skip, conv, case["skip_q"], conv_q)
    total = tail.siso_oracle(dict(kind="add", dtype="int8", x=a, y=b, in_q=qa, in1_q=qb, out_q=case["sum_q"]))
    if case["act"]:
        total = tail.siso_oracle(dict(kind="relu6" if case["act"] == 2 else "relu", dtype="int8", x=total, in_q=case["sum_q"],
                                      out_q=case["out_q"]))
    return dict(conv=conv, out=total)


# ------------------------------------------------------------------------------------------ the device
def conv_desc(c):
    d = pkg.ConvDesc()
    d.layout = pkg.SHL_NHWC if c["layout"] == cases.NHWC else pkg.SHL_NCHW
    d.dtype = pkg.SHL_I8 if c["dtype"] == "int8" else pkg.SHL_F16
    d.act, d.algo = c["act"], pkg.ALGO_AUTO
    d.batch, d.in_h, d.in_w, d.in_c = c["n"], c["h"], c["w"], c["c"]
    d.out_h, d.out_w, d.out_c = c["ho"], c["wo"], c["co"]
    d.kernel_h, d.kernel_w = c["kh"], c["kw"]
    d.stride_h, d.stride_w = c["stride"]
    d.pad_top, d.pad_left = c["pad"][0], c["pad"][1]
    d.dilation_h, d.dilation_w = c["dilation"]
    d.group = c["group"]
    d.in_zp, d.out_zp, d.out_scale = c["in_zp"], c["out_zp"], c["out_scale"]
    return d


def make_plan(hip, c):
    mult = (np.float32(c["in_scale"]) * np.broadcast_to(c["k_scale"], (c["co"],))).astype(np.float32)
    bias = (c["bias"].astype(np.float32) * np.broadcast_to(c["b_scale"], (c["co"],))).astype(np.float32)
    ker = np.ascontiguousarray(c["kernel"])
    plan = C.c_void_p()
    pkg.check(hip.shl_mi355x_conv_plan_create(C.byref(conv_desc(c)), ker.ctypes.data, mult.ctypes.data, bias.ctypes.data, None,
                                              C.byref(plan)), hip, "conv_plan_create")
    return plan


def residual_desc(case):
    d = pkg.ResidualDesc()
    d.conv_first, d.act = case["conv_first"], case["act"]
    d.skip_scale, d.skip_zp = case["skip_q"]
    d.sum_scale, d.sum_zp = case["sum_q"]
    d.out_scale, d.out_zp = case["out_q"]
    return d


def run_both(hip, dev, case):
    """(fused output, unfused output, the guard bytes around the fused output, the fused launch's kernel name)"""
    c = case["conv"]
    n = int(np.prod(c["out_shape"]))
    plan = make_plan(hip, c)
    d_in, d_skip, d_conv, d_sum, d_un = (dev.alloc(c["input"].nbytes), dev.alloc(n), dev.alloc(n), dev.alloc(n), dev.alloc(n))
    d_guarded = dev.alloc(n + 2 * GUARD)
    try:
        dev.upload(d_in, c["input"])
        dev.upload(d_skip, case["skip"])
        dev.upload(d_guarded, np.full(n + 2 * GUARD, POISON, np.uint8))
        d_out = d_guarded + GUARD
        name = hip.shl_mi355x_conv_add_kernel_name(plan, 0).decode()
        pkg.check(hip.shl_mi355x_conv_add_forward(plan, d_in, d_skip, d_out, 0, C.byref(residual_desc(case)), None), hip, "conv_add_forward")
        # the layers one by one
        pkg.check(hip.shl_mi355x_conv_forward(plan, d_in, d_conv, 0, None), hip, "conv_forward")
        (sa, za), (sb, zb) = (float(np.float32(c["out_scale"])), c["out_zp"]), case["skip_q"]
        a, b = (d_conv, d_skip) if case["conv_first"] else (d_skip, d_conv)
        if not case["conv_first"]:
            (sa, za), (sb, zb) = (sb, zb), (sa, za)
        pkg.check(hip.shl_mi355x_add(a, b, d_sum, n, pkg.SHL_I8, sa, za, sb, zb, case["sum_q"][0], case["sum_q"][1], None), hip, "add")
        if case["act"]:
            pkg.check(hip.shl_mi355x_relu_i8(d_sum, d_un, n, case["sum_q"][0], case["sum_q"][1], case["out_q"][0], case["out_q"][1],
                                             int(case["act"] == 2), None), hip, "relu_i8")
        unfused = dev.download(d_un if case["act"] else d_sum, c["out_shape"], np.int8)
        whole = dev.download(d_guarded, (n + 2 * GUARD,), np.uint8)
        fused = whole[GUARD:GUARD + n].view(np.int8).reshape(c["out_shape"])
        guards = np.concatenate([whole[:GUARD], whole[GUARD + n:]])
        return fused, unfused, guards, name
    finally:
        for p in (d_in, d_skip, d_conv, d_sum, d_un, d_guarded):
            dev.free(p)
        hip.shl_mi355x_conv_plan_destroy(plan)


def check_case(hip, dev, case, expect_family):
    want = oracle_chain(case)["out"]
    fused, unfused, guards, name = run_both(hip, dev, case)
    assert name == expect_family + "+add", (case["name"], name)
    assert (guards == POISON).all(), case["name"] + ": the fused launch wrote outside its output"
    for what, got in (("unfused", unfused), ("fused", fused)):
        bad, worst = cases.mismatch_report(got, want)
        assert bad == 0, "%s: %s differs from the oracle chain on %d of %d outputs (max %d)" % (case["name"], what, bad, got.size, worst)
    assert np.array_equal(fused, unfused)
    assert len(np.unique(want)) > 8 or flat_by_record(case), case["name"] + ": the expected output cannot tell results apart"


if __name__ == "__main__":  # the child of tests/test_residual.py: the tile flavours chosen through the environment
    hip = pkg.load_hip()
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    device = cases.HipDevice(hip)
    os.environ["SHL_MI355X_RESIDUAL_FORM"] = "tile"
    for cs in child_cases():
        check_case(hip, device, cs, "tile")
        print("ok", cs["name"])
    print("child ok", len(child_cases()))
    sys.exit(0)

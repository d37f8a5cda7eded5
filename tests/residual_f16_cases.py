"""Cases of the binary16 fused residual tail -- conv2d [+ folded activation] -> add(conv_out, skip) -> [relu | relu6] in the
convolution's launch (shl_mi355x_conv_add_f16_forward) -- with the oracle chain and the two ways to run them on the device.

Every case is binary16 NHWC; the skip tensor is 3 * standard_normal as float16, seeded.  Shapes are the smallest at which each
store path of the two carrying kernel families can go wrong (M = N Ho Wo):
  wave   ragged pixel and channel tiles with 8-byte stores, the element-store path (Co % 4 != 0), the split-K tail (K rows of
         256 bytes on few tiles), 3x3 at stride 1 and 2
  tile   the second ragged tile of the 128 x 128 flavour through the staged stores (Co % 8 == 0), through the 8-byte stores
         (Co % 4 == 0 only) and through the element stores, 256 x 64, 3x3; 256 x 128 and 256 x 256 and the flavours with other
         producer-wave settings in a child process (the switches are read once per process): `python residual_f16_cases.py`
         runs child_cases() under the caller's environment
Across the list: the convolution's value as either operand, no activation / relu / relu6, a convolution with its own folded
relu6.  The specials cases (one per family and operand order) put +-NaN (quiet and signalling), +-inf, +-0, subnormals and
+-65504 into the skip tensor and a NaN into one pixel of the convolution's input, so that NaN meets NaN in both orders.

What "equal" means.  The device's stand-alone layers run the convolution on the wave kernel at these sizes -- its split-K form
when there are at most 256 tiles of K rows of 256 bytes and more.  A fused launch on the wave kernel takes the same form, and
the tile kernels add the K steps up in the order of the wave kernel's one-pass form; the split-K form adds four partial sums,
another fp32 rounding order.  So every case is compared on bits, and the tile cases keep K rows under 256 bytes (or more than
256 tiles), where the two families agree.  Against the oracle: the stand-alone convolution within the tolerance of the binary16
convolution parity tests (golden_util.compare_f16_tol), and the fused output EXACTLY equal to the oracle's add and relu applied
to the halves that convolution stored -- the tail adds no error of its own, so the fused launch is as far from the oracle chain
as the convolution alone carries through two 1-Lipschitz steps.
"""
import ctypes as C
import os
import sys

import numpy as np

import cases
import golden_util
import tail
from cases import pkg
from residual_cases import CHILD_ENVS, conv_desc, make_plan  # noqa: F401  (the same children, descriptors and plans)

POISON = 0x5A
GUARD = 256

# bit patterns of the specials a skip tensor carries: quiet and signalling NaNs of both signs, infinities, zeros, the smallest
# and the largest subnormals, the largest finite values
SPECIALS = np.array([0x7E00, 0xFE00, 0x7C01, 0xFC01, 0x7C00, 0xFC00, 0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x7BFF, 0xFBFF],
                    dtype=np.uint16)


def _case(name, form, conv, conv_first=1, act=0, seed=0, specials=False):
    c = cases.make_case(9300 + seed, dtype="f16", **conv)
    rng = np.random.default_rng(9400 + seed)
    skip = (3 * rng.standard_normal(c["out_shape"])).astype(np.float16)
    if specials:
        # pixel 0 of the convolution's input holds a NaN: every output channel of the pixels that read it is NaN.  The skip's
        # pixels 0 and 1 cycle through the specials, so each of them meets a NaN (pixel 0 of a 1x1) and a finite value
        c["input"] = c["input"].copy()
        c["input"].reshape(-1)[0] = np.float16(np.nan)
        flat = skip.reshape(-1, c["co"]).view(np.uint16)
        for p in (0, 1, 2):
            flat[p, :] = np.resize(np.roll(SPECIALS, p), c["co"])
    return dict(name=name, form=form, conv=c, conv_first=conv_first, act=act, skip=skip, specials=specials)


PW = dict(k=(1, 1), pad=(0, 0, 0, 0))


def all_cases():
    out = []
    # ---- wave
    out.append(_case("wave_1x1_m33_co36", "wave", dict(PW, h=3, w=11, c=16, co=36), conv_first=1, act=1, seed=1))
    out.append(_case("wave_1x1_m33_co30_elements", "wave", dict(PW, h=3, w=11, c=16, co=30), conv_first=0, act=0, seed=2))
    out.append(_case("wave_1x1_c128_splitk", "wave", dict(PW, h=8, w=8, c=128, co=32, act=2), conv_first=0, act=2, seed=3))
    out.append(_case("wave_3x3_5x7", "wave", dict(h=5, w=7, c=16, co=32), conv_first=1, act=2, seed=4))
    out.append(_case("wave_3x3_s2_9x9", "wave", dict(h=9, w=9, c=16, co=32, stride=(2, 2)), conv_first=0, act=1, seed=5))
    # ---- tile
    out.append(_case("tile_m129_co144_staged", "tile", dict(PW, h=3, w=43, c=32, co=144), conv_first=1, act=1, seed=8))
    out.append(_case("tile_m129_co130_elements", "tile", dict(PW, h=3, w=43, c=16, co=130), conv_first=0, act=2, seed=9))
    out.append(_case("tile_m129_co132_8byte", "tile", dict(PW, h=3, w=43, c=16, co=132), conv_first=1, act=0, seed=10))
    out.append(_case("tile_m257_co64_256x64", "tile", dict(PW, h=1, w=257, c=32, co=64, act=2), conv_first=1, act=0, seed=11))
    out.append(_case("tile_3x3_m130_co32", "tile", dict(h=10, w=13, c=8, co=32), conv_first=0, act=1, seed=12))
    # ---- specials: both families, both operand orders; no activation behind the sum where the NaNs are to reach the output
    out.append(_case("wave_specials_conv_first", "wave", dict(PW, h=3, w=11, c=16, co=36), conv_first=1, act=0, seed=13, specials=True))
    out.append(_case("wave_specials_skip_first", "wave", dict(PW, h=3, w=11, c=16, co=30), conv_first=0, act=0, seed=14, specials=True))
    out.append(_case("tile_specials_conv_first", "tile", dict(PW, h=3, w=43, c=32, co=144), conv_first=1, act=0, seed=15, specials=True))
    out.append(_case("tile_specials_skip_first_relu6", "tile", dict(PW, h=3, w=43, c=16, co=130), conv_first=0, act=2, seed=16, specials=True))
    return out


def child_cases():
    """the large tile flavours need uniform-tap addressing (C % 32 == 0); one ragged tile in each direction.  (The 3x3 case has
    more than 256 wave tiles, so that the stand-alone convolution does not split K.)"""
    return [_case("tile_m257_co144_c32", "tile", dict(PW, h=1, w=257, c=32, co=144), conv_first=1, act=2, seed=20),
            _case("tile_m257_co272_c32", "tile", dict(PW, h=1, w=257, c=32, co=272), conv_first=0, act=1, seed=21),
            _case("tile_3x3_m260_co930_c32", "tile", dict(h=10, w=26, c=32, co=930), conv_first=1, act=0, seed=22)]


def wave_tiles(case):
    c = case["conv"]
    return ((c["n"] * c["ho"] * c["wo"] + 31) // 32) * ((c["co"] + 31) // 32)


def k_row_bytes(case):
    """bytes of a packed weight row (csrc/conv_plan.hip pads K rows to a multiple of 64 bytes)"""
    c = case["conv"]
    return (c["kh"] * c["kw"] * c["c"] * 2 + 63) // 64 * 64


def splits_k(case):
    """csrc/conv_igemm.hip:launch_wave_regs_tile restated: the wave kernel's split-K form"""
    return wave_tiles(case) <= 256 and k_row_bytes(case) >= 256


# ------------------------------------------------------------------------------------------ the oracle chain
def tail_of(case, conv):
    """the reference's add and relu (oracle/) on stored halves: `conv` is a convolution's output"""
    one = (1.0, 0)
    a, b = (conv, case["skip"]) if case["conv_first"] else (case["skip"], conv)
    total = tail.siso_oracle(dict(kind="add", dtype="f16", x=a, y=b, in_q=one, in1_q=one, out_q=one))
    if case["act"]:
        total = tail.siso_oracle(dict(kind="relu6" if case["act"] == 2 else "relu", dtype="f16", x=total, in_q=one, out_q=one))
    return total


def oracle_chain(case):
    conv = cases.oracle_run(case["conv"], "f16")
    return dict(conv=conv, out=tail_of(case, conv))


# ------------------------------------------------------------------------------------------ the device
def residual_desc(case):
    """only conv_first and act are read; the scale fields carry what an int8 launch would refuse"""
    d = pkg.ResidualDesc()
    d.conv_first, d.act = case["conv_first"], case["act"]
    d.skip_scale, d.sum_scale, d.out_scale = 0.0, float("nan"), -1.0
    return d


def run_both(hip, dev, case):
    """(fused output, unfused output, the stand-alone convolution's output, the guard bytes around the fused output, the fused
    launch's kernel name, its flavour record)"""
    c = case["conv"]
    n = int(np.prod(c["out_shape"]))
    plan = make_plan(hip, c)
    d_in, d_skip, d_conv, d_sum, d_un = (dev.alloc(c["input"].nbytes), dev.alloc(2 * n), dev.alloc(2 * n), dev.alloc(2 * n), dev.alloc(2 * n))
    d_guarded = dev.alloc(2 * n + 2 * GUARD)
    try:
        dev.upload(d_in, c["input"])
        dev.upload(d_skip, case["skip"])
        dev.upload(d_guarded, np.full(2 * n + 2 * GUARD, POISON, np.uint8))
        d_out = d_guarded + GUARD
        name = hip.shl_mi355x_conv_add_f16_kernel_name(plan, 0).decode()
        pkg.check(hip.shl_mi355x_conv_add_f16_forward(plan, d_in, d_skip, d_out, 0, C.byref(residual_desc(case)), None), hip, "conv_add_f16_forward")
        flavour = hip.shl_mi355x_last_igemm_flavour().decode()
        # the layers one by one
        pkg.check(hip.shl_mi355x_conv_forward(plan, d_in, d_conv, 0, None), hip, "conv_forward")
        a, b = (d_conv, d_skip) if case["conv_first"] else (d_skip, d_conv)
        pkg.check(hip.shl_mi355x_add(a, b, d_sum, n, pkg.SHL_F16, 1.0, 0, 1.0, 0, 1.0, 0, None), hip, "add")
        if case["act"]:
            pkg.check(hip.shl_mi355x_relu_f16(d_sum, d_un, n, int(case["act"] == 2), None), hip, "relu_f16")
        unfused = dev.download(d_un if case["act"] else d_sum, c["out_shape"], np.float16)
        conv = dev.download(d_conv, c["out_shape"], np.float16)
        whole = dev.download(d_guarded, (2 * n + 2 * GUARD,), np.uint8)
        fused = whole[GUARD:GUARD + 2 * n].view(np.float16).reshape(c["out_shape"])
        guards = np.concatenate([whole[:GUARD], whole[GUARD + 2 * n:]])
        return fused, unfused, conv, guards, name, flavour
    finally:
        for p in (d_in, d_skip, d_conv, d_sum, d_un, d_guarded):
            dev.free(p)
        hip.shl_mi355x_conv_plan_destroy(plan)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint16), np.ascontiguousarray(b).view(np.uint16))


def check_case(hip, dev, case, expect_family):
    fused, unfused, conv, guards, name, flavour = run_both(hip, dev, case)
    assert name == expect_family + "+add", (case["name"], name)
    assert flavour.startswith(expect_family + "/") and flavour.endswith("epi0+add"), (case["name"], flavour)
    if expect_family == "wave":
        assert flavour.startswith("wave/ks4/" if splits_k(case) else "wave/ks1/"), (case["name"], flavour)
    assert (guards == POISON).all(), case["name"] + ": the fused launch wrote outside its output"
    diff = np.ascontiguousarray(fused).view(np.uint16) != np.ascontiguousarray(unfused).view(np.uint16)
    assert not diff.any(), "%s: the fused launch differs from the layers on %d of %d halves" % (case["name"], int(diff.sum()), diff.size)
    if case["specials"]:
        assert np.isnan(fused).any() == (case["act"] == 0), case["name"] + ": NaNs reach the output exactly where nothing clamps them"
        return
    want = oracle_chain(case)
    golden_util.compare_f16_tol(conv, want["conv"], case["name"] + ": the stand-alone convolution")
    assert same_bits(fused, tail_of(case, conv)), case["name"] + ": not the oracle's add and relu of the convolution's stored halves"
    assert len(np.unique(want["out"])) > 8 and (want["out"] != want["conv"]).mean() > 0.5, case["name"] + ": the expected output cannot tell results apart"


if __name__ == "__main__":  # the child of tests/test_residual_f16.py: the tile flavours chosen through the environment
    hip = pkg.load_hip()
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    device = cases.HipDevice(hip)
    os.environ["SHL_MI355X_RESIDUAL_FORM"] = "tile"
    for cs in child_cases():
        check_case(hip, device, cs, "tile")
        print("ok", cs["name"])
    print("child ok", len(child_cases()))
    sys.exit(0)

"""Grouped binary16 NCHW convolution on the matrix cores (csrc/conv_group_mfma_f16.hip) against a float64 numpy reference of the
same binary16 operands, under DESIGN section 2's gate for MFMA f16 kernels, |got - ref| <= 1e-3 max(|ref|, 1); the direct kernel
(switch 0) is put to the same gate.  SHL_MI355X_GROUPMFMA_F16 is read at each plan creation, so the tests flip it in-process.
Non-finite inputs: the reference's float -> binary16 conversion saturates (common.h:float_to_f16_bits_ref), so every f16 kernel of
the project, the direct one included, stores an infinite sum as +-65504: the float64 reference is clipped the same way before
the classes are compared, and an infinite reference sum must come out as exactly +-65504."""
import ctypes as C

import numpy as np
import pytest

import cases
import residual_cases as rc
from cases import pkg

SWITCH = "SHL_MI355X_GROUPMFMA_F16"
NAME, DIRECT = "conv_group_mfma_f16_mfma16x16x32", "conv_group_direct_f16"
SHAPES = [
    ("c32_g8_9x7", dict(c=32, co=32, groups=8, h=9, w=7)),                                         # 4 per group, two taps per lane, ragged 63-pixel map
    ("c64_g8_12x9_s2_n3_relu", dict(c=64, co=64, groups=8, h=12, w=9, stride=(2, 2), n=3, act=1)),  # 8 per group, stride-2 patch, batch
    ("c96_g6_7x7", dict(c=96, co=96, groups=6, h=7, w=7)),                                         # 16 per group, half a tap per lane, three units
    ("c64_g2_8x8", dict(c=64, co=64, groups=2)),                                                   # 32 per group: the narrow / wide boundary
    ("c128_co64_g2", dict(c=128, co=64, groups=2)),                                                # two K slabs per tap
    ("c64_co128_g2", dict(c=64, co=128, groups=2)),                                                # several output blocks over one window
    ("c64_g4_1x1", dict(c=64, co=64, groups=4, k=(1, 1), pad=(0, 0, 0, 0))),                       # one tap: every other K slot is padding
    ("c64_g8_5x5_s2_asym", dict(c=64, co=64, groups=8, k=(5, 5), stride=(2, 2), pad=(1, 1, 2, 2))),  # 25 taps, 4 per MFMA; asymmetric padding
    ("c64_g4_relu6", dict(c=64, co=64, groups=4, act=2)),
    ("c32_g8_40x40_n2", dict(c=32, co=32, groups=8, h=40, w=40, n=2)),                             # several rectangles, several tiles per wave
]
OUTSIDE = [
    ("c192_g96", dict(c=192, co=192, groups=96)),  # 2 per group
    ("c32_co64_g8", dict(c=32, co=64, groups=8)),  # 4 in, 8 out
    ("nhwc", dict(c=64, co=64, groups=8, layout="NHWC")),
    ("dilation2", dict(c=64, co=64, groups=8, dilation=(2, 2), pad=(2, 2, 2, 2))),
]
GUARDED = [0, 4]


def make(i, kw):
    return cases.make_case(6100 + i, **dict(dict(layout="NCHW", dtype="f16"), **kw))


def reference(c):
    """float64 grouped convolution (NCHW, OIHW) of the binary16 operands, + bias, relu / relu6"""
    (pt, pl, pb, pr), (sh, sw), G = c["pad"], c["stride"], c["group"]
    xp = np.zeros((c["n"], c["c"], c["h"] + pt + pb, c["w"] + pl + pr))
    xp[:, :, pt:pt + c["h"], pl:pl + c["w"]] = c["input"]
    w, cpg, opg, out = c["kernel"].astype(np.float64), c["c"] // G, c["co"] // G, np.zeros(c["out_shape"])
    with np.errstate(invalid="ignore"):
        for g, ky, kx in np.ndindex(G, c["kh"], c["kw"]):
            win = xp[:, g * cpg:(g + 1) * cpg, ky:ky + sh * (c["ho"] - 1) + 1:sh, kx:kx + sw * (c["wo"] - 1) + 1:sw]
            out[:, g * opg:(g + 1) * opg] += np.einsum("nchw,oc->nohw", win, w[g * opg:(g + 1) * opg, :, ky, kx])
        out += c["bias"].astype(np.float64)[None, :, None, None]
        if c["act"]:
            out = np.where(out > 0, out, 0.0)  # (the kernels' comparison: NaN -> 0)
    return np.minimum(out, 6.0) if c["act"] == 2 else out


def gate(got, ref):
    with np.errstate(invalid="ignore"):
        return np.abs(got.astype(np.float64) - ref) <= 1e-3 * np.maximum(np.abs(ref), 1.0)


def run(standalone, monkeypatch, case, switch):
    fe, hip, opt = standalone
    monkeypatch.setenv(SWITCH, switch)
    keep = []
    got = cases.csinn_run(fe, pkg.API_MI355X, case, device=cases.HipDevice(hip), keep_params=keep)
    name = opt.shl_mi355x_params_kernel_name(keep[0][0]).decode()
    opt.shl_mi355x_release_params(keep[0][0])
    return name, got


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[s[0] for s in SHAPES])
def test_grouped_f16_mfma_and_direct_pass_the_same_gate(standalone, monkeypatch, i):
    case = make(i, SHAPES[i][1])
    ref = reference(case)
    for switch, want in (("1", NAME), ("0", DIRECT)):
        name, got = run(standalone, monkeypatch, case, switch)
        assert name == want
        assert gate(got, ref).all(), "%s: %d outputs outside the gate" % (name, int((~gate(got, ref)).sum()))


@pytest.mark.gpu
def test_non_finite_inputs_stay_inside_their_group(standalone, monkeypatch):
    case = make(50, dict(c=64, co=64, groups=8))
    case["input"][0, 3 * 8 + 1, 1, 2] = np.float16(np.inf)  # group 3, rows 1 and 6: no output reads both
    case["input"][0, 3 * 8 + 5, 6, 5] = np.float16(np.nan)
    full = reference(case)
    ref = np.clip(full, -65504.0, 65504.0)  # the reference's saturating conversion (module docstring); NaN stays NaN
    others = np.arange(64) // 8 != 3
    assert np.isnan(full).any() and np.isinf(full).any() and np.isfinite(full[:, others]).all()
    for switch, want in (("1", NAME), ("0", DIRECT)):
        name, got = run(standalone, monkeypatch, case, switch)
        assert name == want
        assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN positions differ" % name
        assert np.isfinite(got[:, others]).all()
        assert np.array_equal(got[np.isinf(full)].astype(np.float64), ref[np.isinf(full)])  # +-inf -> +-65504, sign kept
        assert gate(got, ref)[np.isfinite(full)].all()


@pytest.mark.gpu
@pytest.mark.parametrize("i", GUARDED, ids=[SHAPES[i][0] for i in GUARDED])
def test_conv_forward_writes_the_output_and_nothing_beside_it(standalone, monkeypatch, i):
    hip, GUARD, POISON, c = standalone[1], 256, 0x5A, make(i, SHAPES[i][1])
    monkeypatch.setenv(SWITCH, "1")
    n, desc, plan, dev = int(np.prod(c["out_shape"])) * 2, rc.conv_desc(c), C.c_void_p(), cases.HipDevice(hip)
    desc.algo = 7  # SHL_MI355X_ALGO_GROUP: the operator API asks for a grouped layer by name
    bias = c["bias"].astype(np.float32)
    pkg.check(hip.shl_mi355x_conv_plan_create(C.byref(desc), c["kernel"].ctypes.data, None, bias.ctypes.data, None, C.byref(plan)), hip, "plan")
    d_in, d_out = dev.alloc(c["input"].nbytes), dev.alloc(n + 2 * GUARD)
    dev.upload(d_in, c["input"]), dev.upload(d_out, np.full(n + 2 * GUARD, POISON, np.uint8))
    name = hip.shl_mi355x_conv_plan_kernel_name(plan).decode()
    pkg.check(hip.shl_mi355x_conv_forward(plan, d_in, d_out + GUARD, 0, None), hip, "conv_forward")
    whole = dev.download(d_out, (n + 2 * GUARD,), np.uint8)
    dev.free(d_in), dev.free(d_out), hip.shl_mi355x_conv_plan_destroy(plan)
    assert name == NAME and np.all(whole[:GUARD] == POISON) and np.all(whole[GUARD + n:] == POISON)
    assert gate(whole[GUARD:GUARD + n].view(np.float16).reshape(c["out_shape"]), reference(c)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(len(OUTSIDE)), ids=[s[0] for s in OUTSIDE])
def test_layers_outside_the_scope_stay_on_the_direct_kernel(standalone, monkeypatch, j):
    assert run(standalone, monkeypatch, make(20 + j, OUTSIDE[j][1]), "1")[0] == DIRECT

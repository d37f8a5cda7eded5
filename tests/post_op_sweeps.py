"""Seeded, stratified draws for the fused post-op launches -- conv2d -> add(skip) -> [relu | relu6] (family "conv_add",
shl_mi355x_conv_add_forward), conv2d -> table (family "conv_lut", shl_mi355x_conv_lut_forward) and depthwise conv2d -> table
(family "dw_lut", shl_mi355x_dwconv_lut_forward) -- over every kernel flavour that carries them.  The hand lists of
residual_cases.py, act_fuse_cases.py and dw_act_cases.py run 21 and 18 of the 56 instantiations
conv_igemm.hip:launch_wave_regs_tile can launch per post-op; these draws run each of them twice.

  strata(family, i)      what case i is there for (round-robin by the index: the same for every seed)
  draw(family, i)        keyword arguments for cases.make_case (free parameters: random, moved by SHL_TEST_FUZZ_SEED)
  case_seed(family, i)   the seed of its operands
  case_env(family, i)    the environment the case needs: the form switch (read per call), and for the flavours that
                         SHL_MI355X_TILE / SHL_MI355X_PIPE / SHL_MI355X_DWMFMA select (read once per process) those
  child_index(family, i) None: the case runs in the test process; k: in the child of residual_cases.CHILD_ENVS[k]
                         ("dw_lut": 0, the child under SHL_MI355X_DWMFMA=1)
  flavour_of(kw, env, post)  the string shl_mi355x_last_igemm_flavour() must give after the fused launch

`python tests/post_op_sweeps.py <family>` runs the family's cases of the calling environment and prints `child ok N`.

conv_add / conv_lut: i = 14 j + f.  f is the flavour (FLAVOURS), j % 4 the requantisation code (0, 1, 3, 4: family_sweeps'
docstring says why 2 and 5 cannot be reached), j // 4 the round.  Every other stratum is a shifted cycle in (f, j), so that a
flavour meets all of its values and no stratum is a function of another.  wave/ks1 meets the 5x5 and 7x7 windows, whose
packed K rows of 400 and 784 bytes at C = 16 are split-K up to 256 tiles, on 257 tiles and more: thousands of pixels at one
or two channel tiles.  Two things the strata cannot hold, by arithmetic:
  * a pixel count M = 1 or TBM - 1 (mod TBM) is odd, so such a case never has batch 2;
  * 256x64 without SHL_MI355X_TILE runs only for Co <= 64: one channel tile.
"""
import os
import sys

import numpy as np

import family_sweeps as fs

BASE_SEED = fs.BASE_SEED
FAMILIES = {"conv_add": dict(n=112, offset=1100, cap=2e8), "conv_lut": dict(n=112, offset=1200, cap=2e8),
            "dw_lut": dict(n=88, offset=1300, cap=2e8)}
CHUNK = 8
EPI = (0, 1, 3, 4)
FORM_SWITCH = {"add": "SHL_MI355X_RESIDUAL_FORM", "lut": "SHL_MI355X_ACT_FORM"}
POST = {"conv_add": "add", "conv_lut": "lut"}
# (flavour, the entry of residual_cases.CHILD_ENVS that reaches it or None: the default environment does)
FLAVOURS = (("wave/ks1", None), ("wave/ks4", None), ("tile/128x128/pipe8/utap", None), ("tile/128x128/pipe4/anytap", None),
            ("tile/256x64/pipe0/utap", None), ("tile/256x64/pipe0/anytap", None),
            ("tile/256x128/pipe0/utap", 0), ("tile/256x128/pipe6/utap", 1), ("tile/256x256/pipe0/utap", 2),
            ("tile/128x128/pipe0/utap", 3), ("tile/128x128/pipe0/anytap", 3), ("tile/128x128/pipe4/utap", 4),
            ("tile/256x64/pipe4/utap", 5), ("tile/256x64/pipe4/anytap", 5))
DW_CHILD_ENV = {"SHL_MI355X_DWMFMA": "1"}
WINDOWS = ("1x1", "1x1s2", "3x3same", "3x3s2", "3x3d2", "5x5", "1x7", "7x7")
# window -> (kernel, stride, dilation); "1x7" is 1x7 or 7x1 with asymmetric padding along the 7
WINDOW_GEOM = {"1x1": ((1, 1), (1, 1), (1, 1)), "1x1s2": ((1, 1), (2, 2), (1, 1)), "3x3same": ((3, 3), (1, 1), (1, 1)),
               "3x3s2": ((3, 3), (2, 2), (1, 1)), "3x3d2": ((3, 3), (1, 1), (2, 2)), "5x5": ((5, 5), (1, 1), (1, 1)),
               "1x7": ((1, 7), (1, 1), (1, 1)), "7x7": ((7, 7), (1, 1), (1, 1))}
CHANNELS = (("staged", 0), ("elements", 1), ("dwords", 0), ("staged", 1), ("elements", 0), ("dwords", 1))  # (store path, a ragged second tile)
PIXELS = ("one", "last", "other")   # M % TBM == 1, == TBM - 1, anything else
ZPS = (-128, 0, 127, None)          # None: random
MIN_OUTPUTS = 640


def case_seed(family, i):
    return 920000 + FAMILIES[family]["offset"] * 10 + i


def _rng(family, i, seed):
    return np.random.default_rng([(BASE_SEED if seed is None else seed) + FAMILIES[family]["offset"], i])


def ceil_div(a, b):
    return (a + b - 1) // b


def tile_of(flavour):
    """(TBM, TBN): the pixels and channels of one workgroup's tile (the wave kernel: of one wave's)"""
    if flavour.startswith("wave"):
        return 32, 32
    a, b = flavour.split("/")[1].split("x")
    return int(a), int(b)


def store_path(co):
    return "staged" if co % 16 == 0 else ("dwords" if co % 4 == 0 else "elements")


def flavour_of(kw, env, post):
    """conv_igemm.hip:launch_wave_regs_tile restated, with the family choice of conv_plan.hip:residual_family / lut_family in
    front of it: the instantiation a fused launch of make_case(**kw) runs under `env`, in the words of
    shl_mi355x_last_igemm_flavour().  post: "add" | "lut" """
    g = fs.geometry(kw)
    M, C, Co = g["M"], kw["c"], kw["co"]
    kh, kw_ = kw.get("k", (3, 3))
    kstride = fs.align_up(kh * kw_ * C, 64)   # conv_plan.hip: the packed K row
    tail = "/epi%d+%s" % (fs.epi_code(kw), post)
    form = env.get(FORM_SWITCH[post])
    if form not in ("wave", "tile"):  # igemm_size_rule
        form = "tile" if ceil_div(M, 128) * ceil_div(Co, 128) >= (24 if kstride >= 8192 else 96 if kstride >= 512 else 128) else "wave"
    if form == "wave":
        split = ceil_div(M, 32) * ceil_div(Co, 32) <= 256 and kstride >= 256
        return "wave/ks%d" % (4 if split else 1) + tail
    utap = C % 64 == 0 and kh * kw_ <= 32
    m256 = ceil_div(M, 256)
    tile = "128x128"
    if Co <= 64:
        tile = "256x64"
    elif utap and Co >= 256 and m256 * ceil_div(Co, 256) >= 1024:
        tile = "256x256"
    elif utap and m256 * ceil_div(Co, 128) >= 2048:
        tile = "256x128"
    forced = env.get("SHL_MI355X_TILE")
    if forced == "128":
        tile = "128x128"
    elif forced == "256x64" or (forced in ("256x128", "256x256") and utap):
        tile = forced
    pipe = 4 if tile == "128x128" else 0
    if tile == "128x128" and utap and ceil_div(M, 128) * ceil_div(Co, 128) <= 256:
        pipe = 8
    pe = env.get("SHL_MI355X_PIPE")
    if pe is not None:
        pipe = {"8": 8, "6": 6, "0": 0}.get(pe[:1], 4)
    if tile == "256x64":
        pipe = 4 if pipe else 0
    elif tile == "256x128":
        pipe = 6 if pipe == 6 else 0
    elif tile == "256x256":
        pipe = 0
    else:
        pipe = 8 if pipe == 8 and utap else (4 if pipe else 0)
    return "tile/%s/pipe%d/%s" % (tile, pipe, "utap" if utap else "anytap") + tail


def child_envs():
    """residual_cases.CHILD_ENVS, the six environments that reach the flavours a once-per-process switch selects"""
    import residual_cases as rc
    return rc.CHILD_ENVS


def windows_of(flavour):
    """(uniform-tap addressing takes at most 32 taps: no 7x7 there)"""
    return WINDOWS[:7] if flavour.endswith("/utap") else WINDOWS


# ------------------------------------------------------------------------------------------------ conv_add, conv_lut
def conv_strata(i):
    f, j = i % 14, i // 14
    flavour, child = FLAVOURS[f]
    wins = windows_of(flavour)
    code = EPI[j % 4]
    pixels = PIXELS[(f // 3 + j + j // 3) % 3]
    by_call = (f + j // 2) % 3 == 0   # the plan is made at batch 1, the call passes the batch
    x = f // 2 + j // 2
    if pixels == "other":
        n = (2, 3)[x % 2] if by_call else (1, 2, 2, 3)[x % 4]
    else:
        n = 3 if by_call else (1, 3)[x % 2]
    path, two = CHANNELS[(f // 2 + j) % 6]
    if flavour.startswith("tile/256x64/pipe0"):
        two = 0
    return dict(flavour=flavour, child=child, code=code, round=j // 4, window=wins[(f + j) % len(wins)], pixels=pixels,
                tiles2=(f + j) % 3 != 0, n=n, by_call=by_call, path=path, two=two, per_channel=(f + j // 2) % 2 == 0,
                exact=code >= 3, act=0 if code in (0, 3) else 1 + (f + j // 4) % 2)


def _channels_in(flavour, window, rng):
    if flavour == "wave/ks4":   # a packed K row of at least 256 bytes, three ways
        return {"1x1": (256, 320, 512), "1x1s2": (256, 320, 512), "5x5": (16,), "7x7": (16,), "1x7": (48, 80)}.get(window, (32,))
    if flavour == "wave/ks1":   # ... and one below
        return {"1x1": (16, 32, 48, 80), "1x1s2": (16, 32, 48, 80), "1x7": (16, 32)}.get(window, (16,))
    if flavour.endswith("/utap"):
        return (64, 128, 192, 256) if window.startswith("1x1") else (64,) if window == "5x5" else (64, 128)
    return (64,) if window == "7x7" else (16, 32, 48, 80)


def _factor(rng, hw):
    pairs = [(a, hw // a) for a in range(1, hw + 1) if hw % a == 0]
    return fs._pick(rng, [p for p in pairs if p[0] != p[1] and min(p) > 2] or [p for p in pairs if p[0] != p[1]] or pairs)


def _window(rng, window):
    (kh, kw_), stride, dil = WINDOW_GEOM[window]
    if window in ("1x1", "1x1s2"):
        pad = (0, 0, 0, 0)
    elif window == "3x3same":
        pad = (1, 1, 1, 1)
    elif window == "1x7":
        a, b = fs._pick(rng, ((0, 3), (3, 0), (1, 3), (2, 3), (3, 1), (0, 2), (2, 0), (1, 2)))
        pad = (0, a, 0, b)
        if rng.integers(0, 2):
            kh, kw_, pad = 7, 1, (a, 0, b, 0)
    else:
        pad = fs._pads(rng) if window != "7x7" else tuple(int(v) for v in rng.integers(0, 4, 4))
    return (kh, kw_), stride, dil, pad


def _in_size(rng, out, k, s, d, p0, p1):
    v = (out - 1) * s + d * (k - 1) + 1 - p0 - p1 + int(rng.integers(0, s))
    return v if v >= 1 and fs.out_size(v, k, s, p0, p1, d) == out else None


def _draw_conv(family, i, rng):
    s = conv_strata(i)
    env = case_env(family, i)
    tbm, tbn = tile_of(s["flavour"])
    cap = FAMILIES[family]["cap"]
    for attempt in range(4000):
        relax = attempt >= 2000   # the tile count gives way before the residue and the batch do
        c = int(fs._pick(rng, _channels_in(s["flavour"], s["window"], rng)))
        (kh, kw_), stride, dil, pad = _window(rng, s["window"])
        res = {"one": 1, "last": tbm - 1}.get(s["pixels"])
        if res is None:
            res = 0 if s["flavour"] != "wave/ks4" and rng.integers(0, 4) == 0 else int(rng.integers(2, tbm - 1))
        hi = 6 if tbm == 32 else 4
        # (one pixel is no sweep case: M % TBM == 1 comes with a tile in front of it)
        t = int(rng.integers(1, hi + 1)) if relax else (int(rng.integers(2, hi + 1)) if s["tiles2"] or res == 1 else 1)
        if s["flavour"] == "wave/ks1" and fs.align_up(kh * kw_ * c, 64) >= 256:
            # K rows of split-K's length: no split from 257 tiles on, with one channel tile or with two
            first = 256 // (2 if s["two"] else 1) + 1
            t = int(rng.integers(first, first + 6))
        M = (t - 1) * tbm + (res or tbm)
        if M % s["n"]:
            continue
        ho, wo = _factor(rng, M // s["n"])
        h, w = _in_size(rng, ho, kh, stride[0], dil[0], pad[0], pad[2]), _in_size(rng, wo, kw_, stride[1], dil[1], pad[1], pad[3])
        if not (h and w):
            continue
        lo, hi_co = (tbn + 1, 2 * tbn - 1) if s["two"] else (65 if s["flavour"].startswith("tile/128x128") and s["child"] is None else 5, tbn)
        # (at least MIN_OUTPUTS outputs, so that the oracle's bytes can spread)
        cos = [v for v in range(lo, hi_co + 1) if store_path(v) == s["path"] and M * v * c * kh * kw_ <= cap and M * v >= MIN_OUTPUTS]
        if not cos:
            continue
        kw = dict(n=s["n"], h=h, w=w, c=c, co=int(fs._pick(rng, cos)), k=(kh, kw_), stride=stride, dilation=dil, pad=pad, act=s["act"],
                  exact=s["exact"], per_channel=s["per_channel"])
        if flavour_of(kw, env, POST[family]) == "%s/epi%d+%s" % (s["flavour"], s["code"], POST[family]):
            return kw
    raise RuntimeError("no draw for %s case %d: %r" % (family, i, s))


def residual_strata(i):
    """the record of the add behind case i of conv_add"""
    f, j = i % 14, i // 14
    act = (f + j + j // 3) % 3
    sum_zp = ZPS[(i + i // 4) % 4]
    if act and sum_zp == 127:   # every sum at or above zero saturates, the activation maps all of it to one byte: not a flat RECORD
        sum_zp = -128
    out_zp = ZPS[(i + i // 16 + 1) % 4]
    if out_zp == 127 and not (act and i % 32 == 9):   # flat by record: held to a few cases
        out_zp = None
    if act and i % 32 == 9:
        out_zp = 127
    skip_zp, skip_fill = ZPS[i % 4], None
    if sum_zp == 127 and skip_zp == -128:   # a skip tensor at or above zero behind a clamped convolution: no sum below zero, one byte
        skip_zp = None
    if i % 16 == 13:   # a constant skip tensor under zero points of 0 (residual_cases' *_skip_all_*): part of the sums saturates, the rest
        # spreads; below zero where the activation is none or relu6 (the add's record puts 0 .. 6 in reach), above it for relu
        skip_fill = 127 if act == 1 or (act == 0 and (i // 16) % 2) else -128
        skip_zp = sum_zp = 0
    return dict(conv_first=(f // 2 + j // 2 + j) % 2, act=act, skip_zp=skip_zp, sum_zp=sum_zp, out_zp=out_zp, pow2=(i // 2 + j) % 2 == 0,
                no_fma_div=i % 16 == 5, skip_fill=skip_fill)


# ------------------------------------------------------------------------------------------------ dw_lut
DW_MFMA_N, DW_DOT4_N, DW_NHWC_N = 40, 24, 24
DW_STRIDES = ((1, 1), (2, 2), (1, 2), (2, 1))
DW_LANES = ("lt64", "64to256", "gt256")   # Wo * C / 4 of the dot4 kernel: part of a block, one block, a second block in y
NHWC_WINDOWS = ((5, 5), (3, 5), (5, 3), (7, 7), (1, 3), (2, 2))


def dw_strata(i):
    if i < DW_MFMA_N:
        return dict(kernel="mfma", child=0, fs_index=i)
    kernel, k = ("dot4", i - DW_MFMA_N) if i < DW_MFMA_N + DW_DOT4_N else ("nhwc", i - DW_MFMA_N - DW_DOT4_N)
    by_call = (2 * k + k // 6) % 3 == 0
    code = EPI[(k + k // 4) % 4]
    return dict(kernel=kernel, child=None, k=(3, 3) if kernel == "dot4" else NHWC_WINDOWS[(k + k // 6) % 6], lanes=DW_LANES[k % 3],
                stride=DW_STRIDES[k % 4], dilation=2 if (k // 2 + k // 5) % 2 == 0 else 1, asym=(k // 3) % 2 == 1, by_call=by_call,
                n=(2, 3)[(k // 2) % 2] if by_call else (1, 2, 3)[(k + k // 2) % 3], code=code, exact=code >= 3,
                act=0 if code in (0, 3) else 1 + (k // 4) % 2, per_channel=(k // 2) % 2 == 1)


def _draw_dw(i, rng):
    s = dw_strata(i)   # (dot4 and nhwc; the matrix-core cases are family_sweeps' own draws)
    kh, kw_ = s["k"]
    d = s["dilation"]
    while True:
        c = 4 * int(rng.integers(2, 13))
        lo, hi = {"lt64": (1, 63), "64to256": (64, 256), "gt256": (257, 600)}[s["lanes"]]
        wos = [v for v in range(1, 80) if lo <= v * (c // 4) <= hi]
        if not wos:
            continue
        wo, ho = int(fs._pick(rng, wos)), int(rng.integers(2, 10))
        if s["asym"]:
            pad = fs._pads(rng)
            if pad[0] == pad[2] and pad[1] == pad[3]:
                continue
        else:
            pad = (int(rng.integers(0, 3)),) * 4
        h, w = _in_size(rng, ho, kh, s["stride"][0], d, pad[0], pad[2]), _in_size(rng, wo, kw_, s["stride"][1], d, pad[1], pad[3])
        if not (h and w) or s["n"] * ho * wo * c < 1024:
            continue
        return dict(depthwise=True, n=s["n"], h=h, w=w, c=c, k=(kh, kw_), stride=s["stride"], dilation=(d, d), pad=pad, act=s["act"],
                    exact=s["exact"], per_channel=s["per_channel"])


def dw_kernel_of(kw, env):
    """dwconv.hip:dwconv_i8_kernel with conv_plan.hip's packing rule (3x3: the dot4 packing) and dwconv_mfma.hip:dwconv_mfma_pick"""
    if kw.get("k", (3, 3)) != (3, 3):
        return "nhwc"
    g = fs.geometry(kw)
    sh, sw = kw.get("stride", (1, 1))
    ok = kw["c"] % 32 == 0 and sh in (1, 2) and sw in (1, 2) and kw.get("dilation", (1, 1)) == (1, 1)
    forced = env.get("SHL_MI355X_DWMFMA", "")[:1]
    if ok and forced != "0" and (forced == "1" or g["M"] * (kw["c"] >> 5) >= 80 * 1024):
        return "mfma"
    return "dot4"


# ------------------------------------------------------------------------------------------------ the interface
def strata(family, i):
    if not 0 <= i < FAMILIES[family]["n"]:
        raise IndexError("%s has %d cases" % (family, FAMILIES[family]["n"]))
    return dw_strata(i) if family == "dw_lut" else conv_strata(i)


_DRAWN = {}


def draw(family, i, seed=None):
    s = strata(family, i)
    key = (family, i, BASE_SEED if seed is None else seed)
    if key not in _DRAWN:
        if family == "dw_lut":
            _DRAWN[key] = fs.draw("dwconv_mfma", i, seed) if s["kernel"] == "mfma" else _draw_dw(i, _rng(family, i, seed))
        else:
            _DRAWN[key] = _draw_conv(family, i, _rng(family, i, seed))
    return dict(_DRAWN[key])


def child_index(family, i):
    return strata(family, i)["child"]


def case_env(family, i):
    s = strata(family, i)
    if family == "dw_lut":
        return dict(DW_CHILD_ENV) if s["child"] is not None else {}
    env = {FORM_SWITCH[POST[family]]: s["flavour"].split("/")[0]}
    if s["child"] is not None:
        env.update(child_envs()[s["child"]])
    return env


def macs(kw):
    g = fs.geometry(kw)
    kh, kw_ = kw.get("k", (3, 3))
    return g["M"] * kw["c"] * kh * kw_ * (1 if kw.get("depthwise") else kw["co"])


def in_process(family):
    return [i for i in range(FAMILIES[family]["n"]) if child_index(family, i) is None]


def chunks():
    """(family, the case indices) of every GPU test of the test process"""
    out = []
    for family in FAMILIES:
        idx = in_process(family)
        out += [(family, tuple(idx[lo:lo + CHUNK])) for lo in range(0, len(idx), CHUNK)]
    return out


def describe(family, i):
    """what a failure message needs to rebuild the case"""
    return "%s case %d: make_case(%d, **%r), SHL_TEST_FUZZ_SEED=%d, environment %r, strata %r" % (
        family, i, case_seed(family, i), draw(family, i), BASE_SEED, case_env(family, i), strata(family, i))


# ------------------------------------------------------------------------------------------------ the cases (these import the package)
TABLE_CYCLE = ("sigmoid", "hard_sigmoid", "silu", "leaky_relu", "silu_zp_min", "leaky_zp_max", "identity", "gate")


def _conv(family, i):
    """make_case of the draw; a folded relu6 gets an output record that keeps [0, 6] apart (make_case's spans three sigmas of the
    accumulator: half a unit per byte and more for deep K); a case whose call passes the batch carries the plan's batch"""
    import cases
    kw = draw(family, i)
    c = cases.make_case(case_seed(family, i), **kw)
    if kw["act"] == 2:
        c["out_scale"] = 2.0 ** -5 if kw["exact"] else float(np.float32(0.0235 * (1.0 + 0.5 * ((i * 7) % 10) / 10.0)))
        c["out_zp"] = -128 + (i * 5) % 40
    if family == "dw_lut" and kw["act"]:
        # (a depthwise channel whose bias lies far below zero stores the clamp's byte alone, and some cases have four channels)
        c["bias"] = np.abs(c["bias"])
    if strata(family, i).get("by_call"):
        c["plan_batch"] = 1
    return c


def add_case(i):
    """case i of conv_add as residual_cases.check_case takes it"""
    import residual_cases as rc
    family = "conv_add"
    s, r = strata(family, i), residual_strata(i)
    kw = draw(family, i)
    rng = np.random.default_rng([BASE_SEED + FAMILIES[family]["offset"], i, 1])
    case = rc._case("sweep_add_%03d" % i, s["flavour"].split("/")[0], kw, conv_first=r["conv_first"], act=r["act"],
                    skip_fill=r["skip_fill"], seed=case_seed(family, i) - 9100)
    case["conv"] = c = _conv(family, i)   # (the same operands: _case made them from the same seed)
    cs = float(np.float32(c["out_scale"]))
    zp = lambda v: int(rng.integers(-100, 101)) if v is None else v
    if r["pow2"]:
        base = 2.0 ** round(np.log2(cs))
        skip_s = base * 2.0 ** int(rng.integers(-1, 2))
        sum_s = base * (0.5 if r["act"] == 2 else 2.0 ** int(rng.integers(0, 2)))
        out_s = 2.0 ** -5 if r["act"] == 2 else sum_s * 2.0 ** int(rng.integers(-1, 1))
    else:
        skip_s = cs * float(rng.uniform(0.6, 1.7))
        sum_s = cs * (float(rng.uniform(0.4, 0.7)) if r["act"] == 2 else float(rng.uniform(1.0, 2.0)))
        out_s = 0.0235 * float(rng.uniform(1.0, 1.6)) if r["act"] == 2 else sum_s * float(rng.uniform(0.45, 1.0))
    if r["skip_fill"] is not None:   # (a constant skip under the convolution's own scale; in front of a relu6: three units below zero)
        skip_s = 3.0 / 128 if r["act"] == 2 else cs
        if r["act"] != 2:   # ... and a sum record with room for it next to the convolution's output
            sum_s = 2.0 * cs
            out_s = sum_s
    if r["no_fma_div"]:
        sum_s = 2.0 ** 41
    out_zp = zp(r["out_zp"]) if r["skip_fill"] is None or r["act"] != 1 else -128
    if r["act"] == 2 and out_zp != 127:
        out_zp = min(out_zp, 0)   # (room for [0, 6] above the zero point)
    f32 = lambda v: float(np.float32(v))
    case.update(skip_q=(f32(skip_s), zp(r["skip_zp"])), sum_q=(f32(sum_s), zp(r["sum_zp"])), out_q=(f32(out_s), out_zp))
    return case


def lut_cases(i):
    """case i of conv_lut as act_fuse_cases.check_case takes it: the permutation table, then one of TABLE_CYCLE, on one problem"""
    import act_fuse_cases as ac
    family = "conv_lut"
    shape = "sweep_lut_%03d" % i
    if shape not in ac._CONVS:
        ac._CONVS[shape] = _conv(family, i)
    form = strata(family, i)["flavour"].split("/")[0]
    return [dict(name=shape + "-" + t, shape=shape, form=form, table=t) for t in ("permutation", TABLE_CYCLE[i % len(TABLE_CYCLE)])]


def dw_cases(i):
    """case i of dw_lut as dw_act_cases.check_case takes it, two tables likewise"""
    import act_fuse_cases as ac
    family = "dw_lut"
    shape = "sweep_dw_%03d" % i
    if shape not in ac._CONVS:
        ac._CONVS[shape] = _conv(family, i)
    kernel = strata(family, i)["kernel"]
    return [dict(name=shape + "-" + t, shape=shape, kernel=kernel, table=t) for t in ("permutation", TABLE_CYCLE[(i + i // 8) % len(TABLE_CYCLE)])]


def forget(i, family):
    """drop the operands and the cached oracle output of a case that has run"""
    import act_fuse_cases as ac
    import dw_act_cases as dc
    shape = {"conv_lut": "sweep_lut_%03d", "dw_lut": "sweep_dw_%03d"}[family] % i
    for cache in (ac._CONVS, ac._ORACLE_CONV, dc._ORACLE):
        cache.pop(shape, None)


class CaseHip:
    """The hip library as the hand lists' run_both functions call it, for one case.  Those make the plan at the tensors' batch and
    launch with batch 0; where the case carries "plan_batch" the plan is made at that batch and every launch (and the name
    asked for) gets the tensors' own.  The flavour the fused launch reported is kept in .flavour_ran: the unfused layers
    behind it launch again"""
    BATCH_AT = {"shl_mi355x_conv_add_forward": 4, "shl_mi355x_conv_lut_forward": 3, "shl_mi355x_dwconv_lut_forward": 3,
                "shl_mi355x_conv_forward": 3, "shl_mi355x_conv_add_kernel_name": 1, "shl_mi355x_conv_lut_kernel_name": 1,
                "shl_mi355x_dwconv_lut_kernel_name": 1}

    def __init__(self, hip, conv):
        self._hip, self._plan_batch, self._batch = hip, conv.get("plan_batch"), conv["n"]
        self.flavour_ran = None

    def __getattr__(self, name):
        fn = getattr(self._hip, name)
        if self._plan_batch is not None and name == "shl_mi355x_conv_plan_create":
            def create(desc, *rest):
                desc._obj.batch = self._plan_batch   # (desc: ctypes.byref of the descriptor)
                return fn(desc, *rest)
            return create
        if name in self.BATCH_AT:
            def call(*args):
                args = list(args)
                if self._plan_batch is not None:
                    assert args[self.BATCH_AT[name]] == 0
                    args[self.BATCH_AT[name]] = self._batch
                status = fn(*args)
                if name.endswith("_lut_forward") or name.endswith("_add_forward"):
                    self.flavour_ran = self._hip.shl_mi355x_last_igemm_flavour().decode()
                return status
            return call
        return fn


def run_case(hip, opt, dev, family, i):
    """the checks of the hand lists on case i, and the flavour the fused launch reported against flavour_of's.  The caller has
    set case_env(family, i).  Whatever goes wrong -- a failed assertion, a status other than OK from an entry point -- is raised
    as an AssertionError with describe(family, i) in front"""
    import act_fuse_cases as ac
    import dw_act_cases as dc
    import residual_cases as rc
    errors = []
    if family == "conv_add":
        todo = [(add_case(i), lambda h, cs: rc.check_case(h, dev, cs, cs["form"]))]
    elif family == "conv_lut":
        todo = [(cs, lambda h, cs: ac.check_case(h, opt, dev, cs, cs["form"])) for cs in lut_cases(i)]
    else:
        todo = [(cs, lambda h, cs: dc.check_case(h, opt, dev, cs)) for cs in dw_cases(i)]
    for cs, check in todo:
        h = CaseHip(hip, cs["conv"] if family == "conv_add" else ac.conv_of(cs["shape"]))
        try:
            check(h, cs)
        except Exception as e:   # (cases.pkg.check raises RuntimeError on a status other than OK)
            errors.append("%s: %s: %s" % (cs["name"], type(e).__name__, e))
        if family != "dw_lut":
            want = flavour_of(draw(family, i), case_env(family, i), POST[family])
            if h.flavour_ran != want:
                errors.append("%s: the fused launch ran %r, flavour_of says %r" % (cs["name"], h.flavour_ran, want))
    if family != "conv_add":
        forget(i, family)
    assert not errors, describe(family, i) + "\n  " + "\n  ".join(errors)


if __name__ == "__main__":  # the child of tests/test_post_op_sweeps.py: the flavours chosen through the environment
    import cases
    from cases import pkg
    fam = sys.argv[1]
    mine = {k: v for k, v in os.environ.items() if k in ("SHL_MI355X_TILE", "SHL_MI355X_PIPE", "SHL_MI355X_DWMFMA")}
    which = 0 if fam == "dw_lut" and mine == DW_CHILD_ENV else child_envs().index(mine) if fam != "dw_lut" else None
    assert which is not None, "dw_lut's child runs under SHL_MI355X_DWMFMA=1"
    fe = pkg.load_frontend("standalone")
    hip_, opt_ = pkg.load_backend(fe)
    pkg.check(hip_.shl_mi355x_set_device(0), hip_, "set_device")
    device = cases.HipDevice(hip_)
    os.environ["SHL_MI355X_TUNE"] = "0"   # (read per plan: no timing runs at conv_plan_create)
    todo_ = [k for k in range(FAMILIES[fam]["n"]) if child_index(fam, k) == which]
    for k in todo_:
        os.environ.update(case_env(fam, k))
        run_case(hip_, opt_, device, fam, k)   # (the first failing case ends the child)
        print("ok", fam, k, flush=True)
    print("child ok", len(todo_))
    sys.exit(0)

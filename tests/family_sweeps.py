"""Seeded, stratified shape draws for the int8 kernels that a size rule (not a shape rule) turns on: the random sweeps of
test_fuzz.py & co. only meet the kernels the planner picks at small and mid sizes, these six run on hand-picked lists.
And for the NCHW-native kernels of latency-bound callers, in int8 and binary16: nchw_small.hip's pointwise kernels (staged
with transposing LDS reads, and the gather form beyond 2048 bytes of K) and depthwise 3 x 3, conv_direct.hip's binary16
stem -- families "nchw1x1", "dwconv3x3_nchw", "stem_f16_nchw"; no switch forces them, their shapes do.

  draw(family, i)        keyword arguments for cases.make_case (case i of the family)
  case_seed(family, i)   the seed of its operands
  case_env(family, i)    switches that belong to the case (beyond FAMILIES[family]["env"], the family's own)

Pure Python, no GPU, no package import: tests/test_family_sweeps.py checks the draws on any machine and runs them on
the device.  The strata (enumerated below, filled round-robin by the case index, so they hold for every seed) come
from the host code; each few lines of geometry restated here name the function they restate.  Free parameters are
random: SHL_TEST_FUZZ_SEED moves them (the idiom of test_dwpw_stream.py).

Two things the strata cannot hold, by arithmetic rather than by choice:
  * the literal dequantise-relu-requantise epilogues (epi_code 2 / 5, the latency kernel's -1) run when
    conv_plan.hip:derive_act_clamp fails.  For an output scale s in the 2^-40 .. 2^40 these kernels admit it cannot:
    x = fl(k s) and fl(x / s) differ from k by at most k 2^-23 < 1/2 for |k| <= 255, so rint returns k and the literal
    map IS the clamp.  The draws reach epi_code 0, 1, 3, 4 and the latency kernel's 0 and 3.
  * conv1x1_resident: resident_geom halves the ranges until a workgroup has at least three tiles, so below the full
    grid (one workgroup per CU) a workgroup has at most six; the full grid costs tiles x 1.07e9 MACs.  Under the cap
    of 2e9 the longest run is therefore 6 tiles = 12 stages at K = 1024: every slot of the six-slot ring is used
    twice (reused once), the issue's 13th stage -- a second reuse -- is out of reach.
"""
import os

import numpy as np

BASE_SEED = int(os.environ.get("SHL_TEST_FUZZ_SEED", "20261018"))  # (a one-off run elsewhere: set the variable)

FAMILIES = {
    # the rival pointwise rules are switched off where a forced kernel would otherwise share shapes with them: the plan
    # NAMES stream -> resident -> latency (the last one wins), the launch ASKS resident -> latency -> stream
    "dwconv_mfma": dict(n=40, offset=100, cap=1e9, env={"SHL_MI355X_DWMFMA": "1"}),
    "conv1x1_stream": dict(n=32, offset=200, cap=1e9,
                           env={"SHL_MI355X_PWSTREAM": "1", "SHL_MI355X_PWRES": "0", "SHL_MI355X_PWLAT": "0"}),
    "conv1x1_resident": dict(n=32, offset=300, cap=2e9, chunk=4, env={"SHL_MI355X_PWRES": "1", "SHL_MI355X_PWLAT": "0"}),
    "conv1x1_latency": dict(n=32, offset=400, cap=1e9, env={"SHL_MI355X_PWLAT": "1"}),
    "stem_mfma": dict(n=32, offset=500, cap=1e9, env={"SHL_MI355X_STEM_MFMA": "1"}),
    "conv_gemv": dict(n=32, offset=600, cap=1e9, env={}),
    # the NCHW-native kernels: latency-sized cases (the cap keeps the CPU oracle under about a second each)
    "nchw1x1": dict(n=48, offset=700, cap=2e8, env={}),
    "dwconv3x3_nchw": dict(n=32, offset=800, cap=2e8, env={}),
    "stem_f16_nchw": dict(n=16, offset=900, cap=2e8, env={}),
}
NCHW_NATIVE = ("nchw1x1", "dwconv3x3_nchw", "stem_f16_nchw")   # binary16 cases of these compare bit for bit
CHUNK = 8   # cases per GPU test (conv1x1_resident: 4, its cases are up to 1.8 GMAC of oracle each)
# switches a case may carry; the sub-process clears them between cases.  All are read per call but SHL_MI355X_STEM_TPW
# (once per process): the stem's chunks are therefore uniform in it.
CASE_SWITCHES = ("SHL_MI355X_PWLAT_SPLIT", "SHL_MI355X_GEMV_OPW", "SHL_MI355X_STEM_TPW")


def out_size(i, k, s, p0, p1, d=1):
    return (i + p0 + p1 - d * (k - 1) - 1) // s + 1


def case_seed(family, i):
    return 910000 + FAMILIES[family]["offset"] * 10 + i


def _rng(family, i, seed):
    return np.random.default_rng([(BASE_SEED if seed is None else seed) + FAMILIES[family]["offset"], i])


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _pads(rng):
    return tuple(int(v) for v in rng.integers(0, 3, 4))  # (top, left, bottom, right), each of {0, 1, 2}


def _in_size_for(rng, out, stride, p0, p1, d=1):
    """an input extent whose 3-tap output extent (dilation d) is `out` (None: the padding alone is already too much)"""
    v = (out - 1) * stride + 2 * d + 1 - p0 - p1 + int(rng.integers(0, stride))
    return v if v >= 1 and out_size(v, 3, stride, p0, p1, d) == out else None


def geometry(kw):
    """n, ho, wo, M, the MACs and the layout of a make_case keyword set"""
    if kw.get("fc"):
        n, ho, wo = kw["n"], 1, 1
        kh = kw_ = 1
    else:
        kh, kw_ = kw.get("k", (3, 3))
        pad, st, dil = kw.get("pad", (1, 1, 1, 1)), kw.get("stride", (1, 1)), kw.get("dilation", (1, 1))
        n = kw.get("n", 1)
        ho, wo = out_size(kw["h"], kh, st[0], pad[0], pad[2], dil[0]), out_size(kw["w"], kw_, st[1], pad[1], pad[3], dil[1])
    M = n * ho * wo
    macs = M * kw["c"] * 9 if kw.get("depthwise") else M * kw["c"] * kw["co"] * kh * kw_
    return dict(n=n, ho=ho, wo=wo, M=M, macs=macs, layout="NHWC" if kw.get("fc") else kw.get("layout", "NHWC"))


def epi_code(kw):
    """common.h:epi_code with conv_plan.hip's flags for make_case's records: div_exact <=> power-of-two scales ("exact"),
    the activation always as a clamp (module docstring)"""
    return (3 if kw.get("exact", True) else 0) + (1 if kw.get("act", 0) else 0)


# ------------------------------------------------------------------------------------------------ dwconv_mfma
DW_C = {32: (32, 96, 160), 64: (64, 192, 320), 128: (128, 256, 384, 512)}
DW_STRIDES = ((1, 1), (2, 2), (2, 1), (1, 2))
DW_PAIRS = [(cb, s) for cb in (32, 64, 128) for s in DW_STRIDES]
DW_WO = {"le8": (1, 8), "9to16": (9, 16), "gt16": (17, 40)}
DW_HO = {"le4": (1, 4), "5to8": (5, 8), "ge9": (9, 24)}
DW_CLASSES = [(a, b) for a in DW_WO for b in DW_HO]


def dw_strata(i):
    """the (cb, stride) pair cycles with i % 12; the map classes are shifted by the round i // 12, so that a pair meets a new Ho
    class and a new Wo class in every round (cycles of 12 and 9 alone share i % 3: the Ho class would be a function of the pair)"""
    p, k = i % 12, i // 12
    cb, stride = DW_PAIRS[p]
    hoc = list(DW_HO)[(p + 2 + k) % 3]
    woc = list(DW_WO)[(p // 3 + p + 2 * k) % 3]
    return dict(cb=cb, stride=stride, wo_class=woc, ho_class=hoc, round=k)


def dwm_geometry(C, sh, sw, Ho, Wo):
    """dwconv_mfma.hip:dwm_geometry"""
    cb = 128 if C % 128 == 0 else (64 if C % 64 == 0 else 32)
    btx = 1 if Wo <= 8 else 2
    s1 = sh == 1 and sw == 1
    bty0 = (4 if cb <= 32 else 2) if s1 else (2 if cb <= 64 else 1)
    bty = bty0
    while bty > 1 and (bty - 1) * 4 >= Ho:
        bty -= 1
    return dict(cb=cb, btx=btx, bty0=bty0, bty=bty, tiles_x=(Wo + btx * 8 - 1) // (btx * 8), tiles_y=(Ho + bty * 4 - 1) // (bty * 4))


def _draw_dw(i, rng):
    s = dw_strata(i)
    sh, sw = s["stride"]
    wo, ho = int(rng.integers(*DW_WO[s["wo_class"]], endpoint=True)), int(rng.integers(*DW_HO[s["ho_class"]], endpoint=True))
    if s["cb"] == 32 and s["stride"] == (1, 1) and s["ho_class"] == "ge9":
        # the one pair that starts at four rows of tiles: 9 .. 12 output rows launch three of them, more launch all four
        ho = int(rng.integers(9, 13)) if s["round"] == 0 else int(rng.integers(13, 25))
    while True:
        pad = _pads(rng)
        h, w = _in_size_for(rng, ho, sh, pad[0], pad[2]), _in_size_for(rng, wo, sw, pad[1], pad[3])
        if h and w:
            break
    return dict(depthwise=True, c=int(_pick(rng, DW_C[s["cb"]])), h=h, w=w, n=int(rng.integers(1, 6)), stride=(sh, sw), pad=pad,
                act=(i // 2) % 3, exact=i % 2 == 0, per_channel=(i // 6) % 2 == 1)


# ------------------------------------------------------------------------------------------------ conv1x1_stream
ST_C = (32, 64, 128, 256, 512)
ST_PAIRS = [(c, ncg) for c in ST_C for ncg in (4, 2)]
ST_CO = {4: (128, 256, 384, 512), 2: (64, 192, 320)}   # Co % 128 == 0: four channel groups per workgroup, % 128 == 64: two


def stream_tile(c):
    """conv1x1_stream.hip:launch_conv1x1_stream: mt * 32 pixels per workgroup"""
    return 96 if c == 512 else 192


def stream_strata(i):
    """-> C, NCG, M % T (None: the case with M < T)"""
    if i < 5:
        return dict(c=ST_C[i], ncg=(4, 2)[i % 2], res=None)
    j = i - 5
    c, ncg = ST_PAIRS[j % 10]
    T = stream_tile(c)
    # (shifted by the round j // 10: pairs and residues alone share j % 2, a channel-group count would meet half the residues)
    return dict(c=c, ncg=ncg, res=(0, 1, 31, 32, 33, T - 1)[(j + j // 10) % 6])


def _map_with(rng, ok, nmax=6, smax=48):
    """n > 1 images of a non-square map whose pixel count satisfies ok()"""
    while True:
        n, h, w = rng.integers(2, nmax + 1, 4096), rng.integers(1, smax + 1, 4096), rng.integers(1, smax + 1, 4096)
        for a, b, c in zip(n.tolist(), h.tolist(), w.tolist()):
            if b != c and ok(a * b * c):
                return a, b, c


def _draw_stream(i, rng):
    s = stream_strata(i)
    c, T = s["c"], stream_tile(s["c"])
    co = int(_pick(rng, ST_CO[s["ncg"]]))
    mmax = max(4 * T, min(6000, int(2.5e8 / (c * co))))  # (the oracle's time, not the cap, sets the size)
    if s["res"] is None:
        n, h, w = _map_with(rng, lambda m: m < T)
    else:
        n, h, w = _map_with(rng, lambda m: T <= m <= mmax and m % T == s["res"])
    return dict(c=c, co=co, h=h, w=w, n=n, k=(1, 1), pad=(0, 0, 0, 0), act=int(rng.integers(0, 3)), exact=bool(rng.integers(0, 2)),
                per_channel=bool(rng.integers(0, 2)))


# ------------------------------------------------------------------------------------------------ conv1x1_resident
RS_PAIRS = [(c, co) for c in (128, 256, 512, 1024) for co in (256, 512, 1024, 2048)]
RS_MODES = ("exact3", "plus1", "ragged", "long")
RS_LAST = (1, 31, 32, 33, "full")
RS_SOFT = 1.0e9   # MACs of a case with more than 8 ranges (the oracle's time; 8 ranges: the family's cap)


def resident_tile(c):
    return 32 if c >= 512 else 32 * (512 // c)


def resident_geom(M, C, Co):
    """conv1x1_resident.hip:resident_geom -> (channel blocks, ranges, tiles) or None; the kernel gives range g the tiles
    [tiles g / ranges, tiles (g + 1) / ranges)"""
    nb = Co // 256
    if nb < 1 or nb > 32 or 32 % nb:
        return None
    tpx = resident_tile(C)
    tiles = (M + tpx - 1) // tpx
    r = 256 // nb
    while r > 8 and tiles < 3 * r:
        r >>= 1
    if tiles < 3 * r or (r * nb) % 8 or ((r * nb) // 8) % nb:
        return None
    return nb, r, tiles


def resident_range_tiles(tiles, ranges):
    return [tiles * (g + 1) // ranges - tiles * g // ranges for g in range(ranges)]


def resident_strata(i):
    p, k = i % 16, i // 16
    c, co = RS_PAIRS[p]
    mode = RS_MODES[(p // 4 + p % 4 + 2 * k) % 4]
    last = RS_LAST[(p + 3 * k) % 5]
    if last == 33 and resident_tile(c) <= 32:
        last = "full"
    # ranges asked for: 64 / 32 / 16 / 8 by the channel-block count in the first round, half of that in the second; _draw_resident
    # halves it further until the case fits RS_SOFT
    want = max(8, (64 >> (p % 4)) >> k)
    return dict(c=c, co=co, mode=mode, last=last, ranges=want)


def _resident_tiles(rng, mode, r, max_tiles):
    """a tile count that resident_geom turns into r ranges (3 r <= tiles < 6 r) in the given mode, or None above max_tiles"""
    if mode == "exact3":
        pick = [3 * r]
    elif mode == "plus1":
        pick = [3 * r + 1]
    elif mode == "ragged":
        pick = [t for t in range(3 * r + 2, 6 * r) if t % r and t <= max_tiles]
    else:  # some workgroup with six tiles
        pick = [t for t in range(5 * r + 1, 6 * r) if t <= max_tiles]
    pick = [t for t in pick if t <= max_tiles]
    return int(_pick(rng, pick)) if pick else None


def _draw_resident(i, rng):
    s = resident_strata(i)
    c, co, tpx = s["c"], s["co"], resident_tile(s["c"])
    cap_tiles = int(FAMILIES["conv1x1_resident"]["cap"] // (tpx * c * co))
    r, tiles = s["ranges"], None
    while tiles is None and r > 8:
        tiles = _resident_tiles(rng, s["mode"], r, int(RS_SOFT // (tpx * c * co)))
        r = r if tiles else r >> 1
    if tiles is None:  # 8 ranges: 24 <= tiles < 48
        tiles = _resident_tiles(rng, s["mode"], 8, cap_tiles) or min(47, cap_tiles)  # (six tiles, or as many as the cap allows)
    last = tpx if s["last"] == "full" else s["last"]
    M = (tiles - 1) * tpx + last
    # M = n h w, n > 1 where M allows it
    facs = [(n, h, M // (n * h)) for n in range(1, 65) for h in range(1, 65) if M % (n * h) == 0]
    best = [f for f in facs if f[0] > 1 and f[1] != f[2] and f[1] > 1 and f[2] > 1] or [f for f in facs if f[0] > 1] or facs
    n, h, w = _pick(rng, best)
    return dict(c=c, co=co, h=int(h), w=int(w), n=int(n), k=(1, 1), pad=(0, 0, 0, 0), act=i % 3, exact=(i // 3) % 2 == 0,
                per_channel=bool(rng.integers(0, 2)))


# ------------------------------------------------------------------------------------------------ conv1x1_latency
LAT_FORMS = ("mt1", "zsplit", "mt2")
LAT_HW = {1: (1, 1), 31: (1, 31), 32: (4, 8), 33: (3, 11), 63: (7, 9), 64: (4, 16)}


def latency_form(kw, env):
    """conv1x1_latency.hip:launch_lat without the pooling"""
    g = geometry(kw)
    hw = g["ho"] * g["wo"]
    if hw <= 32:
        return "mt1"
    if (kw["co"] >> 5) * g["n"] * 2 <= 256 and env.get("SHL_MI355X_PWLAT_SPLIT") != "0":
        return "zsplit"
    return "mt2"


def latency_strata(i):
    form = LAT_FORMS[i % 3]
    r = i // 3  # 0 .. 10
    if form == "mt1":
        hw = (1, 31, 32, None)[r % 4]
    else:
        hw = (33, 63, 64, None)[r % 4]
    return dict(form=form, hw=hw, c=(256, 512, 1024)[r % 3], by_switch=form == "mt2" and r % 2 == 1)


def _draw_latency(i, rng):
    s = latency_strata(i)
    lo, hi = (1, 32) if s["form"] == "mt1" else (33, 64)
    if s["hw"] is None:
        while True:
            h, w = int(rng.integers(1, 65)), int(rng.integers(1, 65))
            if h != w and lo <= h * w <= hi:
                break
    else:
        h, w = LAT_HW[s["hw"]]
        if rng.integers(0, 2):
            h, w = w, h
    while True:
        if s["form"] == "mt2" and not s["by_switch"]:
            co, n = _pick(rng, ((576, 8), (1024, 5), (1024, 7), (2048, 3), (2048, 4)))
        elif s["form"] == "mt1":  # one tile whatever the batch: both ends of N = 1 .. 8 are set, not drawn
            co = int(_pick(rng, (32, 64, 96, 160, 256, 512)))
            n = {0: 1, 1: 8}.get((i // 3) % 4) or int(rng.integers(1, 9))
        else:
            co = int(_pick(rng, (32, 64, 96, 160, 256, 512)))
            n = int(rng.integers(1, min(8, 128 // (co >> 5)) + 1))
        if n * h * w * s["c"] * co <= 4e8:
            break
    return dict(c=s["c"], co=int(co), h=h, w=w, n=int(n), k=(1, 1), pad=(0, 0, 0, 0), act=(i // 2) % 3, exact=i % 2 == 0,
                per_channel=bool(rng.integers(0, 2)))


# ------------------------------------------------------------------------------------------------ the stem on the matrix cores
STEM_TPW = (1, 2, 3, 8)        # one per chunk of eight: the switch is read once per process
STEM_CO = (16, 32, 48, 64)
STEM_STRIDES = ((1, 1), (2, 2), (1, 2), (2, 1))
STEM_TINY = ((1, 2, 2), (1, 1, 4), (1, 4, 1), (2, 3, 3))   # n, h, w: the 12-byte pieces cross the tensor's first or last byte
# no override: conv_stem.hip:launch_conv_stem sets tiles / 8192 = 2 tiles per wave from 524 288 output pixels
STEM_RULE_CASE = dict(c=3, co=32, n=2, h=1024, w=1024, stride=(2, 2))


def stem_launch(M, tpw):
    """conv_stem.hip:launch_conv_stem, MFMA branch -> tiles, tiles per wave, waves"""
    tiles = (M + 31) // 32
    if tpw is None:
        tpw = min(max(tiles // (256 * 4 * 8), 1), 8)
    return tiles, tpw, (tiles + tpw - 1) // tpw


def stem_strata(i):
    return dict(tpw=STEM_TPW[i // 8], tiny=STEM_TINY[i // 8] if i % 8 == 0 else None, co=STEM_CO[i % 4],
                stride=STEM_STRIDES[(i // 4 + i) % 4])


def _draw_stem(i, rng):
    s = stem_strata(i)
    sh, sw = s["stride"]
    while True:
        pad = (2, 2, 2, 2) if s["tiny"] == (2, 3, 3) else _pads(rng)
        if s["tiny"]:
            n, h, w = s["tiny"]
        else:
            n, h, w = int(rng.integers(1, 4)), int(rng.integers(5, 49)), int(rng.integers(5, 49))
        ho, wo = out_size(h, 3, sh, pad[0], pad[2]), out_size(w, 3, sw, pad[1], pad[3])
        if ho < 1 or wo < 1:
            continue
        if s["tiny"]:
            break
        tiles, tpw, waves = stem_launch(n * ho * wo, s["tpw"])
        # the pipeline loop runs, the last wave is ragged, the last workgroup is not full
        if tiles > tpw and (tpw == 1 or tiles % tpw) and waves % 4 and (n * ho * wo) % 32:
            break
    return dict(c=3, co=s["co"], n=n, h=h, w=w, stride=(sh, sw), pad=pad, act=(i // 2) % 3, exact=i % 2 == 0,
                per_channel=bool(rng.integers(0, 2)))


# ------------------------------------------------------------------------------------------------ conv_gemv
GV_KBYTES = (16, 48, 1008, 1024, 1040, 2048, 4112)   # the K loop walks 1-KiB chunks, 16 bytes per lane
GV_CO = (1, 2, 3, 4, 5, 7, 8, 9, 255, 257, 1000, 2049)


def gemv_opw(kw, env):
    """conv_gemv.hip:launch_conv_gemv"""
    two = (kw["co"] + 7) // 8 * geometry(kw)["M"] <= 256 and env.get("SHL_MI355X_GEMV_OPW") != "4"
    return 2 if two else 4


def gemv_strata(i):
    return dict(kbytes=GV_KBYTES[i % 7], co=GV_CO[i % 12], dtype="int8" if (i + i // 12) % 2 == 0 else "f16", fc=(i // 2) % 2 == 0, opw4=i < 7)


def _draw_gemv(i, rng):
    s = gemv_strata(i)
    kw = dict(dtype=s["dtype"], c=s["kbytes"] // (1 if s["dtype"] == "int8" else 2), co=s["co"])
    if s["fc"]:
        kw.update(fc=True, n=int(rng.integers(1, 9)))
    else:
        n, h, w = _pick(rng, [(a, b, c) for a in (1, 2, 3) for b in (1, 2, 3, 4) for c in (1, 2, 3, 4) if a * b * c <= 8])
        kw.update(n=n, h=h, w=w, k=(1, 1), pad=(0, 0, 0, 0), act=int(rng.integers(0, 3)))
    if s["dtype"] == "int8":
        kw.update(exact=bool(rng.integers(0, 2)), per_channel=bool(rng.integers(0, 2)))
    return kw


# ------------------------------------------------------------------------------------------------ nchw1x1
NC_KBYTES = (16, 48, 96, 192, 320, 512, 576, 1024, 1040, 2048, 2080, 4096, 4112)
NC_CO = (1, 3, 5, 8, 31, 32, 36, 61, 64, 70, 160)
# (K row bytes, Co or None: the Co cycle) of case j = i // 2 of either dtype: every row of the table once, then the rows again
# that make each of staged / gather x fragment-ordered / row-ordered weights appear at least twice per dtype
NC_PLAN = ((16, None), (48, None), (96, None), (192, None), (320, None), (512, None), (576, None), (1024, None), (1040, None),
           (2048, 64), (2080, None), (4096, 32), (4112, None), (4096, 160), (2048, None), (1024, 160), (512, 32), (192, 64),
           (576, None), (1040, None), (320, None), (96, None), (48, None), (2080, None))
NC_HW = ("tiny", "lt16", "r0", "r1to15", "r16", "r17to31", "big_aligned", "big_odd", "r0_tiles")
NC_HW_SETS = {"lt16": (3, 5, 7, 9, 11, 13, 15), "r0": (32, 64), "r1to15": (33, 35, 37, 39, 42, 45, 47), "r16": (16, 48, 80),
              "r17to31": (17, 21, 27, 31, 49, 51, 55, 57, 63), "big_aligned": (112, 128, 144, 160, 176, 208),
              "big_odd": (101, 105, 117, 135, 143, 165, 187, 201), "r0_tiles": (64, 96, 128)}


def align_up(v, a):
    return (v + a - 1) // a * a


def nchw1x1_launch(kbytes, co=None):
    """nchw_small.hip:launch_conv1x1_nchw for a K row of kbytes = C * esize (and conv_plan.hip's fragment-ordered weight copy
    together with the kernels' own test for it, when co is given)"""
    kstride = align_up(kbytes, 64)
    nsub = kstride // 32
    waves = 16 if nsub >= 32 else (8 if nsub >= 16 else 4)
    per = (nsub + waves - 1) // waves
    out = dict(kstride=kstride, nsub=nsub, waves=waves, per=per, staged=waves * per * 1024 <= 65536,
               # the 32-byte sub-steps each wave walks (negative before the kernels' clamp: its start lies beyond the end)
               wave_nsub=[min(per, nsub - w * per) for w in range(waves)])
    if co is not None:
        out["frag"] = kbytes % 64 == 0 and kbytes <= 4096 and co % 32 == 0
    return out


def nchw1x1_strata(i):
    j = i // 2
    kb, co = NC_PLAN[j]
    f16 = i % 2 == 1
    if co is None:
        co = NC_CO[(j + (5 if f16 else 0)) % 11]
    return dict(dtype="f16" if f16 else "int8", kbytes=kb, co=co, hw_class=NC_HW[i % 9], n=1 + (i + i // 9) % 3)


def _factor(rng, hw):
    """h, w with h * w = hw, not square where hw allows it"""
    pairs = [(a, hw // a) for a in range(1, hw + 1) if hw % a == 0]
    return _pick(rng, [p for p in pairs if p[0] != p[1] and min(p) > 1] or [p for p in pairs if p[0] != p[1]] or pairs)


def _draw_nchw1x1(i, rng):
    s = nchw1x1_strata(i)
    es = 1 if s["dtype"] == "int8" else 2
    c, co, n = s["kbytes"] // es, s["co"], s["n"]
    if s["hw_class"] == "tiny":  # N * HW <= 8 on more than one pixel: the NHWC view of this shape is the GEMV's
        hw = int(rng.integers(2, 8 // n + 1))
    else:
        fits = [v for v in NC_HW_SETS[s["hw_class"]] if n * v * c * co <= FAMILIES["nchw1x1"]["cap"]]
        hw = int(_pick(rng, fits))
    h, w = _factor(rng, hw)
    kw = dict(layout="NCHW", dtype=s["dtype"], c=c, co=co, n=n, h=int(h), w=int(w), k=(1, 1), pad=(0, 0, 0, 0), act=i % 3)
    if es == 1:
        kw.update(exact=(i // 2) % 2 == 0, per_channel=bool(rng.integers(0, 2)))
    return kw


def exact_f16_operands(case):
    """binary16 operands whose fp32 sums are exact in any order (the MFMA's is not the reference's): input, kernel and bias become
    multiples of 2^-4 in [-2, 2], seeded by the case.  Every product is a multiple of 2^-8 of magnitude <= 4, so a partial sum over
    K <= 2^14 terms is a multiple of 2^-8 below 2^16: 24 bits.  (The device of deconv_cases.py.)"""
    rng = np.random.default_rng([int(case["seed"]), 16])
    for key, shape in (("input", case["in_shape"]), ("kernel", case["w_shape"]), ("bias", (case["co"],))):
        case[key] = (rng.integers(-32, 33, shape) / 16.0).astype(np.float16)
    return case


# ------------------------------------------------------------------------------------------------ dwconv3x3_nchw
DN_STRIDES = ((1, 1), (2, 2), (1, 2), (3, 2))
DN_DILATIONS = ((1, 1), (2, 2), (1, 1), (1, 2), (1, 1))
DN_C = (2, 3, 19, 32, 100)
DN_MAP = ("lt256", "eq256", "257to511", "gt512")   # Ho * Wo: one block row, a full one, a ragged second one, three and more


def dwn_strata(i):
    return dict(stride=DN_STRIDES[i % 4], dilation=DN_DILATIONS[i % 5], c=DN_C[(i // 2) % 5], n=1 + i % 3, map_class=DN_MAP[(i // 4) % 4],
                line=i == 0, dtype="int8" if (i + i // 8) % 2 == 0 else "f16")


def _draw_dwn(i, rng):
    s = dwn_strata(i)
    (sh, sw), (dh, dw) = s["stride"], s["dilation"]
    while True:
        if s["line"]:
            ho, wo = _pick(rng, ((1, int(rng.integers(9, 40))), (int(rng.integers(9, 40)), 1)))
        elif s["map_class"] == "eq256":
            ho, wo = _pick(rng, ((8, 32), (32, 8), (4, 64), (64, 4), (2, 128), (16, 16)))
        else:
            lo, hi = {"lt256": (2, 255), "257to511": (257, 511), "gt512": (513, 1100)}[s["map_class"]]
            ho, wo = int(rng.integers(2, 48)), int(rng.integers(2, 48))
            if ho == wo or not lo <= ho * wo <= hi:
                continue
        pad = _pads(rng)
        h, w = _in_size_for(rng, ho, sh, pad[0], pad[2], dh), _in_size_for(rng, wo, sw, pad[1], pad[3], dw)
        if h and w:
            break
    kw = dict(layout="NCHW", dtype=s["dtype"], depthwise=True, c=s["c"], n=s["n"], h=h, w=w, stride=(sh, sw), dilation=(dh, dw),
              pad=pad, act=(i // 2) % 3)
    if s["dtype"] == "int8":
        kw.update(exact=(i // 2) % 2 == 0, per_channel=bool(rng.integers(0, 2)))
    return kw


# ------------------------------------------------------------------------------------------------ stem_f16_nchw
SN_CO = (1, 7, 8, 20, 33, 64)
SN_STRIDES = ((1, 1), (2, 2), (2, 1))


def stem_f16_threads(kw):
    """conv_direct.hip:launch_conv_direct: one thread per (image, group of eight output channels, output pixel), 256 per workgroup"""
    g = geometry(kw)
    return g["n"] * ((kw["co"] + 7) // 8) * g["ho"] * g["wo"]


def stemn_strata(i):
    return dict(co=SN_CO[i % 6], stride=SN_STRIDES[(i + i // 6) % 3], dilation=((1, 1), (2, 2))[(i // 4) % 2], n=1 + (i // 3) % 3,
                one_group=i % 2 == 0, act=(i // 2) % 2)


def _draw_stemn(i, rng):
    s = stemn_strata(i)
    (sh, sw), (dh, dw) = s["stride"], s["dilation"]
    while True:
        ho, wo = (int(rng.integers(1, 8)), int(rng.integers(1, 8))) if s["one_group"] else (int(rng.integers(3, 24)), int(rng.integers(3, 24)))
        pad = _pads(rng)
        h, w = _in_size_for(rng, ho, sh, pad[0], pad[2], dh), _in_size_for(rng, wo, sw, pad[1], pad[3], dw)
        if not (h and w) or ho == wo:
            continue
        kw = dict(layout="NCHW", dtype="f16", c=3, co=s["co"], n=s["n"], h=h, w=w, stride=(sh, sw), dilation=(dh, dw), pad=pad, act=s["act"])
        t = stem_f16_threads(kw)
        # one workgroup that is not full, or several with a ragged last one (the gid >= total clamp)
        if (t < 256) if s["one_group"] else (t >= 257 and t % 256):
            return kw


_DRAW = {"dwconv_mfma": _draw_dw, "conv1x1_stream": _draw_stream, "conv1x1_resident": _draw_resident,
         "conv1x1_latency": _draw_latency, "stem_mfma": _draw_stem, "conv_gemv": _draw_gemv,
         "nchw1x1": _draw_nchw1x1, "dwconv3x3_nchw": _draw_dwn, "stem_f16_nchw": _draw_stemn}


def draw(family, i, seed=None):
    if not 0 <= i < FAMILIES[family]["n"]:
        raise IndexError("%s has %d cases" % (family, FAMILIES[family]["n"]))
    return _DRAW[family](i, _rng(family, i, seed))


def case_env(family, i):
    if family == "conv1x1_latency" and latency_strata(i)["by_switch"]:
        return {"SHL_MI355X_PWLAT_SPLIT": "0"}
    if family == "stem_mfma":
        return {"SHL_MI355X_STEM_TPW": str(stem_strata(i)["tpw"])}
    if family == "conv_gemv" and gemv_strata(i)["opw4"]:
        return {"SHL_MI355X_GEMV_OPW": "4"}
    return {}


def kernel_name(family, kw):
    f16 = kw.get("dtype", "int8") != "int8"
    if family == "nchw1x1":
        return "conv1x1_nchw_f16" if f16 else "conv1x1_nchw_i8"
    if family == "dwconv3x3_nchw":
        return "dwconv3x3_nchw_f16" if f16 else "dwconv3x3_nchw_i8"
    if family == "stem_f16_nchw":   # (the plan's name for every binary16 direct kernel: admissible() restates which one the launch takes)
        return "conv_direct_f16"
    return {"dwconv_mfma": "dwconv_mfma_i8", "conv1x1_stream": "conv1x1_stream_i8_mfma32x32x32",
            "conv1x1_resident": "conv1x1_resident_i8_mfma32x32x32", "conv1x1_latency": "conv1x1_latency_i8_mfma32x32x32",
            "stem_mfma": "conv_stem_i8_mfma32x32x32",
            "conv_gemv": "conv_gemv_i8_dot4" if kw.get("dtype", "int8") == "int8" else "conv_gemv_f16_fma"}[family]


def _pointwise(kw):
    return kw.get("k") == (1, 1) and kw.get("pad") == (0, 0, 0, 0) and kw.get("stride", (1, 1)) == (1, 1)


def admissible(family, kw):
    """the family's pick condition with its switch at "1" (and its rivals as FAMILIES[family]["env"] sets them), for an int8 /
    binary16 make_case keyword set (NHWC; the three NCHW-native families: NCHW)"""
    g = geometry(kw)
    i8 = kw.get("dtype", "int8") == "int8"
    if family == "nchw1x1":  # conv_igemm.hip:igemm_supports, igemm_variant + nchw_small.hip:conv1x1_nchw_eligible; a 1 x 1 map goes to the NHWC kernels
        hw = kw["h"] * kw["w"]
        return bool(g["layout"] == "NCHW" and not kw.get("depthwise") and _pointwise(kw) and (kw["c"] * (1 if i8 else 2)) % 16 == 0 and
                    ((g["M"] + 127) // 128) * ((kw["co"] + 127) // 128) < 128 and g["n"] * ((hw + 31) // 32) <= 65535 and hw >= 2)
    if family == "dwconv3x3_nchw":  # nchw_small.hip:dwconv_nchw_supports (make_case's zero point is -5); the dilated kernel fits the padded image
        return bool(g["layout"] == "NCHW" and kw.get("depthwise") and kw.get("multiplier", 1) == 1 and kw["c"] > 1 and
                    kw.get("k", (3, 3)) == (3, 3) and g["ho"] >= 1 and g["wo"] >= 1 and g["ho"] * g["wo"] <= 65535 * 256 and g["n"] * kw["c"] < 2 ** 31)
    if family == "stem_f16_nchw":  # conv_direct.hip:launch_conv_direct (conv_plan.hip:choose_algo: 6 bytes of K are no implicit GEMM's)
        return bool(g["layout"] == "NCHW" and not i8 and not kw.get("depthwise") and kw.get("groups", 1) == 1 and kw["c"] == 3 and
                    kw.get("k", (3, 3)) == (3, 3) and kw["co"] <= 64 and g["ho"] >= 1 and g["wo"] >= 1 and
                    (stem_f16_threads(kw) + 255) // 256 < 2 ** 31 - 1)
    if family == "dwconv_mfma":  # conv_plan.hip (3x3, dilation 1, dot4 packing: C % 4) + dwconv_mfma.hip:dwconv_mfma_pick, dwm_geometry
        sh, sw = kw["stride"]
        return bool(i8 and kw.get("depthwise") and kw["c"] % 32 == 0 and sh in (1, 2) and sw in (1, 2) and g["ho"] >= 1 and g["wo"] >= 1 and
                    kw["h"] * kw["w"] * kw["c"] < 2 ** 31 and dwm_geometry(kw["c"], sh, sw, g["ho"], g["wo"])["tiles_y"] * g["n"] <= 65535)
    if family == "conv1x1_stream":  # conv1x1_stream.hip:conv1x1_stream_pick
        return bool(i8 and _pointwise(kw) and kw["c"] in ST_C and kw["co"] % 64 == 0 and (g["M"] + 95) // 96 <= 65535)
    if family == "conv1x1_resident":  # conv1x1_resident.hip:conv1x1_resident_pick
        return bool(i8 and _pointwise(kw) and kw["c"] in (128, 256, 512, 1024) and kw["co"] % 256 == 0 and
                    resident_geom(g["M"], kw["c"], kw["co"]) is not None)
    if family == "conv1x1_latency":  # conv1x1_latency.hip:lat_shape
        return bool(i8 and _pointwise(kw) and kw["c"] in (256, 512, 1024) and kw["co"] % 32 == 0 and 1 <= g["ho"] * g["wo"] <= 64 and
                    1 <= g["n"] <= 65535)
    if family == "stem_mfma":  # conv_stem.hip:stem_supports, stem_mfma_pick
        return bool(i8 and kw["c"] == 3 and kw.get("k", (3, 3)) == (3, 3) and kw["co"] % 16 == 0 and kw["co"] <= 64 and g["M"] < 2 ** 22 and
                    12 <= g["n"] * kw["h"] * kw["w"] * 3 < 2 ** 31 - 16 and g["M"] >= 1)
    if family == "conv_gemv":  # conv_gemv.hip:conv_gemv_pick; no pointwise form of its own may take the layer first (Co % 32 != 0)
        return bool((kw.get("fc") or _pointwise(kw)) and 1 <= g["M"] <= 8 and (kw["c"] * (1 if i8 else 2)) % 16 == 0 and kw["co"] % 32 != 0)
    raise KeyError(family)


def chunks():
    """(family, first case) of every GPU test"""
    return [(f, lo) for f in FAMILIES for lo in range(0, FAMILIES[f]["n"], FAMILIES[f].get("chunk", CHUNK))]

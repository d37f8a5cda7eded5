"""Seeded, stratified draws for the fused PAIR kernels -- two layers in one launch -- that the hand-picked lists of test_fusion.py,
test_pwdw_fuzz.py and test_pwdw_window.py reach with square maps, isotropic strides, one intermediate zero point and the same
`exact` flag on both layers:

  "pwdw_i8"          pwdw_fused.hip        pointwise 1 x 1 + the depthwise 3 x 3 consuming it, int8 NHWC      64 cases
  "stemdw_i8"        stemdw_fused.hip      the 3 -> 32 stem + the depthwise 3 x 3 consuming it, int8 NHWC      32 cases
  "stemdw_f16_nchw"  stemdw_f16_nchw.hip   the 3 -> Co <= 32 stem + depthwise 3 x 3, binary16 NCHW             24 cases

  draw(family, i)        dict(first=<make_case keywords>, second=<make_case keywords>, zp=<intermediate zero point | None>)
  case_seed(family, i)   the seed of the first layer's operands (the second layer's: + SECOND_SEED)
  case_env(family, i)    switches that belong to the case
  admissible(family, pair, env)   the launch's own admission rule, restated
  strata(family, i)      what the index alone fixes

The contract of family_sweeps.py: pure Python, no GPU, no package import.  The strata are filled round-robin by the case index,
so they hold for every seed; SHL_TEST_FUZZ_SEED moves the free parameters.  Where a stratum is a property of the geometry the
library chooses (choose_rect's grid, the XCD groups), the index names the property and the free parameters are drawn again until
the restated geometry has it.  A pair is built as test_fusion.make_pwdw builds it (couple(), below, is run by the tests on the
two make_case records): the second layer's input record is the first layer's output record, b_scale = in_scale * k_scale; on
top of that the two layers get independent `exact`, `act` and `per_channel`, and the intermediate zero point is set on both.

Every few lines of geometry restated here name the function they restate; tests/test_pair_sweeps.py pins choose_rect's
restatement to the code on the device (shl_mi355x_pwdw_geometry, all 12 fields).

What the caps leave out, by arithmetic:
  * the XCD group xg = 8 needs Co / 32 to be a multiple of 32 (whole 128-byte lines per XCD): 1024 output channels, which
    the list of Co / 32 does not hold; xg = 0 (the plain grid) is reached through SHL_MI355X_PWDW_XG only, which is read once per
    process.  The draws reach xg = 1, 2, 4.
  * stemdw_f16_nchw with ONE stem output channel: conv_plan.hip:is_depthwise asks group > 1, so the layer behind a 1-channel
    stem is a plain 1 -> 1 convolution to the planner (ALGO_DIRECT), shl_mi355x_pwdw_form is 0 and the fused kernel is never
    launched.  The smallest channel count the kernel can meet is 2, which stands in for 1 in the Co cycle: still a ragged group
    of eight, still channels beyond `dlive`.
  * an intermediate zero point of 127 under a relu on the first layer leaves one representable value: the intermediate is the
    constant 127.  Those cases (index-fixed, about one in eight) check the padding dword and the depthwise phase only.
  * stemdw_i8's class Wo >= 57 with both strides 2 needs an input 4 x 57 wide: the inputs go up to 270 x 60 x 3 (the largest
    at both strides 1 is 70 wide) -- still far below a millisecond of oracle.
"""
import functools

import numpy as np

from family_sweeps import BASE_SEED, _in_size_for, _pads, _pick, out_size

FAMILIES = {
    "pwdw_i8": dict(n=64, offset=1100, form=1, cap=3e8),
    "stemdw_i8": dict(n=32, offset=1200, form=3, cap=3e8),
    "stemdw_f16_nchw": dict(n=24, offset=1300, form=5, cap=3e8),
}
CHUNK = 8
SECOND_SEED = 500   # the second layer's operands: case_seed + SECOND_SEED
# switches a case may carry; both are read per call, the sub-process clears them between cases
CASE_SWITCHES = ("SHL_MI355X_PWDW_GENERIC", "SHL_MI355X_STEMDW_TILE")
MID_ZP = (-128, -3, 0, 7, 127)
STRIDES = ((1, 1), (2, 2), (1, 2), (2, 1))
EXACT_PAIRS = ((True, True), (True, False), (False, True), (False, False))
GEOMETRY_FIELDS = ("tiles_y", "tiles_x", "bh", "bw", "ey_lo", "ey_hi", "ex_lo", "ex_hi", "mt", "ks", "nwin", "blocks")


def case_seed(family, i):
    return 920000 + FAMILIES[family]["offset"] * 10 + i


def _rng(family, i, seed):
    return np.random.default_rng([(BASE_SEED if seed is None else seed) + FAMILIES[family]["offset"], i])


def _in_class(rng, bounds):
    return int(rng.integers(bounds[0], bounds[1], endpoint=True))


def _out_map(rng, hb, wb):
    """Ho, Wo in their classes, Ho != Wo unless both classes are the single value 1"""
    while True:
        ho, wo = _in_class(rng, hb), _in_class(rng, wb)
        if ho != wo or (hb[0] == hb[1] and wb[0] == wb[1]):
            return ho, wo


def couple(first, second, zp):
    """what test_fusion.make_pwdw does to its two make_case records, plus the intermediate zero point (int8; binary16 records
    carry no quantisation)"""
    if zp is None:
        return
    second["in_scale"] = first["out_scale"]
    first["out_zp"] = second["in_zp"] = zp
    second["b_scale"] = (np.float32(second["in_scale"]) * second["k_scale"]).astype(np.float32)


def epilogue(kw):
    """launch_pwdw_fused / launch_stemdw_fused: epq, epd = (act && !act_clamp) ? -1 : (div_exact ? 3 : 0).  conv_plan.hip:
    pow2_fold_ok is a property of the OUTPUT scale (make_case's `exact`), whatever the input record; derive_act_clamp succeeds for
    every scale make_case draws and every zero point (family_sweeps' docstring)"""
    return 3 if kw.get("exact", True) else 0


def flavour(pair):
    """the instantiation both launchers dispatch: <3, 3>, <0, 0> or the run-time flavour (-1, -1)"""
    e = (epilogue(pair["first"]), epilogue(pair["second"]))
    return e if e in ((3, 3), (0, 0)) else (-1, -1)


def dims(pair):
    """N, the first layer's input map, the intermediate map, the output map"""
    a, b = pair["first"], pair["second"]
    k, st, pad, dil = a.get("k", (3, 3)), a.get("stride", (1, 1)), a.get("pad", (1, 1, 1, 1)), a.get("dilation", (1, 1))
    hm, wm = out_size(a["h"], k[0], st[0], pad[0], pad[2], dil[0]), out_size(a["w"], k[1], st[1], pad[1], pad[3], dil[1])
    (sh, sw), p = b["stride"], b["pad"]
    return dict(n=a["n"], h=a["h"], w=a["w"], hm=hm, wm=wm, ho=out_size(hm, 3, sh, p[0], p[2]), wo=out_size(wm, 3, sw, p[1], p[3]))


def first_macs(pair):
    a, g = pair["first"], dims(pair)
    k = a.get("k", (3, 3))
    return g["n"] * g["hm"] * g["wm"] * a["c"] * a["co"] * k[0] * k[1]


def _coherent(pair):
    """the record every family shares: the second layer consumes the first one's output, image by image"""
    a, b, g = pair["first"], pair["second"], dims(pair)
    return bool(b.get("depthwise") and b["c"] == a["co"] and (b["h"], b["w"]) == (g["hm"], g["wm"]) and b["n"] == a["n"] and
                g["ho"] >= 1 and g["wo"] >= 1 and b.get("dilation", (1, 1)) == (1, 1))


# ------------------------------------------------------------------------------------------------ dw_patch.h
def dw_patch_pitch(npx):
    return ((npx + 31) & ~31) + 8


def dw_patch_bytes(npx):
    return dw_patch_pitch(npx) * 32


# the depthwise layers that belong to the OTHER pairing (depthwise -> pointwise) at throughput sizes: conv_plan.hip:pwdw_kernel_for
# asks these two first, and a latency form yields.  (Their epilogue condition holds for every make_case record and is left out:
# this restatement yields at least as often as the code.)
def dwpw_stream_takes(c, n, ho, wo, stride):
    """dwpw_stream.hip:dwpw_stream_takes without its switch"""
    if stride[0] != stride[1] or c not in (32, 64, 128, 256) or (c == 256 and stride[0] != 1):
        return False
    return n >= 8 or n * ho * wo * c >= 4 << 20


def dwpw_resident_takes(c, n, h, w, ho, wo, stride, pad):
    """dwpw_resident.hip:dwpw_resident_takes without its switch"""
    if stride != (1, 1) or pad[0] != 1 or pad[1] != 1 or c not in (256, 512) or (ho, wo) != (h, w):
        return False
    if c == 512 and (w & 1 or w > 16 or w < 4 or h & 1):
        return False
    if c == 256 and (w & 3 or w > 32 or w <= 16):
        return False
    return n * h >= (6 * 256 if c == 512 else 7 * 256)


def _yields(pair):
    b, g = pair["second"], dims(pair)
    return (dwpw_stream_takes(b["c"], g["n"], g["ho"], g["wo"], b["stride"]) or
            dwpw_resident_takes(b["c"], g["n"], g["hm"], g["wm"], g["ho"], g["wo"], b["stride"], b["pad"]))


# ------------------------------------------------------------------------------------------------ pwdw_i8
PW_C = (32, 64, 96, 128, 160, 192, 256, 384, 512, 768, 1024)
PW_SLICES = (1, 2, 3, 4, 8, 16)    # Co / 32
PW_CLASSES = ((1, 1), (2, 4), (5, 8), (9, 16), (17, 30))
PW_SPECIALISED = ((4, 4), (2, 4), (2, 2), (2, 1), (1, 1))   # (nsw, ks) of SHL_PWDW_FIXED
PW_FIXED = ((4, 4, 2), (4, 4, 1), (2, 4, 2), (2, 4, 1), (2, 2, 2), (2, 2, 1), (2, 1, 1), (2, 1, 2), (1, 1, 1), (1, 1, 2))   # in the launcher's order
PWDW_PAD_DWORDS = 3
PWDW_MTW = 4
# geometry the index asks of choose_rect's result (the free parameters are drawn until the restatement has it); None: whatever comes
PW_WANT = ("xg4", None, "stick_y", "xg2", None, "y_lo", "xg4", "x_lo", None, "mt3odd", "xg2", "y_hi", None, "x_hi", "xg4", "grid3d",
           None, "y_both", "xg2", "x_both", None, "stick_x", "xg4", "mt2", None, "pads2", "xg2", "mt3", None, "mt1", "xg4", None)


def ks_for(nsub):
    """pwdw_fused.hip:ks_for"""
    return 4 if nsub >= 8 else (2 if nsub >= 4 else 1)


def ks_nsw(c):
    """(K sub-steps per wave, K split) of a pointwise layer with c input channels: choose_rect's nsw and ks"""
    nsub = c >> 5
    return (nsub + ks_for(nsub) - 1) // ks_for(nsub), ks_for(nsub)


def axis_window(in_len, out_len, s, pad, b, n, e_lo, e_hi):
    """pwdw_fused.hip:axis_window"""
    best = 0
    for t in range(n):
        o0 = t * b + (e_lo if t > 0 else 0)
        ln = min(b + (e_lo if t == 0 else 0) + (e_hi if t == n - 1 else 0), out_len - o0)
        r0 = o0 * s - pad
        best = max(best, min(r0 + (ln - 1) * s + 3, in_len) - max(r0, 0))
    return best


def axis_grids(in_len, out_len, s, pad, lens, max_n):
    """pwdw_fused.hip:axis_grids (no grid forced) -> (b, n, e_lo, e_hi, win)"""
    v = [(b, (out_len + b - 1) // b, 0, 0) for b in lens]
    for n in range(2, min(max_n, out_len) + 1):
        for e in (1, 2, 3):
            e_lo, e_hi = e & 1, e >> 1
            rest = out_len - e_lo - e_hi
            if rest < n or rest % n:
                continue
            v.append((rest // n, n, e_lo, e_hi))
    return [a + (axis_window(in_len, out_len, s, pad, *a),) for a in v]


@functools.lru_cache(maxsize=None)
def choose_rect(C, Co, N, H, W, Ho, Wo, sh, sw, pt, pl):
    """pwdw_fused.hip:choose_rect without its two tuning switches -> the 12 fields of shl_mi355x_pwdw_geometry, xg, and what the
    launcher's form selection reads; None when nothing fits"""
    nsub = C >> 5
    ks = ks_for(nsub)
    mt_max = (4 // ks) * PWDW_MTW
    nsw = (nsub + ks - 1) // ks
    slices = Co >> 5
    lens_y = list(range(1, min(Ho, 32) + 1))
    lens_x = []
    for div in range(1, 17):
        bw = (Wo + div - 1) // div
        if div > 1 and bw == (Wo + div - 2) // (div - 1):
            continue
        lens_x.append(bw)
    gy, gx = axis_grids(H, Ho, sh, pt, lens_y, 32), axis_grids(W, Wo, sw, pl, lens_x, 16)
    best, pick = 1e30, None
    for y in gy:
        for x in gx:
            dbh, dbw = y[0] + max(y[2], y[3]), x[0] + max(x[2], x[3])
            rh, rw = (dbh - 1) * sh + 3, (dbw - 1) * sw + 3
            npx = rh * rw
            nwin = max(y[4], 1) * max(x[4], 1)
            mt = (nwin + 31) // 32
            if dbh > 32 or mt > mt_max or rw > 256 or dbw > 256 or npx >= 4096 or dbh * dbw >= 4096:
                continue
            if mt * ks * 4096 + dw_patch_bytes(npx) > 96 * 1024:
                continue
            blocks = slices * y[1] * x[1] * N
            rounds = float((blocks + 255) // 256)
            score = rounds * ((mt + 1) * nsub + 2.0 * ((dbh * dbw + 31) // 32) + 4.0) - (blocks / 1024.0 if blocks <= 256 else 0.0) + nwin * 1e-7
            if score < best:
                best, pick = score, (y, x)
    if pick is None:
        return None
    y, x = pick
    g = dict(tiles_y=y[1], tiles_x=x[1], bh=y[0], bw=x[0], ey_lo=y[2], ey_hi=y[3], ex_lo=x[2], ex_hi=x[3])
    g["dbh"], g["dbw"] = g["bh"] + max(g["ey_lo"], g["ey_hi"]), g["bw"] + max(g["ex_lo"], g["ex_hi"])
    g["iwm"] = max(x[4], 1)
    g["rw"] = (g["dbw"] - 1) * sw + 3
    g["npx"] = ((g["dbh"] - 1) * sh + 3) * g["rw"]
    g["nwin"] = max(y[4], 1) * max(x[4], 1)
    g["mt"] = (g["nwin"] + 31) // 32
    g.update(ks=ks, nsw=nsw, nsub=nsub)
    R = g["tiles_x"] * g["tiles_y"] * N
    act, wts = float(N) * H * W * C, float(C) * Co
    best_g, best_c = 0, 1e30
    for xg in (1, 2, 4, 8):
        if slices % xg or (xg > 1 and ((slices // xg) & 3)):
            continue
        rpg = 8 // xg
        if (slices // xg) * ((R + rpg - 1) // rpg) >= 4096 or R >= 4096:
            continue
        c = xg * act + rpg * wts
        if c < best_c:
            best_c, best_g = c, xg
    g.update(xg=best_g, nrect=R, blocks=slices * R)
    return g


def pwdw_rect(pair):
    a, b, g = pair["first"], pair["second"], dims(pair)
    return choose_rect(a["c"], a["co"], g["n"], g["hm"], g["wm"], g["ho"], g["wo"], b["stride"][0], b["stride"][1], b["pad"][0], b["pad"][1])


def pwdw_form(geo, generic):
    """launch_pwdw_fused's form selection -> ("fixed", nsw, ks, tiles per wave, exact tile count) or ("runtime", NSW bound, EXACT)"""
    if not generic:
        for nswv, ksv, tpw in PW_FIXED:
            t = tpw * (4 // ksv)
            if (geo["nsw"] == nswv and geo["nsub"] == ksv * nswv and geo["ks"] == ksv and (tpw - 1) * (4 // ksv) < geo["mt"] <= t and
                    dw_patch_bytes(geo["npx"]) <= 1024 * PWDW_PAD_DWORDS * t):
                return ("fixed", nswv, ksv, tpw, geo["mt"] == t)
    nswv = 2 if geo["nsw"] <= 2 else (4 if geo["nsw"] <= 4 else 8)
    return ("runtime", nswv, geo["nsw"] == nswv and geo["nsub"] == geo["ks"] * nswv)


def pwdw_admissible(pair):
    """pwdw_fused.hip:shapes_pair + pwdw_fusable (blocks <= 512), conv_plan.hip:pwdw_kernel_for (no yielding to the other pairing),
    igemm_supports + the fragment-ordered weight copy for the first layer, dwconv_dot4_supports for the second"""
    a, b = pair["first"], pair["second"]
    if not _coherent(pair) or a.get("k") != (1, 1) or a.get("pad") != (0, 0, 0, 0) or a.get("stride", (1, 1)) != (1, 1):
        return False
    g = dims(pair)
    (sh, sw), p = b["stride"], b["pad"]
    if a["c"] % 32 or a["co"] % 32 or a["c"] > 1024 or sh not in (1, 2) or sw not in (1, 2) or not (0 <= p[0] <= 2 and 0 <= p[1] <= 2):
        return False
    if g["hm"] * g["wm"] * a["c"] >= 1 << 31 or g["ho"] * g["wo"] * b["c"] >= 1 << 31 or _yields(pair):
        return False
    geo = pwdw_rect(pair)
    return bool(geo and geo["tiles_y"] * g["n"] <= 65535 and geo["tiles_x"] <= 65535 and geo["blocks"] <= 512)


def pwdw_has(geo, n, want):
    """the geometry properties PW_WANT names"""
    uniform_y, uniform_x = not (geo["ey_lo"] or geo["ey_hi"]), not (geo["ex_lo"] or geo["ex_hi"])
    return {
        "xg4": geo["xg"] == 4, "xg2": geo["xg"] == 2, "xg1": geo["xg"] == 1,
        "stick_y": uniform_y and geo["tiles_y"] * geo["bh"] > geo["_ho"], "stick_x": uniform_x and geo["tiles_x"] * geo["bw"] > geo["_wo"],
        "y_lo": (geo["ey_lo"], geo["ey_hi"]) == (1, 0), "y_hi": (geo["ey_lo"], geo["ey_hi"]) == (0, 1), "y_both": (geo["ey_lo"], geo["ey_hi"]) == (1, 1),
        "x_lo": (geo["ex_lo"], geo["ex_hi"]) == (1, 0), "x_hi": (geo["ex_lo"], geo["ex_hi"]) == (0, 1), "x_both": (geo["ex_lo"], geo["ex_hi"]) == (1, 1),
        "mt1": geo["mt"] == 1, "mt2": geo["mt"] == 2, "mt3": geo["mt"] >= 3, "mt3odd": geo["mt"] >= 3 and geo["mt"] % 2 == 1,
        "grid3d": geo["tiles_x"] > 1 and geo["tiles_y"] > 1 and n > 1,
        "fixed": pwdw_form(geo, False)[0] == "fixed", "tpw2": pwdw_form(geo, False)[0] == "fixed" and pwdw_form(geo, False)[3] == 2,
    }[want]


def pwdw_geometry(pair):
    """choose_rect's result with the output map beside it (pwdw_has reads both)"""
    geo = pwdw_rect(pair)
    if geo is None:
        return None
    g = dims(pair)
    return dict(geo, _ho=g["ho"], _wo=g["wo"])


PW_TPW2 = (12, 28, 33, 36, 63)   # one case per specialised (nsw, ks) pair that must run its two-tiles-per-wave instantiation


def _pw_classed(i):
    """the case keeps the map classes its index names: no geometry is asked of it (a class may not hold a given geometry at all)"""
    return PW_WANT[i % 32] is None and i not in PW_TPW2


PW_CLASSED = tuple(i for i in range(64) if _pw_classed(i))


def pwdw_strata(i):
    c, generic = PW_C[i % 11], i % 3 == 2
    want = (PW_WANT[i % 32],) if PW_WANT[i % 32] else ()
    if not generic and ks_nsw(c) in PW_SPECIALISED:   # without the switch a specialised pair runs a specialised form
        want += ("tpw2",) if i in PW_TPW2 else ("fixed",)
    r = PW_CLASSED.index(i) if i in PW_CLASSED else None   # the classes cycle over the cases that keep them
    return dict(c=c, generic=generic, stride=STRIDES[i % 4], exact=EXACT_PAIRS[(i // 4 + i // 16) % 4],
                act=((i // 3) % 3, (i // 9) % 3), per_channel=((i // 5) % 2 == 1, (i // 7) % 2 == 1), zp=MID_ZP[(i + i // 5) % 5],
                ho_class=None if r is None else PW_CLASSES[r % 5], wo_class=None if r is None else PW_CLASSES[(r + r // 5) % 5],
                # the classed cases stay below eight slices -- xg = 1 whatever the map, by the rule's "whole 128-byte lines"
                slices=PW_SLICES[:4] if r is not None else None, want=want)


def _draw_pwdw(i, rng):
    s = pwdw_strata(i)
    (sh, sw), want = s["stride"], s["want"]
    for _ in range(20000):
        hb = s["ho_class"] or _pick(rng, PW_CLASSES[:3] if "pads2" in want else PW_CLASSES)
        wb = s["wo_class"] or _pick(rng, PW_CLASSES[:3] if "pads2" in want else PW_CLASSES)
        ho, wo = _out_map(rng, hb, wb)
        pad = (2, 2, 2, 2) if "pads2" in want else _pads(rng)
        h, w = _in_size_for(rng, ho, sh, pad[0], pad[2]), _in_size_for(rng, wo, sw, pad[1], pad[3])
        if not (h and w):
            continue
        slices = 16 if "xg4" in want else (int(_pick(rng, (8, 16))) if "xg2" in want else int(_pick(rng, s["slices"] or PW_SLICES)))
        n = int(rng.integers(2, 4)) if "grid3d" in want else int(rng.integers(1, 4))
        first = dict(c=s["c"], co=32 * slices, h=h, w=w, n=n, k=(1, 1), pad=(0, 0, 0, 0), act=s["act"][0], exact=s["exact"][0],
                     per_channel=s["per_channel"][0])
        second = dict(depthwise=True, c=32 * slices, h=h, w=w, n=n, stride=(sh, sw), pad=pad, act=s["act"][1], exact=s["exact"][1],
                      per_channel=s["per_channel"][1])
        pair = dict(first=first, second=second, zp=s["zp"])
        if first_macs(pair) > FAMILIES["pwdw_i8"]["cap"] or not pwdw_admissible(pair):
            continue
        if "pads2" in want and max(ho, wo) > 5:
            continue
        if not all(pwdw_has(pwdw_geometry(pair), n, v) for v in want if v != "pads2"):
            continue
        return pair
    raise RuntimeError("pwdw_i8 case %d: no draw with %r" % (i, s))


# ------------------------------------------------------------------------------------------------ stemdw_i8
SD_HO = {"1": (1,), "2": (2,), "odd": (3, 5, 7, 9, 11), "even": (4, 6, 8, 10, 12)}   # the values of a class
SD_WO = {"lt28": tuple(range(1, 28)), "28": (28,), "29to55": tuple(range(29, 56)), "ge57": tuple(range(57, 65))}
SD_TILES = ("1x28", "3x9", "4x16", "2x64")
# the six cases with SHL_MI355X_STEMDW_TILE, each on a map it cuts differently from the rule's 2 x 28: "2x64" (four rounds of the
# depthwise loop) on two maps with Wo >= 57, "4x16" on two maps of at least four rows, "1x28" and "3x9" once
SD_TILE_CASES = {5: "2x64", 12: "3x9", 13: "1x28", 14: "4x16", 23: "2x64", 27: "4x16"}


def _ho_class(ho):
    return "1" if ho == 1 else ("2" if ho == 2 else ("odd" if ho % 2 else "even"))


def _wo_class(wo):
    return "lt28" if wo < 28 else ("28" if wo == 28 else ("29to55" if wo <= 55 else ("ge57" if wo >= 57 else "56")))


def stem_kernel(kw):
    """conv_plan.hip:choose_algo + conv_stem.hip:stem_supports, stem_mfma_pick (no switch) for an int8 NHWC layer: a 3-channel
    3 x 3 layer of at most 64 output channels is ALGO_STEM whatever its stride, padding and DILATION; the matrix-core form refuses
    a dilated layer and any layer below 2^24 outputs, so the dot4 kernel (which walks y0 + ky dh, x0 + kx dw) runs it"""
    if kw.get("dtype", "int8") != "int8" or kw.get("depthwise") or kw["c"] != 3 or kw.get("k", (3, 3)) != (3, 3) or kw["co"] > 64:
        return None
    st, pad, dil = kw.get("stride", (1, 1)), kw.get("pad", (1, 1, 1, 1)), kw.get("dilation", (1, 1))
    M = kw["n"] * out_size(kw["h"], 3, st[0], pad[0], pad[2], dil[0]) * out_size(kw["w"], 3, st[1], pad[1], pad[3], dil[1])
    mfma = kw["co"] % 16 == 0 and dil == (1, 1) and M < 1 << 22 and 12 <= kw["n"] * kw["h"] * kw["w"] * 3 < (1 << 31) - 16 and M * kw["co"] >= 1 << 24
    return "conv_stem_i8_mfma32x32x32" if mfma else "conv_stem_i8_dot4"


def stemdw_geometry(ho, wo, sh, sw, n, tile=None):
    """stemdw_fused.hip:stemdw_geometry, SHL_MI355X_STEMDW_TILE included -> the grid, the patch and the two loops' trip counts;
    None where it refuses"""
    bh, bw = min(ho, 2), min(wo, 28)
    if tile:
        th, tw = (int(v) for v in tile.split("x"))
        if th > 0 and tw > 0:
            bh, bw = min(th, ho), min(tw, wo)
    tiles_y, tiles_x = (ho + bh - 1) // bh, (wo + bw - 1) // bw
    rw = (bw - 1) * sw + 3
    npx = ((bh - 1) * sh + 3) * rw
    if npx >= 2048 or tiles_x > 65535 or tiles_y * n > 65535 or tiles_x * tiles_y * n > 2048:
        return None
    return dict(bh=bh, bw=bw, tiles_y=tiles_y, tiles_x=tiles_x, rw=rw, npx=npx, lds=(7 * 32 + 96) * 4 + dw_patch_bytes(npx),
                phase1_trips=(2 * npx + 255) // 256, dw_trips=(bh * bw + 31) // 32)


def stemdw_rect(pair, env):
    b, g = pair["second"], dims(pair)
    return stemdw_geometry(g["ho"], g["wo"], b["stride"][0], b["stride"][1], g["n"], env.get("SHL_MI355X_STEMDW_TILE"))


def stemdw_admissible(pair, env):
    """conv_plan.hip:pwdw_kernel_for (ALGO_STEM first layer, dot4-packed depthwise, no yielding) + stemdw_fused.hip:stemdw_geometry"""
    a, b = pair["first"], pair["second"]
    if not _coherent(pair) or stem_kernel(a) is None or a["co"] != 32:
        return False
    (sh, sw), p = b["stride"], b["pad"]
    if sh not in (1, 2) or sw not in (1, 2) or not (0 <= p[0] <= 2 and 0 <= p[1] <= 2) or _yields(pair):
        return False
    return stemdw_rect(pair, env) is not None


def stemdw_strata(i):
    a, b, c = i % 4, (i // 4) % 4, i // 16
    return dict(stem_stride=STRIDES[(a + 1) % 4], dw_stride=STRIDES[(a + b) % 4], dilation=(2, 2) if (i + i // 8) % 4 == 3 else (1, 1),
                ho_class=list(SD_HO)[(b + c) % 4], wo_class=list(SD_WO)[(a + b + 2 * c + 1) % 4], n=1 + (i + i // 4) % 3,
                exact=EXACT_PAIRS[(i // 2) % 4], act=(i % 3, (i // 3) % 3), per_channel=((i // 5) % 2 == 1, (i // 7) % 2 == 1),
                zp=MID_ZP[i % 5], tile=SD_TILE_CASES.get(i))


def _draw_stemdw(i, rng):
    s = stemdw_strata(i)
    (qh, qw), (sh, sw), (dh, dw) = s["stem_stride"], s["dw_stride"], s["dilation"]
    for _ in range(4000):
        ho, wo = int(_pick(rng, SD_HO[s["ho_class"]])), int(_pick(rng, SD_WO[s["wo_class"]]))
        pad2, pad1 = _pads(rng), _pads(rng)
        hm, wm = _in_size_for(rng, ho, sh, pad2[0], pad2[2]), _in_size_for(rng, wo, sw, pad2[1], pad2[3])
        if not (hm and wm):
            continue
        h, w = _in_size_for(rng, hm, qh, pad1[0], pad1[2], dh), _in_size_for(rng, wm, qw, pad1[1], pad1[3], dw)
        if not (h and w):
            continue
        first = dict(c=3, co=32, n=s["n"], h=h, w=w, stride=(qh, qw), pad=pad1, dilation=(dh, dw), act=s["act"][0], exact=s["exact"][0],
                     per_channel=s["per_channel"][0])
        second = dict(depthwise=True, c=32, n=s["n"], h=hm, w=wm, stride=(sh, sw), pad=pad2, act=s["act"][1], exact=s["exact"][1],
                      per_channel=s["per_channel"][1])
        pair = dict(first=first, second=second, zp=s["zp"])
        if stemdw_admissible(pair, case_env("stemdw_i8", i)):
            return pair
    raise RuntimeError("stemdw_i8 case %d: no draw with %r" % (i, s))


# ------------------------------------------------------------------------------------------------ stemdw_f16_nchw
SF_CO = (2, 7, 8, 16, 24, 32)   # (2, not 1: the module docstring)
SF_HO = {"lt4": (1, 2, 3), "4": (4,), "5to7": (5, 6, 7), "ge9": (9, 10, 11, 12)}
SF_WO = {"lt16": tuple(range(1, 16)), "16": (16,), "17to31": tuple(range(17, 32)), "ge33": tuple(range(33, 41))}
SF_STEM_STRIDES = ((1, 1), (2, 2), (2, 1), (1, 2))


def stemdw_f16_geometry(pair):
    """stemdw_f16_nchw.hip:geometry + the launcher's grid and LDS size"""
    a, b, g = pair["first"], pair["second"], dims(pair)
    (qh, qw), (sh, sw) = a["stride"], b["stride"]
    bh, bw = min(g["ho"], 4), min(g["wo"], 16)
    rh, rw = (bh - 1) * sh + 3, (bw - 1) * sw + 3
    npx = rh * rw
    ppitch, groups = (npx + 7) & ~7, (a["co"] + 7) // 8
    ih, iw = (rh - 1) * qh + 3, (rw - 1) * qw + 3
    lds = 27 * groups * 8 * 4 + ((a["co"] * ppitch * 2 + 15) & ~15) + 3 * ih * iw * 4
    return dict(bh=bh, bw=bw, rh=rh, rw=rw, npx=npx, ppitch=ppitch, groups=groups, tiles_x=(g["wo"] + bw - 1) // bw,
                tiles_y=(g["ho"] + bh - 1) // bh, lds=lds, items=npx * groups)


def stemdw_f16_admissible(pair):
    """stemdw_f16_nchw.hip:shapes + stemdw_f16_nchw_fusable, conv_plan.hip:pwdw_kernel_for (a binary16 3-channel layer is
    ALGO_DIRECT: 6 bytes of K are no implicit GEMM's) -- AND the launcher's own 64 KiB of LDS, which the pair test does not ask:
    no draw may live on that difference"""
    a, b = pair["first"], pair["second"]
    if not _coherent(pair) or a.get("dtype") != "f16" or b.get("dtype") != "f16" or a.get("layout") != "NCHW" or b.get("layout") != "NCHW":
        return False
    if a["c"] != 3 or a.get("k", (3, 3)) != (3, 3) or not 1 <= a["co"] <= 32 or a.get("dilation", (1, 1)) != (1, 1) or b["c"] < 2:
        return False
    (qh, qw), (sh, sw), p, g = a["stride"], b["stride"], b["pad"], dims(pair)
    if not all(v in (1, 2) for v in (qh, qw, sh, sw)) or not (0 <= p[0] <= 2 and 0 <= p[1] <= 2):
        return False
    if g["n"] * 3 * g["h"] * g["w"] >= 1 << 31 or g["n"] * b["c"] * g["ho"] * g["wo"] >= 1 << 31:
        return False
    geo = stemdw_f16_geometry(pair)
    return geo["tiles_x"] * geo["tiles_y"] * g["n"] <= 2048 and g["n"] <= 65535 and geo["lds"] <= 64 * 1024


def stemdw_f16_strata(i):
    a, b, c = i % 4, (i // 4) % 4, i // 16
    return dict(co=SF_CO[i % 6], stem_stride=SF_STEM_STRIDES[a], dw_stride=STRIDES[(a + b) % 4], ho_class=list(SF_HO)[(b + c) % 4],
                wo_class=list(SF_WO)[(a + b + 2 * c + 1) % 4], n=1 + (i + i // 3) % 3, act=(i % 3, (i // 3) % 3))


def _draw_stemdw_f16(i, rng):
    s = stemdw_f16_strata(i)
    (qh, qw), (sh, sw) = s["stem_stride"], s["dw_stride"]
    for _ in range(4000):
        ho, wo = int(_pick(rng, SF_HO[s["ho_class"]])), int(_pick(rng, SF_WO[s["wo_class"]]))
        pad2, pad1 = _pads(rng), _pads(rng)
        hm, wm = _in_size_for(rng, ho, sh, pad2[0], pad2[2]), _in_size_for(rng, wo, sw, pad2[1], pad2[3])
        if not (hm and wm):
            continue
        h, w = _in_size_for(rng, hm, qh, pad1[0], pad1[2]), _in_size_for(rng, wm, qw, pad1[1], pad1[3])
        if not (h and w):
            continue
        first = dict(layout="NCHW", dtype="f16", c=3, co=s["co"], n=s["n"], h=h, w=w, stride=(qh, qw), pad=pad1, act=s["act"][0])
        second = dict(layout="NCHW", dtype="f16", depthwise=True, c=s["co"], n=s["n"], h=hm, w=wm, stride=(sh, sw), pad=pad2, act=s["act"][1])
        pair = dict(first=first, second=second, zp=None)
        if stemdw_f16_admissible(pair):
            return pair
    raise RuntimeError("stemdw_f16_nchw case %d: no draw with %r" % (i, s))


# ------------------------------------------------------------------------------------------------ the families' common face
_DRAW = {"pwdw_i8": _draw_pwdw, "stemdw_i8": _draw_stemdw, "stemdw_f16_nchw": _draw_stemdw_f16}
_STRATA = {"pwdw_i8": pwdw_strata, "stemdw_i8": stemdw_strata, "stemdw_f16_nchw": stemdw_f16_strata}


@functools.lru_cache(maxsize=None)
def _draw_cached(family, i, seed):
    return _DRAW[family](i, _rng(family, i, seed))


def draw(family, i, seed=None):
    if not 0 <= i < FAMILIES[family]["n"]:
        raise IndexError("%s has %d cases" % (family, FAMILIES[family]["n"]))
    p = _draw_cached(family, i, BASE_SEED if seed is None else seed)
    return dict(first=dict(p["first"]), second=dict(p["second"]), zp=p["zp"])


def strata(family, i):
    return _STRATA[family](i)


def case_env(family, i):
    if family == "pwdw_i8" and pwdw_strata(i)["generic"]:
        return {"SHL_MI355X_PWDW_GENERIC": "1"}
    if family == "stemdw_i8" and stemdw_strata(i)["tile"]:
        return {"SHL_MI355X_STEMDW_TILE": stemdw_strata(i)["tile"]}
    return {}


def admissible(family, pair, env=None):
    """the pair runs the family's fused kernel (shl_mi355x_pwdw_form = FAMILIES[family]["form"]) with the case's switches"""
    if family == "pwdw_i8":
        return pwdw_admissible(pair)
    if family == "stemdw_i8":
        return stemdw_admissible(pair, env or {})
    if family == "stemdw_f16_nchw":
        return stemdw_f16_admissible(pair)
    raise KeyError(family)


def chunks():
    """(family, first case) of every GPU test"""
    return [(f, lo) for f in FAMILIES for lo in range(0, FAMILIES[f]["n"], CHUNK)]

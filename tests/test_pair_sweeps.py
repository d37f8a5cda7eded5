"""Seeded, stratified sweeps (tests/pair_sweeps.py) over the fused pair kernels -- pwdw_fused.hip, stemdw_fused.hip (both on
dw_patch.h) and stemdw_f16_nchw.hip -- on non-square maps, anisotropic strides, mixed epilogue flavours, every intermediate zero
point that matters and every K split, with the library's own geometry pinned to a restatement.

CPU: the draws are reproducible, fill every stratum, stay under the MAC cap and inside the fused kernel's admission rule; the
restated choose_rect gives the grid that test_pwdw_window.py reads from the device for MobileNetV1's 14 x 14 pairs.
GPU: per chunk of eight cases one sub-process.  Per case: both layers stand-alone through csinn_* on device tensors (the second
fed the first's output), shl_mi355x_pwdw_form = the family's, shl_mi355x_pwdw_geometry = the restatement in all 12 fields
(pwdw_i8), zero mismatches (binary16: zero differing words) of the stand-alone AND of the fused output against the oracle chain
oracle(second, input = oracle(first)), then the fused launch into the middle of an allocation filled with 0x5A, 4 KiB of guard
on either side -- the stand-alone bytes, both bands untouched -- and once more into an allocation filled with 0xA5: the same
bytes again (an output byte the kernel never writes cannot match under both fills)."""
import collections
import os
import subprocess
import sys
import time

import pytest

import pair_sweeps as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(f, i) for f in ps.FAMILIES for i in range(ps.FAMILIES[f]["n"])]
SEEDS = (None, ps.BASE_SEED + 1, ps.BASE_SEED + 2)   # the strata hold for every seed: three are asked


def draws(family, seed=None):
    return [ps.draw(family, i, seed) for i in range(ps.FAMILIES[family]["n"])]


def fixed_by_index(family, i, pair):
    """what strata() names of the draw: a changed seed must leave it alone"""
    a, b = pair["first"], pair["second"]
    if family == "stemdw_f16_nchw":
        return dict(co=a["co"], stem_stride=a["stride"], dw_stride=b["stride"], n=a["n"], act=(a["act"], b["act"]))
    out = dict(exact=(a["exact"], b["exact"]), act=(a["act"], b["act"]), per_channel=(a["per_channel"], b["per_channel"]), zp=pair["zp"])
    if family == "pwdw_i8":
        out.update(c=a["c"], stride=b["stride"])
    else:
        out.update(stem_stride=a["stride"], dw_stride=b["stride"], dilation=a["dilation"], n=a["n"])
    return out


# ------------------------------------------------------------------------------------------------ CPU: the draws
def test_draws_are_reproducible_and_the_seed_moves_only_the_free_parameters():
    assert [ps.FAMILIES[f]["n"] for f in ps.FAMILIES] == [64, 32, 24] and len(ps.chunks()) == 15
    moved = 0
    for f, i in ALL:
        a, s = ps.draw(f, i), ps.strata(f, i)
        assert a == ps.draw(f, i), (f, i)
        b = ps.draw(f, i, seed=ps.BASE_SEED + 1)
        moved += a != b
        for pair in (a, b):
            fixed = fixed_by_index(f, i, pair)
            assert fixed == {k: s[k] for k in fixed}, (f, i, pair, s)
            assert ps.admissible(f, pair, ps.case_env(f, i)) and ps.first_macs(pair) <= ps.FAMILIES[f]["cap"], (f, i, pair)
    assert moved > len(ALL) // 2


@pytest.mark.parametrize("family", list(ps.FAMILIES))
def test_every_case_is_coupled_under_the_mac_cap_and_inside_the_fused_kernels_domain(family):
    total = 0
    for i, pair in enumerate(draws(family)):
        a, b, g = pair["first"], pair["second"], ps.dims(pair)
        assert (b["h"], b["w"], b["c"], b["n"]) == (g["hm"], g["wm"], a["co"], a["n"]) and g["ho"] >= 1 and g["wo"] >= 1, (i, pair)
        assert ps.admissible(family, pair, ps.case_env(family, i)), (i, pair)   # the share that may fall back is zero
        assert ps.first_macs(pair) <= ps.FAMILIES[family]["cap"], (i, pair)
        assert all(p in (0, 1, 2) for p in a["pad"] + b["pad"]) and 1 <= a["n"] <= 3
        assert set(ps.case_env(family, i)) <= set(ps.CASE_SWITCHES)
        total += ps.first_macs(pair) + g["n"] * g["ho"] * g["wo"] * b["c"] * 9
    assert total <= 6e9, total   # a few seconds of the CPU oracle per family, over its chunks


def test_an_inadmissible_pair_is_recognised():
    pair = ps.draw("pwdw_i8", 1)
    assert ps.admissible("pwdw_i8", pair)
    for change in (dict(first=dict(pair["first"], co=48), second=dict(pair["second"], c=48)),           # no whole 32-channel slice
                   dict(second=dict(pair["second"], h=pair["second"]["h"] + 1)),                          # not the first layer's output
                   dict(second=dict(pair["second"], stride=(3, 1))),
                   dict(first=dict(pair["first"], n=64, h=30, w=29), second=dict(pair["second"], n=64, h=30, w=29))):   # throughput sizes
        assert not ps.admissible("pwdw_i8", dict(pair, **change)), change
    assert ps.stemdw_geometry(12, 64, 2, 2, 1, "4x64") and ps.stemdw_geometry(12, 64, 2, 2, 1, "12x64") is None   # npx >= 2048
    f16 = ps.draw("stemdw_f16_nchw", 3)
    assert not ps.admissible("stemdw_f16_nchw", dict(first=dict(f16["first"], co=1), second=dict(f16["second"], c=1), zp=None))   # no depthwise layer
    assert not ps.admissible("stemdw_f16_nchw", dict(f16, first=dict(f16["first"], dilation=(2, 2))))


def test_the_restated_choose_rect_gives_the_grids_the_device_is_known_to_choose():
    # test_pwdw_window.py reads these from shl_mi355x_pwdw_geometry: 14 x 14, stride 1, 256 / 512 -> 512 channels
    for c in (256, 512):
        g = ps.choose_rect(c, 512, 1, 14, 14, 14, 14, 1, 1, 1, 1)
        assert [g[k] for k in ps.GEOMETRY_FIELDS] == [4, 4, 3, 3, 1, 1, 1, 1, 1, 4, 25, 256], g
    assert ps.ks_nsw(512) == (4, 4) and ps.ks_nsw(256) == (2, 4) and ps.ks_nsw(128) == (2, 2) and ps.ks_nsw(64) == (2, 1) and ps.ks_nsw(32) == (1, 1)
    assert ps.axis_window(14, 14, 1, 1, 3, 4, 1, 1) == 5 and ps.axis_window(14, 14, 1, 1, 4, 4, 0, 0) == 6
    assert ps.dw_patch_bytes(25) == 40 * 32 and ps.dw_patch_bytes(33) == 72 * 32


@pytest.mark.parametrize("seed", SEEDS)
def test_pwdw_i8_strata(seed):
    F = "pwdw_i8"
    N = ps.FAMILIES[F]["n"]
    pairs = draws(F, seed)
    geo = [ps.pwdw_geometry(p) for p in pairs]
    generic = [bool(ps.case_env(F, i)) for i in range(N)]
    form = [ps.pwdw_form(g, sw) for g, sw in zip(geo, generic)]
    assert generic == [i % 3 == 2 for i in range(N)]
    assert collections.Counter(p["first"]["c"] for p in pairs) == collections.Counter(ps.PW_C[i % 11] for i in range(N))
    # the K splits: every specialised (nsw, ks) pair at least four times in its own instantiation, each with one and with two tiles
    # per wave; the three run-time forms with EXACT true and false; every specialised pair in the run-time form too (the switch)
    fixed = collections.Counter(f[1:3] for f in form if f[0] == "fixed")
    assert set(fixed) == set(ps.PW_SPECIALISED) and min(fixed.values()) >= 4, fixed
    assert {f[1:4] for f in form if f[0] == "fixed"} >= {(a, b, t) for a, b in ps.PW_SPECIALISED for t in (1, 2)}, form
    assert {f[4] for f in form if f[0] == "fixed"} == {True, False}   # the tile count fills the instantiation, or leaves padded tiles
    runtime = collections.Counter(f[1:] for f in form if f[0] == "runtime")
    assert set(runtime) == {(b, e) for b in (2, 4, 8) for e in (True, False)} and min(runtime.values()) >= 2, runtime
    assert {(g["nsw"], g["ks"]) for g, sw in zip(geo, generic) if sw} >= set(ps.PW_SPECIALISED)
    assert {p["first"]["c"] for p, f in zip(pairs, form) if f[0] == "runtime"} >= {96, 160, 192, 384, 768, 1024}
    # the epilogue pair
    fl = collections.Counter(ps.flavour(p) for p in pairs)
    assert set(fl) == {(3, 3), (0, 0), (-1, -1)} and min(fl.values()) >= 12, fl
    assert len({(p["first"]["exact"], p["second"]["exact"]) for p in pairs}) == 4
    mixed = {f[1:3] for p, f in zip(pairs, form) if f[0] == "fixed" and ps.flavour(p) == (-1, -1)}
    assert mixed == set(ps.PW_SPECIALISED), mixed   # SHL_PWDW_EPI's default-argument instantiation, for every K split
    assert {f[1:] for p, f in zip(pairs, form) if f[0] == "runtime" and ps.flavour(p) == (-1, -1)} >= {(2, True), (4, False), (8, True), (8, False)}
    # strides, activations, tables, the intermediate zero point
    st = collections.Counter(p["second"]["stride"] for p in pairs)
    assert set(st) == set(ps.STRIDES) and min(st.values()) == 16
    assert len({(p["second"]["stride"], p["first"]["exact"], p["second"]["exact"]) for p in pairs}) == 16
    acts = collections.Counter((p["first"]["act"], p["second"]["act"]) for p in pairs)
    assert len(acts) == 9 and min(acts.values()) >= 2, acts
    assert len({(p["first"]["per_channel"], p["second"]["per_channel"]) for p in pairs}) == 4
    zps = collections.Counter(p["zp"] for p in pairs)
    assert set(zps) == set(ps.MID_ZP) and min(zps.values()) >= 12, zps
    assert {(p["zp"], f[0]) for p, f in zip(pairs, form)} == {(z, k) for z in ps.MID_ZP for k in ("fixed", "runtime")}
    # the slices and the batch
    assert {p["first"]["co"] // 32 for p in pairs} == set(ps.PW_SLICES) and {p["first"]["n"] for p in pairs} == {1, 2, 3}
    # the output map: every class of Ho and of Wo, never square (but 1 x 1), pads 0 .. 2 on every side
    cls = lambda v: [k for k, (lo, hi) in enumerate(ps.PW_CLASSES) if lo <= v <= hi][0]
    for axis in ("_ho", "_wo"):
        c = collections.Counter(cls(g[axis]) for g in geo)
        assert len(c) == 5 and min(c.values()) >= 2, (axis, c)
        by_index = collections.Counter(cls(g[axis]) for i, g in enumerate(geo) if i in ps.PW_CLASSED)
        assert len(by_index) == 5 and min(by_index.values()) >= 2, (axis, by_index)
    for i in ps.PW_CLASSED:
        s = ps.pwdw_strata(i)
        assert (ps.PW_CLASSES[cls(geo[i]["_ho"])], ps.PW_CLASSES[cls(geo[i]["_wo"])]) == (s["ho_class"], s["wo_class"]) and geo[i]["xg"] == 1
    assert all(g["_ho"] != g["_wo"] or g["_ho"] == 1 for g in geo)
    assert len({p["second"]["pad"] for p in pairs}) >= 30
    assert sum(p["second"]["pad"] == (2, 2, 2, 2) and max(g["_ho"], g["_wo"]) <= 5 for p, g in zip(pairs, geo)) >= 2   # most windows are padding
    # choose_rect's grids
    has = lambda want: sum(ps.pwdw_has(g, p["first"]["n"], want) for p, g in zip(pairs, geo))
    for want in ("stick_y", "stick_x", "y_lo", "y_hi", "y_both", "x_lo", "x_hi", "x_both", "mt1", "mt2", "mt3", "mt3odd", "grid3d"):
        assert has(want) >= 2, want
    for want in ("xg1", "xg2", "xg4"):
        assert has(want) >= 6, want
    assert all(g["xg"] in (1, 2, 4) and g["blocks"] <= 512 for g in geo)
    for i in range(N):   # ... where the index asks for them
        assert all(v == "pads2" or ps.pwdw_has(geo[i], pairs[i]["first"]["n"], v) for v in ps.pwdw_strata(i)["want"]), i
    # the magic divisions (j * magic) >> 20 the kernel uses are exact for every index it forms
    for g in geo:
        for div, top in ((g["iwm"], 32 * 16), (g["dbw"], g["dbh"] * g["dbw"] + 64), (g["tiles_x"], g["nrect"] + 8), (g["blocks"] // g["nrect"] // g["xg"], 4096)):
            magic = ((1 << 20) + div - 1) // div
            assert all((j * magic) >> 20 == j // div for j in range(min(top, 4096))), (g, div)


@pytest.mark.parametrize("seed", SEEDS)
def test_stemdw_i8_strata(seed):
    F = "stemdw_i8"
    N = ps.FAMILIES[F]["n"]
    pairs = draws(F, seed)
    envs = [ps.case_env(F, i) for i in range(N)]
    geo = [ps.stemdw_rect(p, e) for p, e in zip(pairs, envs)]
    dm = [ps.dims(p) for p in pairs]
    assert all(p["first"]["c"] == 3 and p["first"]["co"] == 32 and ps.stem_kernel(p["first"]) == "conv_stem_i8_dot4" for p in pairs)
    combos = collections.Counter((p["first"]["stride"], p["second"]["stride"]) for p in pairs)
    assert len(combos) == 16 and min(combos.values()) == 2, combos
    dil = [p["first"]["dilation"] for p in pairs]
    assert dil.count((2, 2)) == N // 4 and {p["first"]["stride"] for p in pairs if p["first"]["dilation"] == (2, 2)} == set(ps.STRIDES)
    assert len({p["first"]["pad"] for p in pairs}) >= 12 and len({p["second"]["pad"] for p in pairs}) >= 12
    assert {v for p in pairs for v in p["first"]["pad"]} == {0, 1, 2}
    classes = collections.Counter((ps._ho_class(d["ho"]), ps._wo_class(d["wo"])) for d in dm)
    assert set(classes) == {(h, w) for h in ps.SD_HO for w in ps.SD_WO} and min(classes.values()) == 2, classes   # crossed
    assert [(ps._ho_class(d["ho"]), ps._wo_class(d["wo"])) for d in dm] == [(ps.stemdw_strata(i)["ho_class"], ps.stemdw_strata(i)["wo_class"]) for i in range(N)]
    assert {d["n"] for d in dm} == {1, 2, 3}
    assert sum(d["n"] > 1 and g["tiles_y"] > 1 for d, g in zip(dm, geo)) >= 6    # n = ty / tiles_y
    # what a last rectangle needs: it sticks out in x, in y (an odd Ho), both; a single row; a map narrower than a rectangle
    assert sum(g["tiles_x"] * g["bw"] > d["wo"] for d, g in zip(dm, geo)) >= 6 and sum(g["tiles_y"] * g["bh"] > d["ho"] for d, g in zip(dm, geo)) >= 4
    assert sum(g["tiles_x"] * g["bw"] > d["wo"] and g["tiles_y"] * g["bh"] > d["ho"] for d, g in zip(dm, geo)) >= 2
    assert sum(g["tiles_x"] >= 3 for g in geo) >= 4 and sum(g["bh"] == 1 for g in geo) >= 4 and sum(g["bw"] < 28 for g in geo) >= 4
    # epilogue flavours, activations, tables, the intermediate zero point
    fl = collections.Counter(ps.flavour(p) for p in pairs)
    assert set(fl) == {(3, 3), (0, 0), (-1, -1)} and min(fl.values()) >= 8 and len({(p["first"]["exact"], p["second"]["exact"]) for p in pairs}) == 4, fl
    acts = collections.Counter((p["first"]["act"], p["second"]["act"]) for p in pairs)
    assert len(acts) == 9 and min(acts.values()) >= 2, acts
    assert len({(p["first"]["per_channel"], p["second"]["per_channel"]) for p in pairs}) == 4
    zps = collections.Counter(p["zp"] for p in pairs)
    assert set(zps) == set(ps.MID_ZP) and min(zps.values()) >= 6, zps
    assert {(p["zp"], ps.flavour(p) == (-1, -1)) for p in pairs} == {(z, m) for z in ps.MID_ZP for m in (True, False)}
    # the tile switch: six cases, every value, each cutting its map differently from the rule
    tiled = [i for i in range(N) if envs[i]]
    assert len(tiled) == 6 and {envs[i]["SHL_MI355X_STEMDW_TILE"] for i in tiled} == set(ps.SD_TILES)
    for i in tiled:
        rule = ps.stemdw_rect(pairs[i], {})
        th, tw = (int(v) for v in envs[i]["SHL_MI355X_STEMDW_TILE"].split("x"))
        assert (geo[i]["bh"], geo[i]["bw"]) != (rule["bh"], rule["bw"]) and geo[i]["bh"] == min(th, dm[i]["ho"]) and geo[i]["bw"] == min(tw, dm[i]["wo"]), i
    assert all(g["npx"] < 2048 and g["lds"] <= 64 * 1024 and g["tiles_x"] * g["tiles_y"] * d["n"] <= 2048 for d, g in zip(dm, geo))
    p1 = collections.Counter(min(g["phase1_trips"], 3) for g in geo)   # ntasks = 2 npx over 256 threads
    assert set(p1) == {1, 2, 3} and min(p1.values()) >= 2, p1
    p2 = collections.Counter(min(g["dw_trips"], 3) for g in geo)       # bh * bw outputs, 32 per round
    assert set(p2) == {1, 2, 3} and min(p2.values()) >= 2, p2
    for g in geo:   # the kernel's two magic divisions
        for div, top in ((g["rw"], g["npx"]), (g["bw"], g["bh"] * g["bw"] + 32)):
            magic = ((1 << 20) + div - 1) // div
            assert all((j * magic) >> 20 == j // div for j in range(top)), (g, div)
    assert max(d["h"] for d in dm) <= 60 and max(d["w"] for d in dm) <= 280   # the inputs stay small (pair_sweeps' docstring)


def test_a_dilated_three_channel_layer_is_the_dot4_stem():
    kw = ps.draw("stemdw_i8", 3)["first"]
    assert kw["dilation"] == (2, 2) and ps.stem_kernel(kw) == "conv_stem_i8_dot4"
    assert ps.stem_kernel(dict(kw, c=4)) is None and ps.stem_kernel(dict(kw, co=96)) is None
    # the matrix-core form takes a large undilated layer, never a dilated one
    big = dict(c=3, co=32, n=2, h=1024, w=1024, stride=(2, 2))
    assert ps.stem_kernel(big) == "conv_stem_i8_mfma32x32x32" and ps.stem_kernel(dict(big, dilation=(2, 2))) == "conv_stem_i8_dot4"


@pytest.mark.parametrize("seed", SEEDS)
def test_stemdw_f16_nchw_strata(seed):
    F = "stemdw_f16_nchw"
    N = ps.FAMILIES[F]["n"]
    pairs = draws(F, seed)
    geo = [ps.stemdw_f16_geometry(p) for p in pairs]
    dm = [ps.dims(p) for p in pairs]
    assert all(p["zp"] is None and p["first"]["layout"] == "NCHW" and p["first"]["dtype"] == "f16" and p["second"]["dtype"] == "f16" for p in pairs)
    co = collections.Counter(p["first"]["co"] for p in pairs)
    assert set(co) == set(ps.SF_CO) == {2, 7, 8, 16, 24, 32} and min(co.values()) == 4   # (2 for 1: pair_sweeps' docstring)
    assert {c % 8 == 0 for c in co} == {True, False} and {32 - c > 0 for c in co} == {True, False}   # ragged groups, channels beyond dlive
    combos = {(p["first"]["stride"], p["second"]["stride"]) for p in pairs}
    assert len(combos) == 16
    assert {v for p in pairs for v in p["first"]["pad"] + p["second"]["pad"]} == {0, 1, 2} and len({p["second"]["pad"] for p in pairs}) >= 10
    hc = lambda v: [k for k, vals in ps.SF_HO.items() if v in vals][0]
    wc = lambda v: [k for k, vals in ps.SF_WO.items() if v in vals][0]
    classes = collections.Counter((hc(d["ho"]), wc(d["wo"])) for d in dm)
    assert set(classes) == {(h, w) for h in ps.SF_HO for w in ps.SF_WO}, classes
    assert {d["n"] for d in dm} == {1, 2, 3}
    acts = collections.Counter((p["first"]["act"], p["second"]["act"]) for p in pairs)
    assert len(acts) == 9 and min(acts.values()) >= 2, acts
    # 4 x 16 rectangles: one, several, a last one that sticks out (in x, in y), a map smaller than a rectangle
    assert sum(g["tiles_x"] * g["bw"] > d["wo"] for d, g in zip(dm, geo)) >= 4 and sum(g["tiles_y"] * g["bh"] > d["ho"] for d, g in zip(dm, geo)) >= 4
    assert sum(g["bh"] < 4 for g in geo) >= 2 and sum(g["bw"] < 16 for g in geo) >= 2 and sum(g["tiles_x"] >= 3 for g in geo) >= 2
    assert sum(g["items"] > 512 for g in geo) >= 2 and sum(g["items"] <= 512 for g in geo) >= 2   # the item loop: one round, several
    # the launcher refuses above 64 KiB of LDS although stemdw_f16_nchw_fusable does not ask: no draw depends on that
    assert max(g["lds"] for g in geo) <= 64 * 1024
    for g in geo:
        for div, top in ((g["npx"], g["items"] + 512), (g["rw"], g["npx"]), (g["bw"], g["bh"] * g["bw"] + 16)):
            magic = ((1 << 20) + div - 1) // div
            assert top < 4096 * 4 and all((j * magic) >> 20 == j // div for j in range(top)), (g, div)


# ------------------------------------------------------------------------------------------------ GPU
SCRIPT = r"""
import ctypes as C, os, sys, time
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import cases, pair_sweeps as ps
from cases import pkg
family, todo = %(family)r, %(todo)r
fe = pkg.load_frontend("standalone")
hip, opt = pkg.load_backend(fe)
opt.shl_mi355x_registry_get.restype = C.c_void_p
opt.shl_mi355x_registry_get.argtypes = [C.c_void_p]
dev = cases.HipDevice(hip)
BAND = 4096
# (every HIP error raises: the sub-process prints what it has, exits non-zero and launches nothing further)


def differing(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.int8:
        return cases.mismatch_report(a, b)
    return int((a.view(np.uint16) != b.view(np.uint16)).sum()), "%%.3g" %% float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


def fused_into_guarded(plan_a, plan_b, d_in, nb, n, fill):
    buf = dev.alloc(nb + 2 * BAND)
    pkg.check(hip.shl_mi355x_memset(buf, fill, nb + 2 * BAND, None), hip, "memset")
    pkg.check(hip.shl_mi355x_pwdw_forward(plan_a, plan_b, d_in, buf + BAND, n, None), hip, "pwdw_forward")
    raw = dev.download(buf, (nb + 2 * BAND,), np.uint8)
    dev.free(buf)
    return raw, int((raw[:BAND] != fill).sum()), int((raw[BAND + nb:] != fill).sum())


for i in todo:
    t0 = time.time()
    pair, seed, env = ps.draw(family, i), ps.case_seed(family, i), ps.case_env(family, i)
    for v in ps.CASE_SWITCHES:
        os.environ.pop(v, None)
    os.environ.update(env)
    recs = []
    for kw, sd in ((pair["first"], seed), (pair["second"], seed + ps.SECOND_SEED)):
        kw = dict(kw)
        layout = cases.NCHW if kw.pop("layout", "NHWC") == "NCHW" else cases.NHWC
        recs.append(cases.make_case(sd, layout=layout, **kw))
    first, second = recs
    ps.couple(first, second, pair["zp"])
    form_name = "exact" if first["dtype"] == "int8" else "f16"
    # 1. both layers stand-alone, the second fed the first's output; the plans are kept
    keep = []
    mid = cases.csinn_run(fe, pkg.API_MI355X, first, device=dev, keep_params=keep)
    second["input"] = mid
    alone = cases.csinn_run(fe, pkg.API_MI355X, second, device=dev, keep_params=keep)
    name = opt.shl_mi355x_params_kernel_name(keep[0][0]).decode()
    plan_a, plan_b = (opt.shl_mi355x_registry_get(p) for p, _ in keep)
    assert plan_a and plan_b, "no plan behind a layer's params"
    # 2. the form, and the geometry the library chooses
    form = hip.shl_mi355x_pwdw_form(plan_a, plan_b, first["n"])
    geo = "-"
    if family == "pwdw_i8" and form == 1:
        g = (C.c_int32 * 12)()
        pkg.check(hip.shl_mi355x_pwdw_geometry(plan_a, plan_b, first["n"], g, 12), hip, "pwdw_geometry")
        geo = ",".join(str(v) for v in g)
    # 3. the oracle chain
    o_mid = cases.oracle_run(first, form_name)
    o_second = dict(second)
    o_second["input"] = o_mid
    want = cases.oracle_run(o_second, form_name)
    bad_mid, _ = differing(mid, o_mid)
    bad_alone, worst_alone = differing(alone, want)
    bad_fused = worst_fused = front = back = differ = refill = "-"
    if form == ps.FAMILIES[family]["form"]:   # (a pair that would fall back is reported, not launched)
        nb = alone.nbytes
        alone_bytes = np.ascontiguousarray(alone).view(np.uint8).reshape(-1)
        d_in = dev.alloc(first["input"].nbytes)
        dev.upload(d_in, first["input"])
        # 4. the fused launch between two guard bands
        raw, front, back = fused_into_guarded(plan_a, plan_b, d_in, nb, first["n"], 0x5A)
        got = raw[BAND:BAND + nb]
        differ = int((got != alone_bytes).sum())
        bad_fused, worst_fused = differing(got.view(alone.dtype).reshape(alone.shape), want)
        # 5. ... and again under the other fill
        raw2, front2, back2 = fused_into_guarded(plan_a, plan_b, d_in, nb, first["n"], 0xA5)
        refill = int((raw2[BAND:BAND + nb] != got).sum()) + front2 + back2
        dev.free(d_in)
    for p, _ in keep:
        opt.shl_mi355x_release_params(p)
    print("CASE", i, form, name, geo, bad_mid, bad_alone, worst_alone, bad_fused, worst_fused, differ, front, back, refill,
          "%%.2f" %% (time.time() - t0), flush=True)
"""
# switches of the fused forms that must not leak in from the caller's environment
FOREIGN = ("SHL_MI355X_PWDW", "SHL_MI355X_PWDW_TILE", "SHL_MI355X_PWDW_XG", "SHL_MI355X_NO_FUSION", "SHL_MI355X_DWPW", "SHL_MI355X_DWPW_RES",
           "SHL_MI355X_STEM_MFMA", "SHL_MI355X_IGEMM")


def run_cases(family, todo):
    env = dict(os.environ, SHL_MI355X_TUNE="0")   # the selection is by rule, not measured
    for v in ps.CASE_SWITCHES + FOREIGN:
        env.pop(v, None)
    res = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=ROOT, family=family, todo=todo)], capture_output=True, text=True,
                         timeout=300, env=env)
    rows = {int(l.split()[1]): l.split() for l in res.stdout.splitlines() if l.startswith("CASE")}
    for l in res.stdout.splitlines():
        print(l)
    assert len(rows) == len(todo) and res.returncode == 0, res.stdout + res.stderr
    return rows


def check_row(family, i, pair, env, row):
    what = "%s case %d: make_case(%d, **%r) -> make_case(%d, **%r), intermediate zero point %r, with %r" % (
        family, i, ps.case_seed(family, i), pair["first"], ps.case_seed(family, i) + ps.SECOND_SEED, pair["second"], pair["zp"], env)
    _, _, form, name, geo, bad_mid, bad_alone, worst_alone, bad_fused, worst_fused, differ, front, back, refill, _ = row
    assert form == str(ps.FAMILIES[family]["form"]), "%s: shl_mi355x_pwdw_form is %s" % (what, form)
    if family == "stemdw_i8":
        assert name == ps.stem_kernel(pair["first"]), "%s: the stem ran on %s" % (what, name)
    if family == "pwdw_i8":
        g = ps.pwdw_geometry(pair)
        mine = ",".join(str(g[k]) for k in ps.GEOMETRY_FIELDS)
        assert geo == mine, "%s: shl_mi355x_pwdw_geometry gives %s, the restatement %s (%s)" % (what, geo, mine, ", ".join(ps.GEOMETRY_FIELDS))
    assert bad_mid == "0" and bad_alone == "0", "%s: the stand-alone launches differ from the oracle chain in %s + %s places (worst %s)" % (what, bad_mid, bad_alone, worst_alone)
    assert bad_fused == "0", "%s: the fused launch differs from the oracle chain in %s places (worst %s)" % (what, bad_fused, worst_fused)
    assert differ == "0", "%s: %s bytes of the fused launch differ from the stand-alone launches" % (what, differ)
    assert front == "0" and back == "0", "%s: %s bytes in front of the output and %s behind it were written" % (what, front, back)
    assert refill == "0", "%s: %s bytes differ when the allocation is filled with 0xA5 instead of 0x5A" % (what, refill)


def test_a_row_that_is_wrong_in_any_column_is_reported_with_its_shape():
    for family, i in (("pwdw_i8", 9), ("stemdw_i8", 14), ("stemdw_f16_nchw", 5)):
        pair, env = ps.draw(family, i), ps.case_env(family, i)
        geo = ",".join(str(ps.pwdw_geometry(pair)[k]) for k in ps.GEOMETRY_FIELDS) if family == "pwdw_i8" else "-"
        name = {"pwdw_i8": "conv_igemm_tile_i8_mfma32x32x32", "stemdw_i8": "conv_stem_i8_dot4", "stemdw_f16_nchw": "conv_direct_f16"}[family]
        good = ["CASE", str(i), str(ps.FAMILIES[family]["form"]), name, geo, "0", "0", "0", "0", "0", "0", "0", "0", "0", "0.01"]
        check_row(family, i, pair, env, good)
        wrong = [(2, "0"), (2, "6"), (5, "3"), (6, "1"), (8, "2"), (8, "-"), (10, "32"), (10, "-"), (11, "1"), (12, "4096"), (13, "7"), (13, "-")]
        if family == "pwdw_i8":
            fields = geo.split(",")
            wrong += [(4, ",".join(fields[:k] + [str(int(fields[k]) + 1)] + fields[k + 1:])) for k in range(12)] + [(4, "-")]
        if family == "stemdw_i8":
            wrong += [(3, "conv_stem_i8_mfma32x32x32")]
        for col, value in wrong:
            row = list(good)
            row[col] = value
            with pytest.raises(AssertionError) as e:
                check_row(family, i, pair, env, row)
            assert repr(pair["first"]) in str(e.value) and repr(pair["second"]) in str(e.value) and str(ps.case_seed(family, i)) in str(e.value), (family, col)


@pytest.mark.gpu
@pytest.mark.parametrize("family,lo", ps.chunks(), ids=["%s-%d" % c for c in ps.chunks()])
def test_fused_pair_is_bit_exact_and_stays_inside_its_output(family, lo):
    todo = list(range(lo, min(lo + ps.CHUNK, ps.FAMILIES[family]["n"])))
    t0 = time.time()
    rows = run_cases(family, todo)
    print("%s-%d: %.1f s" % (family, lo, time.time() - t0))
    for i in todo:
        check_row(family, i, ps.draw(family, i), ps.case_env(family, i), rows[i])

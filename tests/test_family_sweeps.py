"""Seeded shape sweeps (tests/family_sweeps.py) over the kernels a size rule turns on -- dwconv_mfma.hip, conv1x1_stream.hip,
conv1x1_resident.hip, conv1x1_latency.hip, the MFMA form of conv_stem.hip, conv_gemv.hip -- each forced by its switch; and over
the NCHW-native kernels that their shapes alone select, int8 and binary16: families "nchw1x1" (nchw_small.hip: the staged kernel
with transposing LDS reads over 4 / 8 / 16 waves, the gather kernel beyond 2048 bytes of K), "dwconv3x3_nchw" (its depthwise
3 x 3) and "stem_f16_nchw" (conv_direct.hip: the binary16 stem).

CPU: the draws are reproducible, fill every stratum, stay under the MAC cap and inside the forced kernel's domain.
GPU: per chunk of eight cases one sub-process (the switches are read once per process) runs every case through csinn_* on
device tensors: the forced kernel's name, zero mismatches against the exact oracle (binary16 GEMV: 1e-3; binary16 cases of the
NCHW-native families: zero differing words -- the depthwise and stem kernels sum in the reference's order, the pointwise
kernels run on operands whose fp32 sums are exact in any order), then the same plan
again through shl_mi355x_conv_forward into a buffer with 4 KiB of 0x5A on either side -- the same bytes, the bands untouched
(the ragged-tile stores of these kernels are guarded in hand-unrolled epilogues)."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import family_sweeps as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(f, i) for f in fs.FAMILIES for i in range(fs.FAMILIES[f]["n"])]


def count(family, key):
    return collections.Counter(key(i, fs.draw(family, i)) for i in range(fs.FAMILIES[family]["n"]))


# ------------------------------------------------------------------------------------------------ CPU: the draws
def test_draws_are_reproducible_and_the_seed_moves_only_the_free_parameters():
    assert [fs.FAMILIES[f]["n"] for f in fs.FAMILIES] == [40, 32, 32, 32, 32, 32, 48, 32, 16]
    moved = 0
    for f, i in ALL:
        a = fs.draw(f, i)
        assert a == fs.draw(f, i), (f, i)
        b = fs.draw(f, i, seed=fs.BASE_SEED + 1)
        moved += a != b
        assert fs.admissible(f, b) and fs.geometry(b)["macs"] <= fs.FAMILIES[f]["cap"], (f, i, b)
    assert moved > len(ALL) // 2


@pytest.mark.parametrize("family", list(fs.FAMILIES))
def test_every_case_is_under_the_mac_cap_and_inside_the_forced_kernels_domain(family):
    total = 0
    for i in range(fs.FAMILIES[family]["n"]):
        kw = fs.draw(family, i)
        g = fs.geometry(kw)
        assert g["ho"] >= 1 and g["wo"] >= 1 and g["macs"] <= fs.FAMILIES[family]["cap"], (i, kw, g)
        assert fs.admissible(family, kw), (i, kw)   # the share that may fall back is zero
        total += g["macs"]
    assert total <= 30e9, total   # ~20 s of the CPU oracle per family at the most (conv1x1_resident, over eight tests)


def test_dwconv_mfma_strata():
    F = "dwconv_mfma"
    geo = lambda kw: fs.dwm_geometry(kw["c"], kw["stride"][0], kw["stride"][1], fs.geometry(kw)["ho"], fs.geometry(kw)["wo"])
    pairs = count(F, lambda i, kw: (geo(kw)["cb"], kw["stride"]))
    assert len(pairs) == 12 and min(pairs.values()) >= 2, pairs
    woc = lambda wo: "le8" if wo <= 8 else ("9to16" if wo <= 16 else "gt16")
    hoc = lambda ho: "le4" if ho <= 4 else ("5to8" if ho <= 8 else "ge9")
    cls = count(F, lambda i, kw: (woc(fs.geometry(kw)["wo"]), hoc(fs.geometry(kw)["ho"])))
    assert len(cls) == 9 and min(cls.values()) >= 2, cls
    for i in range(40):
        kw, s = fs.draw(F, i), fs.dw_strata(i)
        assert (geo(kw)["cb"], kw["stride"], woc(fs.geometry(kw)["wo"]), hoc(fs.geometry(kw)["ho"])) == (s["cb"], s["stride"], s["wo_class"], s["ho_class"])
        assert kw["c"] in fs.DW_C[s["cb"]] and all(p in (0, 1, 2) for p in kw["pad"]) and 1 <= kw["n"] <= 5
    # what the issue names: stride (1, 2) (the stride-2 swizzle with stride-1 rows) and 128-channel blocks at stride 2 on a wide map
    assert sum(1 for i in range(40) if fs.draw(F, i)["stride"] == (1, 2)) >= 6
    assert any(geo(kw)["cb"] == 128 and kw["stride"] == (2, 2) and fs.geometry(kw)["wo"] > 8 and geo(kw)["tiles_y"] > 1
               for kw in (fs.draw(F, i) for i in range(40)))
    assert len(count(F, lambda i, kw: geo(kw)["btx"])) == 2
    # the LAUNCHED rows of tiles: every value, every starting value, and the shrink loop from four rows to three, two and one
    launched = count(F, lambda i, kw: (geo(kw)["bty0"], geo(kw)["bty"]))
    assert {b for _, b in launched} == {1, 2, 3, 4} and {(4, 4), (4, 3), (4, 2), (4, 1), (2, 2), (2, 1), (1, 1)} <= set(launched), launched
    per_pair = collections.defaultdict(set)
    for i in range(40):
        kw = fs.draw(F, i)
        per_pair[(geo(kw)["cb"], kw["stride"])].add(hoc(fs.geometry(kw)["ho"]))
    assert all(len(v) == 3 for v in per_pair.values()), per_pair   # the Ho class is no function of the pair
    assert any(geo(fs.draw(F, i))["tiles_x"] > 1 and geo(fs.draw(F, i))["tiles_y"] > 1 for i in range(40))
    pads = count(F, lambda i, kw: kw["pad"])
    assert len(pads) >= 15
    # epi_code 0, 1, 3, 4 (2 and 5 cannot be reached: family_sweeps' docstring); per-channel tables both ways
    assert sorted(count(F, lambda i, kw: fs.epi_code(kw))) == [0, 1, 3, 4]
    assert len(count(F, lambda i, kw: (kw["act"], kw["exact"]))) == 6 and len(count(F, lambda i, kw: kw["per_channel"])) == 2


def test_conv1x1_stream_strata():
    F = "conv1x1_stream"
    ncg = lambda co: 4 if co % 128 == 0 else 2
    pairs = count(F, lambda i, kw: (kw["c"], ncg(kw["co"])))
    assert len(pairs) == 10 and min(pairs.values()) >= 2, pairs
    res, joint = collections.Counter(), collections.Counter()
    small = set()
    for i in range(32):
        kw = fs.draw(F, i)
        M, T = fs.geometry(kw)["M"], fs.stream_tile(kw["c"])
        assert kw["co"] % 64 == 0 and kw["n"] > 1 and kw["h"] != kw["w"]
        if M < T:
            small.add(kw["c"])
        else:
            res[M % T if M % T != T - 1 else "T-1"] += 1
            joint[(ncg(kw["co"]), M % T if M % T != T - 1 else "T-1")] += 1
    assert small == set(fs.ST_C)
    assert set(res) == {0, 1, 31, 32, 33, "T-1"} and min(res.values()) >= 4, res
    assert len(joint) == 12, joint   # both channel-group counts meet every residue


def test_conv1x1_resident_strata():
    F = "conv1x1_resident"
    pairs = count(F, lambda i, kw: (kw["c"], kw["co"]))
    assert len(pairs) == 16 and min(pairs.values()) >= 1, pairs
    modes, lasts, stages = collections.Counter(), collections.Counter(), collections.Counter()
    ranges = collections.defaultdict(set)
    for i in range(32):
        kw = fs.draw(F, i)
        M, tpx = fs.geometry(kw)["M"], fs.resident_tile(kw["c"])
        nb, r, tiles = fs.resident_geom(M, kw["c"], kw["co"])
        per = fs.resident_range_tiles(tiles, r)
        assert min(per) >= 3 and sum(per) == tiles
        modes["exact3" if tiles == 3 * r else "plus1" if tiles == 3 * r + 1 else "ragged" if tiles % r else "even"] += 1
        ranges["exact3" if tiles == 3 * r else "plus1" if tiles == 3 * r + 1 else "ragged" if tiles % r else "even"].add(r)
        ranges["all"].add(r)
        modes["six tiles"] += max(per) >= 6
        modes["eight blocks"] += nb == 8
        if kw["c"] == 1024:
            stages[(min(per) * 2, max(per) * 2)] += 1
        last = M - (tiles - 1) * tpx
        lasts["full" if last == tpx else last] += 1
    assert modes["exact3"] >= 6 and modes["plus1"] >= 6 and modes["ragged"] >= 8 and modes["six tiles"] >= 4 and modes["eight blocks"] >= 8, modes
    # the workgroup -> (XCD, slot) -> range arithmetic and tiles * range / ranges: 8 ranges is one per XCD (slot / ncb = 0), more
    # put several on an XCD; each tile-count mode at more than one ranges value
    assert len(ranges["all"]) >= 3 and max(ranges["all"]) // 8 > 1, ranges
    assert all(len(ranges[m]) >= 2 for m in ("exact3", "plus1", "ragged")), ranges
    # K = 1024: every workgroup at exactly three tiles = six stages (one turn of the ring), and some workgroup at six tiles =
    # twelve stages, the most the MAC cap allows (family_sweeps' docstring)
    assert stages[(6, 6)] >= 1 and any(hi >= 12 for _, hi in stages), stages
    assert set(lasts) == {1, 31, 32, 33, "full"} and min(lasts.values()) >= 2, lasts
    assert len(count(F, lambda i, kw: (kw["act"], kw["exact"]))) == 6


def test_conv1x1_latency_strata():
    F = "conv1x1_latency"
    forms = count(F, lambda i, kw: fs.latency_form(kw, fs.case_env(F, i)))
    assert set(forms) == {"mt1", "zsplit", "mt2"} and min(forms.values()) >= 6, forms
    for i in range(32):
        assert fs.latency_form(fs.draw(F, i), fs.case_env(F, i)) == fs.latency_strata(i)["form"]
    # mt = 2 both ways: by the product, and by the switch on a shape that would split.  (The form a launch took cannot be read
    # back from the device: the by-switch cases are checked against this restatement of launch_lat only; on the device they
    # assert the results of whichever form ran.)
    assert sum(1 for i in range(32) if fs.latency_form(fs.draw(F, i), {}) == "mt2") >= 3
    assert sum(1 for i in range(32) if fs.case_env(F, i) and fs.latency_form(fs.draw(F, i), {}) == "zsplit") >= 3
    hw = count(F, lambda i, kw: kw["h"] * kw["w"])
    assert {1, 31, 32, 33, 63, 64} <= set(hw) and len(hw) >= 9, hw
    assert all(kw["h"] != kw["w"] or kw["h"] == 1 for kw in (fs.draw(F, i) for i in range(32)))
    assert set(count(F, lambda i, kw: kw["c"])) == {256, 512, 1024}
    assert set(count(F, lambda i, kw: kw["n"])) >= {1, 8}
    assert all(kw["co"] % 32 == 0 and 1 <= kw["n"] <= 8 for kw in (fs.draw(F, i) for i in range(32)))
    # the epilogue forms that can be reached (lat_epi 3 and 0), each with and without an activation
    assert len(count(F, lambda i, kw: (kw["exact"], kw["act"] > 0))) == 4


def test_stem_strata():
    F = "stem_mfma"
    assert set(count(F, lambda i, kw: kw["co"])) == {16, 32, 48, 64}
    assert len(count(F, lambda i, kw: kw["stride"])) == 4 and len(count(F, lambda i, kw: (kw["co"], kw["stride"]))) >= 12
    assert len(count(F, lambda i, kw: kw["pad"])) >= 15
    tiny = {(kw["n"], kw["h"], kw["w"]): kw for kw in (fs.draw(F, i) for i in range(32))}
    assert all(t in tiny for t in fs.STEM_TINY) and tiny[(2, 3, 3)]["pad"] == (2, 2, 2, 2)
    tpw = collections.Counter()
    for i in range(32):
        kw, s = fs.draw(F, i), fs.stem_strata(i)
        assert fs.case_env(F, i) == {"SHL_MI355X_STEM_TPW": str(s["tpw"])}
        assert len({fs.stem_strata(j)["tpw"] for j in range(i - i % 8, i - i % 8 + 8)}) == 1   # read once per process
        if s["tiny"]:
            continue
        tiles, t, waves = fs.stem_launch(fs.geometry(kw)["M"], s["tpw"])
        assert tiles > t and (t == 1 or tiles % t) and waves % 4 and fs.geometry(kw)["M"] % 32, (i, kw)
        tpw[t] += 1
    assert set(tpw) == {1, 2, 3, 8} and min(tpw.values()) >= 7
    g = fs.geometry(fs.STEM_RULE_CASE)
    assert g["M"] == 524288 and fs.stem_launch(g["M"], None)[1] == 2 and g["M"] * 32 >= 1 << 24   # the size rule picks it, two tiles per wave
    assert sorted(count(F, lambda i, kw: fs.epi_code(kw))) == [0, 1, 3, 4]


def test_conv_gemv_strata():
    F = "conv_gemv"
    kb = lambda kw: kw["c"] * (1 if kw["dtype"] == "int8" else 2)
    assert set(count(F, lambda i, kw: kb(kw))) == set(fs.GV_KBYTES)
    assert set(count(F, lambda i, kw: kw["co"])) == set(fs.GV_CO)
    assert min(count(F, lambda i, kw: (kw["dtype"], bool(kw.get("fc")))).values()) >= 6 and len(count(F, lambda i, kw: (kw["dtype"], bool(kw.get("fc"))))) == 4
    assert {kb(fs.draw(F, i)) for i in range(32) if fs.case_env(F, i)} == set(fs.GV_KBYTES)   # each K once with the four-channel form forced
    opw = count(F, lambda i, kw: (fs.gemv_opw(kw, fs.case_env(F, i)), fs.gemv_opw(kw, {})))
    assert opw[(2, 2)] >= 6 and opw[(4, 4)] >= 3 and opw[(4, 2)] >= 3, opw
    assert all(fs.geometry(kw)["M"] <= 8 for kw in (fs.draw(F, i) for i in range(32)))


def test_nchw1x1_strata():
    F = "nchw1x1"
    N = fs.FAMILIES[F]["n"]
    draws = [fs.draw(F, i) for i in range(N)]
    es = lambda kw: 1 if kw["dtype"] == "int8" else 2
    kb = lambda kw: kw["c"] * es(kw)
    geo = lambda kw: fs.nchw1x1_launch(kb(kw), kw["co"])
    for i, kw in enumerate(draws):
        s = fs.nchw1x1_strata(i)
        assert (kw["dtype"], kb(kw), kw["co"], kw["n"], kw["act"]) == (("int8", "f16")[i % 2], s["kbytes"], s["co"], s["n"], i % 3)
        assert kw["layout"] == "NCHW" and fs.geometry(kw)["layout"] == "NCHW" and 1 <= kw["n"] <= 3
    for dt in ("int8", "f16"):
        mine = [kw for kw in draws if kw["dtype"] == dt]
        assert len(mine) == N // 2 and {kb(kw) for kw in mine} == set(fs.NC_KBYTES), dt
        paths = collections.Counter((geo(kw)["staged"], geo(kw)["frag"]) for kw in mine)
        assert len(paths) == 4 and min(paths.values()) >= 2, (dt, paths)   # staged / gather x fragment-ordered / row-ordered weights
        assert len({kw["act"] for kw in mine}) == 3
    assert {kw["co"] for kw in draws} == set(fs.NC_CO)
    # what the K rows are in the table for, by the restatement of launch_conv1x1_nchw
    rows = {k: fs.nchw1x1_launch(k) for k in fs.NC_KBYTES}
    pad = lambda k: rows[k]["kstride"] - k
    assert any(pad(k) >= 32 for k in rows) and any(pad(k) % 32 == 16 for k in rows)    # a sub-step of padding alone; one that is half padding
    assert any(min(g["wave_nsub"][:4]) <= 0 for g in rows.values())                    # a finishing wave with no K of its own
    assert any(0 < g["wave_nsub"][w] < g["per"] for g in rows.values() for w in range(g["waves"]))   # a short last wave
    assert any(g["waves"] == 8 and 0 in g["wave_nsub"] for g in rows.values())         # eight waves, idle ones among them
    assert any(g["waves"] == 16 and min(g["wave_nsub"]) > 0 for g in rows.values())
    assert any(g["waves"] == 16 and g["staged"] and min(g["wave_nsub"]) < 0 for g in rows.values())   # a start beyond the end: the clamp
    assert any(not g["staged"] and min(g["wave_nsub"]) < 0 for g in rows.values())
    assert {g["waves"] for g in rows.values()} == {4, 8, 16}
    assert any(g["staged"] and g["waves"] * g["per"] * 1024 == 65536 for g in rows.values())   # the largest staged row: 64 KiB
    assert sorted(k for k, g in rows.items() if not g["staged"]) == [2080, 4096, 4112]
    assert all(g["staged"] == (fs.align_up(k, 64) <= 2048) for k, g in rows.items())            # "the packed K row exceeds 2048 bytes"
    # the map
    hw = [kw["h"] * kw["w"] for kw in draws]
    res = collections.Counter("0" if v % 32 == 0 else "1..15" if v % 32 < 16 else "16" if v % 32 == 16 else "17..31" for v in hw)
    assert len(res) == 4 and min(res.values()) >= 4, res
    assert sum(v < 16 for v in hw) >= 4 and sum(33 <= v <= 63 for v in hw) >= 4 and sum(v >= 100 for v in hw) >= 4, hw
    assert sum(kw["h"] != kw["w"] for kw in draws) > N // 2
    staged = [kw for kw in draws if geo(kw)["staged"]]
    odd = sum((kw["h"] * kw["w"] * es(kw)) % 16 != 0 for kw in staged)
    assert 3 * odd >= len(staged) and 3 * (len(staged) - odd) >= len(staged), (odd, len(staged))   # misaligned planes; aligned ones
    for dt in ("int8", "f16"):   # ... and a misaligned plane on more than one pixel tile, where pieces of the next plane are staged
        assert any(kw["dtype"] == dt and kw["h"] * kw["w"] > 32 and (kw["h"] * kw["w"] * es(kw)) % 16 for kw in staged), dt
    assert any(kw["h"] * kw["w"] > 32 for kw in draws if not geo(kw)["staged"])
    assert 2 * sum(kw["n"] > 1 for kw in draws) >= N
    tiny = [kw for kw in draws if kw["n"] * kw["h"] * kw["w"] <= 8 and kw["h"] * kw["w"] >= 2]   # the NHWC view is the GEMV's
    assert len(tiny) >= 2 and len({kw["dtype"] for kw in tiny}) == 2, tiny
    i8 = [kw for kw in draws if kw["dtype"] == "int8"]
    assert [kw["exact"] for kw in i8] == [j % 2 == 0 for j in range(len(i8))]
    assert len({kw["per_channel"] for kw in i8}) == 2
    assert len({(kw["exact"], kw["act"]) for kw in i8}) == 6


def test_nchw1x1_binary16_operands_sum_exactly_in_any_order():
    F = "nchw1x1"
    seen = 0
    for i in range(fs.FAMILIES[F]["n"]):
        kw = fs.draw(F, i)
        if kw["dtype"] == "int8":
            continue
        case = dict(seed=fs.case_seed(F, i), in_shape=(kw["n"], kw["c"], kw["h"], kw["w"]), w_shape=(kw["co"], kw["c"], 1, 1), co=kw["co"])
        again = fs.exact_f16_operands(dict(case))
        fs.exact_f16_operands(case)
        for key in ("input", "kernel", "bias"):
            v = case[key].astype(np.float64) * 16
            assert case[key].dtype == np.float16 and np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 32, (i, key)
            assert np.array_equal(case[key], again[key])
        x = np.abs(case["input"].astype(np.float64) * 16).transpose(0, 2, 3, 1).reshape(-1, kw["c"])
        w = np.abs(case["kernel"].astype(np.float64) * 16).reshape(kw["co"], kw["c"])
        worst = float((x @ w.T).max())   # sum |16 x| |16 w| over K: every partial sum, in units of 2^-8, is below it
        assert worst < 2 ** 24, (i, kw, worst)
        assert 4 * kw["c"] + 2 < 65504   # |S + bias| stays a finite binary16
        seen += 1
    assert seen == fs.FAMILIES[F]["n"] // 2


def test_dwconv3x3_nchw_strata():
    F = "dwconv3x3_nchw"
    N = fs.FAMILIES[F]["n"]
    draws = [fs.draw(F, i) for i in range(N)]
    geo = [fs.geometry(kw) for kw in draws]
    for i, kw in enumerate(draws):
        s = fs.dwn_strata(i)
        assert (kw["stride"], kw["dilation"], kw["c"], kw["n"], kw["dtype"]) == (s["stride"], s["dilation"], s["c"], s["n"], s["dtype"])
        assert kw["layout"] == "NCHW" and kw["depthwise"] and all(p in (0, 1, 2) for p in kw["pad"])
    assert {kw["stride"] for kw in draws} == {(1, 1), (2, 2), (1, 2), (3, 2)}
    assert {kw["dilation"] for kw in draws} == {(1, 1), (2, 2), (1, 2)}
    assert 3 * sum(kw["dilation"] != (1, 1) for kw in draws) >= N
    assert len({(kw["stride"], kw["dilation"]) for kw in draws}) == 12
    assert len({kw["pad"] for kw in draws}) >= 12
    assert sum(kw["pad"][0] != kw["pad"][2] or kw["pad"][1] != kw["pad"][3] for kw in draws if kw["dilation"] != (1, 1)) >= 4   # dilation with asymmetric padding
    assert {kw["c"] for kw in draws} == {2, 3, 19, 32, 100} and {kw["n"] for kw in draws} == {1, 2, 3}
    assert {kw["c"] for kw in draws if kw["n"] > 1 and kw["c"] % 2} == {3, 19}   # c = plane % C on odd C behind the first image
    cls = lambda g: "lt256" if g["ho"] * g["wo"] < 256 else "eq256" if g["ho"] * g["wo"] == 256 else "257to511" if g["ho"] * g["wo"] < 512 else "gt512"
    maps = collections.Counter(cls(g) for g in geo)
    assert set(maps) == set(fs.DN_MAP) and min(maps.values()) >= 6 and all(g["ho"] * g["wo"] != 512 for g in geo), maps
    assert [cls(g) for g in geo] == [fs.dwn_strata(i)["map_class"] for i in range(N)]
    assert len({(kw["stride"], cls(g)) for kw, g in zip(draws, geo)}) == 16
    assert any(kw["stride"] == (3, 2) and g["ho"] * g["wo"] > 256 for kw, g in zip(draws, geo))
    assert any(g["ho"] == 1 or g["wo"] == 1 for g in geo)
    for dt in ("int8", "f16"):
        mine = [(kw, g) for kw, g in zip(draws, geo) if kw["dtype"] == dt]
        assert len(mine) == N // 2 and {cls(g) for _, g in mine} == set(fs.DN_MAP) and {kw["act"] for kw, _ in mine} == {0, 1, 2}, dt
        assert len({kw["stride"] for kw, _ in mine}) == 4 and len({kw["dilation"] for kw, _ in mine}) == 3, dt
    i8 = [kw for kw in draws if kw["dtype"] == "int8"]
    assert len({kw["exact"] for kw in i8}) == 2 and len({kw["per_channel"] for kw in i8}) == 2 and len({(kw["exact"], kw["act"] > 0) for kw in i8}) == 4


def test_stem_f16_nchw_strata():
    F = "stem_f16_nchw"
    N = fs.FAMILIES[F]["n"]
    draws = [fs.draw(F, i) for i in range(N)]
    assert all(kw["layout"] == "NCHW" and kw["dtype"] == "f16" and kw["c"] == 3 and kw.get("k", (3, 3)) == (3, 3) for kw in draws)
    assert {kw["co"] for kw in draws} == {1, 7, 8, 20, 33, 64}
    assert {kw["stride"] for kw in draws} == {(1, 1), (2, 2), (2, 1)} and {kw["dilation"] for kw in draws} == {(1, 1), (2, 2)}
    assert len({(kw["stride"], kw["dilation"]) for kw in draws}) == 6
    assert len({kw["pad"] for kw in draws}) >= 8 and {kw["n"] for kw in draws} == {1, 2, 3} and {kw["act"] for kw in draws} == {0, 1}
    threads = [fs.stem_f16_threads(kw) for kw in draws]
    assert sum(t < 256 for t in threads) == N // 2 and sum(t >= 257 and t % 256 != 0 for t in threads) == N // 2, threads
    # both launch sizes meet ragged channel groups (Co % 8 != 0), full ones, and both dilations
    for small in (True, False):
        mine = [kw for kw, t in zip(draws, threads) if (t < 256) == small]
        assert {kw["co"] % 8 == 0 for kw in mine} == {True, False} and {kw["dilation"] for kw in mine} == {(1, 1), (2, 2)}, small


# ------------------------------------------------------------------------------------------------ GPU
SCRIPT = r"""
import os, sys, time
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import cases, golden_util, family_sweeps as fs
from cases import pkg
family, todo = %(family)r, %(todo)r
fe = pkg.load_frontend("standalone")
hip, opt = pkg.load_backend(fe)
dev = cases.HipDevice(hip)
BAND = 4096
for i in todo:
    t0 = time.time()
    if i == "rule":
        kw, seed, env = dict(fs.STEM_RULE_CASE), 910999, {}
    else:
        kw, seed, env = fs.draw(family, i), fs.case_seed(family, i), fs.case_env(family, i)
    for v in fs.CASE_SWITCHES:
        os.environ.pop(v, None)
    os.environ.update(env)
    kw = dict(kw)
    layout = cases.NCHW if kw.pop("layout", "NHWC") == "NCHW" else cases.NHWC
    case = cases.make_case(seed, layout=layout, **kw)
    if family == "nchw1x1" and case["dtype"] != "int8":
        fs.exact_f16_operands(case)   # fp32 sums that are exact in the MFMA's order as in the reference's
    keep = []
    got = cases.csinn_run(fe, pkg.API_MI355X, case, device=dev, keep_params=keep)
    name = opt.shl_mi355x_params_kernel_name(keep[0][0]).decode()
    if case["dtype"] == "int8":
        bad, worst = cases.mismatch_report(got, cases.oracle_run(case, "exact"))
    elif family in fs.NCHW_NATIVE:   # bit for bit
        want = cases.oracle_run(case, "f16")
        bad = int((np.ascontiguousarray(got).view(np.uint16) != want.view(np.uint16)).sum())
        worst = "%%.3g" %% float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    else:
        bad, worst = 0, 0
        try:
            golden_util.compare_f16_tol(got, cases.oracle_run(case, "f16"), "binary16 GEMV")
        except AssertionError as e:
            bad, worst = 1, str(e).replace(" ", "_")
    # the same plan once more, into the middle of a larger allocation
    plan = opt.shl_mi355x_registry_get(keep[0][0])
    assert plan, "no plan behind the layer's params"
    nb = got.nbytes
    buf = dev.alloc(nb + 2 * BAND)
    pkg.check(hip.shl_mi355x_memset(buf, 0x5A, nb + 2 * BAND, None), hip, "memset")
    d_in = dev.alloc(case["input"].nbytes)
    dev.upload(d_in, case["input"])
    pkg.check(hip.shl_mi355x_conv_forward(plan, d_in, buf + BAND, case["n"], None), hip, "conv_forward")
    raw = dev.download(buf, (nb + 2 * BAND,), np.uint8)
    front, back = int((raw[:BAND] != 0x5A).sum()), int((raw[BAND + nb:] != 0x5A).sum())
    differ = int((raw[BAND:BAND + nb] != np.ascontiguousarray(got).view(np.uint8).reshape(-1)).sum())
    dev.free(buf)
    dev.free(d_in)
    for p, _ in keep:
        opt.shl_mi355x_release_params(p)
    print("CASE", i, name, bad, worst, front, back, differ, "%%.2f" %% (time.time() - t0), flush=True)
"""


def run_cases(family, todo, extra_env=None):
    env = dict(os.environ, SHL_MI355X_TUNE="0")   # a kernel A/B: the selection is forced, not measured
    for v in fs.CASE_SWITCHES:
        env.pop(v, None)
    env.update(fs.FAMILIES[family]["env"])
    env.update(extra_env or {})
    env = {k: v for k, v in env.items() if v is not None}   # None: the variable is taken away
    res = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=ROOT, family=family, todo=todo)], capture_output=True, text=True,
                         timeout=600, env=env)
    rows = {l.split()[1]: l.split() for l in res.stdout.splitlines() if l.startswith("CASE")}
    assert len(rows) == len(todo) and res.returncode == 0, res.stdout + res.stderr
    for l in res.stdout.splitlines():
        print(l)
    return rows


def check_row(family, i, kw, env, row, want_name):
    what = "%s case %s: make_case(%d, **%r) with %r" % (family, i, 910999 if i == "rule" else fs.case_seed(family, i), kw, env)
    _, _, name, bad, worst, front, back, differ, _ = row
    assert name == want_name, "%s ran on %s" % (what, name)
    assert bad == "0", "%s: %s mismatches against the oracle (worst %s)" % (what, bad, worst)
    assert differ == "0", "%s: %s bytes of the second run through conv_forward differ from the first" % (what, differ)
    assert front == "0" and back == "0", "%s: %s bytes in front of the output and %s behind it were written" % (what, front, back)


def test_a_row_that_is_wrong_in_any_column_is_reported_with_its_shape():
    kw = fs.draw("conv1x1_stream", 7)
    good = ["CASE", "7", "conv1x1_stream_i8_mfma32x32x32", "0", "0", "0", "0", "0", "0.01"]
    check_row("conv1x1_stream", 7, kw, {}, good, good[2])
    for col, value in ((2, "conv_igemm_tile_i8_mfma32x32x32"), (3, "5"), (5, "16"), (6, "16"), (7, "1")):
        row = list(good)
        row[col] = value
        with pytest.raises(AssertionError) as e:
            check_row("conv1x1_stream", 7, kw, {}, row, good[2])
        assert repr(kw) in str(e.value) and str(fs.case_seed("conv1x1_stream", 7)) in str(e.value)
    # a binary16 row of an NCHW-native family: `bad` counts differing words
    kw = fs.draw("nchw1x1", 21)
    good = ["CASE", "21", "conv1x1_nchw_f16", "0", "0", "0", "0", "0", "0.01"]
    check_row("nchw1x1", 21, kw, {}, good, fs.kernel_name("nchw1x1", kw))
    for col, value in ((2, "conv_igemm_wave_f16_mfma32x32x16"), (2, "conv_gemv_f16_fma"), (3, "1"), (5, "2"), (6, "2"), (7, "4")):
        row = list(good)
        row[col] = value
        with pytest.raises(AssertionError) as e:
            check_row("nchw1x1", 21, kw, {}, row, good[2])
        assert repr(kw) in str(e.value) and str(fs.case_seed("nchw1x1", 21)) in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("family,lo", fs.chunks(), ids=["%s-%d" % c for c in fs.chunks()])
def test_forced_kernel_is_bit_exact_and_stays_inside_its_output(family, lo):
    todo = list(range(lo, min(lo + fs.FAMILIES[family].get("chunk", fs.CHUNK), fs.FAMILIES[family]["n"])))
    # a switch that is read once per process must be there from the start (the stem's tiles per wave: uniform per chunk)
    rows = run_cases(family, todo, fs.case_env(family, lo) if family == "stem_mfma" else None)
    for i in todo:
        kw = fs.draw(family, i)
        check_row(family, i, kw, fs.case_env(family, i), rows[str(i)], fs.kernel_name(family, kw))


@pytest.mark.gpu
def test_stem_pipeline_at_the_size_the_rule_itself_sets_two_tiles_per_wave():
    """n = 2, 1024 x 1024 x 3, stride 2, 32 channels: 524 288 output pixels, the smallest map at which launch_conv_stem
    sets two tiles per wave without SHL_MI355X_STEM_TPW -- and the size rule, not the switch, picks the MFMA form"""
    env = {"SHL_MI355X_STEM_MFMA": None}
    rows = run_cases("stem_mfma", ["rule"], env)
    check_row("stem_mfma", "rule", fs.STEM_RULE_CASE, env, rows["rule"], "conv_stem_i8_mfma32x32x32")

"""Seeded sweeps (tests/post_op_sweeps.py) of the fused post-op launches over every kernel flavour that carries them: the residual
tail and the table post-op on the 14 flavours of the wave and tile implicit-GEMM kernels crossed with the requantisation codes
0, 1, 3, 4 -- each of the 2 x 56 instantiations conv_igemm.hip:launch_wave_regs_tile can reach, twice -- and the table post-op on
the three depthwise kernels.

CPU: the draws are reproducible, fill every cell of the cross and every rotating stratum, stay under the MAC cap and inside the
entry points' domain; the oracle chains can tell results apart.
GPU: the checks of the hand lists (residual_cases / act_fuse_cases / dw_act_cases .check_case: fused and unfused against the
oracle chain byte for byte, fused equal to unfused, guard bands untouched) on every case, and after each fused launch
shl_mi355x_last_igemm_flavour() against post_op_sweeps.flavour_of.  Cases of the flavours a once-per-process switch selects run
in one child process per environment; after a child that ended by a signal or at its time limit no further child starts."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import family_sweeps as fs
import post_op_sweeps as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV = ("conv_add", "conv_lut")
ALL = [(f, i) for f in ps.FAMILIES for i in range(ps.FAMILIES[f]["n"])]
OTHER_SEEDS = (ps.BASE_SEED + 1, ps.BASE_SEED + 2)


# ------------------------------------------------------------------------------------------------ CPU: the draws
def test_draws_are_reproducible_and_the_seed_moves_only_the_free_parameters():
    assert [ps.FAMILIES[f]["n"] for f in ps.FAMILIES] == [112, 112, 88]
    moved = 0
    for f, i in ALL:
        a = ps.draw(f, i)
        ps._DRAWN.clear()
        assert a == ps.draw(f, i), (f, i)
        for seed in OTHER_SEEDS:
            b = ps.draw(f, i, seed=seed)
            moved += a != b
            assert ps.macs(b) <= ps.FAMILIES[f]["cap"], (f, i, b)
            if f in CONV:   # the cell and every stratum are the index's, whatever the seed
                assert ps.flavour_of(b, ps.case_env(f, i), ps.POST[f]) == cell_of(f, i), (f, i, b)
                assert conv_classes(f, i, b) == conv_classes(f, i, a), (f, i, a, b)
            else:
                assert ps.dw_kernel_of(b, ps.case_env(f, i)) == ps.strata(f, i)["kernel"], (f, i, b)
    assert moved > len(ALL)


def cell_of(family, i):
    s = ps.strata(family, i)
    return "%s/epi%d+%s" % (s["flavour"], s["code"], ps.POST[family])


def conv_classes(family, i, kw):
    """the strata of a conv_add / conv_lut draw, read off the draw alone"""
    s = ps.strata(family, i)
    tbm, tbn = ps.tile_of(s["flavour"])
    g = fs.geometry(kw)
    res = g["M"] % tbm
    kh, kw_ = kw["k"]
    if (kh, kw_) == (1, 1):
        window = "1x1" if kw["stride"] == (1, 1) else "1x1s2"
    elif (kh, kw_) == (3, 3):
        window = "3x3d2" if kw["dilation"] == (2, 2) else ("3x3s2" if kw["stride"] == (2, 2) else "3x3same")
    else:
        window = {(5, 5): "5x5", (1, 7): "1x7", (7, 1): "1x7", (7, 7): "7x7"}[(kh, kw_)]
    return dict(window=window, pixels="one" if res == 1 else ("last" if res == tbm - 1 else "other"), n=kw["n"], path=ps.store_path(kw["co"]),
                two=int(kw["co"] > tbn), per_channel=kw["per_channel"], code=fs.epi_code(kw))


@pytest.mark.parametrize("family", list(ps.FAMILIES))
def test_every_case_is_under_the_mac_cap_and_inside_the_entry_points_domain(family):
    total = 0
    for i in range(ps.FAMILIES[family]["n"]):
        kw = ps.draw(family, i)
        g = fs.geometry(kw)
        assert g["ho"] >= 1 and g["wo"] >= 1 and ps.macs(kw) <= ps.FAMILIES[family]["cap"], (i, kw, g)
        assert "layout" not in kw and "groups" not in kw and "dtype" not in kw   # NHWC, group 1, int8: make_case's defaults
        if family == "dw_lut":   # conv_plan.hip:choose_algo -> dwconv.hip:dwconv_supports: SHL_MI355X_ALGO_DW
            assert kw["depthwise"] and kw["c"] % 4 == 0 and kw["c"] > 1, (i, kw)
            assert ps.dw_kernel_of(kw, ps.case_env(family, i)) == ps.strata(family, i)["kernel"], (i, kw)
            if ps.strata(family, i)["kernel"] == "mfma":
                assert fs.admissible("dwconv_mfma", kw) and kw == fs.draw("dwconv_mfma", i)
        else:   # conv_igemm.hip:igemm_supports: SHL_MI355X_ALGO_IGEMM (C = 3 would be the stem's)
            assert not kw.get("depthwise") and kw["c"] % 16 == 0, (i, kw)
        total += ps.macs(kw)
    assert total <= 5e9, total   # a few seconds of the CPU oracle per family


def test_the_child_environments_are_the_hand_lists():
    import residual_cases as rc
    assert ps.child_envs() is rc.CHILD_ENVS
    assert sorted({c for _, c in ps.FLAVOURS if c is not None}) == list(range(len(rc.CHILD_ENVS)))


@pytest.mark.parametrize("family", CONV)
def test_conv_post_op_strata(family):
    n = ps.FAMILIES[family]["n"]
    rows = [(i, ps.strata(family, i), ps.draw(family, i)) for i in range(n)]
    # the cross: 14 flavours x 4 codes, every cell at least twice, as flavour_of reads the draws under the cases' environments
    cells = collections.Counter(ps.flavour_of(kw, ps.case_env(family, i), ps.POST[family]) for i, s, kw in rows)
    want = {"%s/epi%d+%s" % (fl, code, ps.POST[family]) for fl, _ in ps.FLAVOURS for code in ps.EPI}
    assert len(ps.FLAVOURS) == 14 and len(want) == 56 and set(cells) == want and min(cells.values()) >= 2, cells
    for i, s, kw in rows:
        assert ps.flavour_of(kw, ps.case_env(family, i), ps.POST[family]) == cell_of(family, i)
        c = conv_classes(family, i, kw)
        assert {k: s[k] for k in c} == c, (i, s, c)
        assert kw["exact"] == (s["code"] >= 3) and (kw["act"] != 0) == (s["code"] in (1, 4))
    # in the test process: the six flavours of the default environment; the others in the child of their environment
    inproc = {s["flavour"] for i, s, kw in rows if s["child"] is None}
    assert inproc == {"wave/ks1", "wave/ks4", "tile/128x128/pipe8/utap", "tile/128x128/pipe4/anytap", "tile/256x64/pipe0/utap",
                      "tile/256x64/pipe0/anytap"}
    assert all(set(ps.case_env(family, i)) == {ps.FORM_SWITCH[ps.POST[family]]} for i, s, kw in rows if s["child"] is None)
    per_flavour = collections.defaultdict(lambda: collections.defaultdict(set))
    for i, s, kw in rows:
        for key in ("window", "pixels", "n", "by_call", "path", "two", "per_channel", "tiles2"):
            per_flavour[s["flavour"]][key].add(s[key])
        per_flavour[s["flavour"]]["act"].add(kw["act"])
        per_flavour[s["flavour"]]["path_two"].add((ps.store_path(kw["co"]), int(kw["co"] > ps.tile_of(s["flavour"])[1])))
    for fl, seen in per_flavour.items():
        # windows: all a flavour can take (uniform-tap addressing: at most 32 taps)
        assert seen["window"] == set(ps.windows_of(fl)), (fl, seen["window"])
        assert len(ps.windows_of(fl)) == (7 if fl.endswith("/utap") else 8)
        assert seen["pixels"] == set(ps.PIXELS) and seen["n"] == {1, 2, 3} and seen["by_call"] == {True, False}, (fl, seen)
        assert seen["path"] == {"staged", "dwords", "elements"} and seen["per_channel"] == {True, False} and seen["tiles2"] == {True, False}
        assert seen["two"] == ({0} if fl.startswith("tile/256x64/pipe0") else {0, 1}), (fl, seen["two"])
        # each store path once with one channel tile and once with a ragged second one, per flavour
        assert seen["path_two"] == {(p, t) for p in ("staged", "dwords", "elements") for t in seen["two"]}, (fl, seen["path_two"])
        assert seen["act"] == {0, 1, 2}   # the convolution's own folded relu and relu6
    # no stratum is a function of another: every pair of values meets, but for the two exceptions of the module docstring
    # (and the 7x7, which six flavours see once each, meets three of the four codes)
    keys = ("code", "window", "pixels", "n", "by_call", "path", "two", "per_channel")
    for a in range(len(keys)):
        for b in range(a + 1, len(keys)):
            ka, kb = keys[a], keys[b]
            met = {(s[ka], s[kb]) for i, s, kw in rows}
            full = {(x, y) for x in {s[ka] for i, s, kw in rows} for y in {s[kb] for i, s, kw in rows}}
            allowed = {("pixels", "n"): {("one", 2), ("last", 2)}, ("n", "by_call"): {(1, True)}}.get((ka, kb), set())
            missing = full - met - allowed
            if (ka, kb) == ("code", "window"):
                assert len(missing) <= 1 and all(w == "7x7" for _, w in missing), missing
            elif "window" in (ka, kb):
                assert len(missing) <= 3, (ka, kb, missing)
            else:
                assert not missing, (ka, kb, missing)
    # windows: geometry as named
    for i, s, kw in rows:
        if s["window"] == "1x7":
            along = (kw["pad"][1], kw["pad"][3]) if kw["k"] == (1, 7) else (kw["pad"][0], kw["pad"][2])
            assert along[0] != along[1], (i, kw)
        if s["window"] == "3x3same":
            assert fs.geometry(kw)["ho"] == kw["h"] and fs.geometry(kw)["wo"] == kw["w"]
        utap = kw["c"] % 64 == 0 and kw["k"][0] * kw["k"][1] <= 32
        assert utap == s["flavour"].endswith("/utap") or s["flavour"].startswith("wave"), (i, kw)
        if s["flavour"].endswith("/anytap"):
            assert kw["c"] in (16, 32, 48, 80) or (kw["k"] == (7, 7) and kw["c"] == 64), (i, kw)
    assert sum(1 for i, s, kw in rows if kw["k"] == (7, 7) and kw["c"] == 64) == 4   # 49 taps: no uniform tap at C % 64 == 0 (each such tile flavour once)
    assert {kw["k"] for i, s, kw in rows} >= {(1, 7), (7, 1)}
    # batch: in a third of the cases the plan is made at batch 1 and the call passes the batch
    assert n // 3 <= sum(1 for i, s, kw in rows if s["by_call"]) and all(kw["n"] > 1 for i, s, kw in rows if s["by_call"])
    # pixels: two or more pixel tiles in at least half of the cases, a batch boundary inside a tile in at least a quarter
    tbm = lambda s: ps.tile_of(s["flavour"])[0]
    assert sum(1 for i, s, kw in rows if fs.geometry(kw)["M"] > tbm(s)) >= n // 2
    assert sum(1 for i, s, kw in rows if kw["n"] > 1 and (fs.geometry(kw)["ho"] * fs.geometry(kw)["wo"]) % tbm(s)) >= n // 4
    assert sum(1 for i, s, kw in rows if fs.geometry(kw)["M"] % tbm(s) == 0) >= 1   # and complete tiles somewhere
    assert sum(1 for i, s, kw in rows if kw["per_channel"]) == n // 2
    # wave/ks1 on K rows of split-K's length (5x5 and 7x7 at C = 16): more than 256 tiles, with one channel tile and with two
    long_k = [kw for i, s, kw in rows if s["flavour"] == "wave/ks1" and s["window"] in ("5x5", "7x7")]
    assert {kw["k"] for kw in long_k} == {(5, 5), (7, 7)} and all(kw["c"] * kw["k"][0] * kw["k"][1] >= 256 for kw in long_k)
    assert all(ps.ceil_div(fs.geometry(kw)["M"], 32) * ps.ceil_div(kw["co"], 32) > 256 for kw in long_k)
    # split-K: its condition three ways; ragged channel tile + element stores + ragged pixel tile together at least twice
    ks4 = [(s, kw) for i, s, kw in rows if s["flavour"] == "wave/ks4"]
    assert any(kw["k"] == (1, 1) and kw["c"] >= 256 for s, kw in ks4) and any(kw["k"] == (3, 3) and kw["c"] == 32 for s, kw in ks4)
    assert any(kw["k"] == (5, 5) and kw["c"] == 16 for s, kw in ks4)
    assert sum(1 for s, kw in ks4 if kw["co"] > 32 and kw["co"] % 32 and kw["co"] % 4 and fs.geometry(kw)["M"] % 32) >= 2
    assert all(fs.geometry(kw)["M"] % 32 for s, kw in ks4)
    if family == "conv_add":
        recs = [ps.residual_strata(i) for i in range(n)]
        per = collections.defaultdict(lambda: collections.defaultdict(set))
        for (i, s, kw), r in zip(rows, recs):
            per[s["flavour"]]["conv_first"].add(r["conv_first"])
            per[s["flavour"]]["act"].add(r["act"])
        assert all(v["conv_first"] == {0, 1} and v["act"] == {0, 1, 2} for v in per.values()), per
        for key in ("skip_zp", "sum_zp"):
            assert {r[key] for r in recs} == {-128, 0, 127, None}, key
        assert {r["out_zp"] for r in recs if r["act"]} == {-128, 0, 127, None}
        assert {r["pow2"] for r in recs} == {True, False}
        assert sum(r["no_fma_div"] for r in recs) == n // 16 and sum(r["skip_fill"] is not None for r in recs) == n // 16
        assert {r["skip_fill"] for r in recs} == {None, -128, 127}
    else:
        assert {ps.TABLE_CYCLE[i % 8] for i in range(n)} == set(ps.TABLE_CYCLE)
        import act_fuse_cases as ac
        assert set(ps.TABLE_CYCLE) | {"permutation"} == set(ac.TABLES)


def test_dw_lut_strata():
    F = "dw_lut"
    assert [ps.strata(F, i)["kernel"] for i in range(88)] == ["mfma"] * 40 + ["dot4"] * 24 + ["nhwc"] * 24
    assert all(ps.child_index(F, i) == (0 if i < 40 else None) for i in range(88))
    for kernel, lo in (("dot4", 40), ("nhwc", 64)):
        rows = [(ps.strata(F, i), ps.draw(F, i)) for i in range(lo, lo + 24)]
        lanes = lambda kw: fs.geometry(kw)["wo"] * kw["c"] // 4
        cls = lambda v: "lt64" if v < 64 else ("64to256" if v <= 256 else "gt256")
        for s, kw in rows:
            assert cls(lanes(kw)) == s["lanes"] and kw["stride"] == s["stride"] and kw["dilation"] == (s["dilation"],) * 2
            assert (kw["pad"][0] != kw["pad"][2] or kw["pad"][1] != kw["pad"][3]) == s["asym"] and kw["n"] == s["n"] and kw["k"] == s["k"]
            assert fs.epi_code(kw) == s["code"]
        keys = ("lanes", "stride", "dilation", "asym", "by_call", "code") + (("k",) if kernel == "nhwc" else ())
        for a in range(len(keys)):
            assert len({s[keys[a]] for s, kw in rows}) == {"lanes": 3, "stride": 4, "dilation": 2, "asym": 2, "by_call": 2, "code": 4, "k": 6}[keys[a]]
            for b in range(len(keys)):   # no stratum is a function of another: each value meets two or more of any other stratum
                for va in {s[keys[a]] for s, kw in rows} if a != b else ():
                    assert len({s[keys[b]] for s, kw in rows if s[keys[a]] == va}) >= 2, (keys[a], va, keys[b])
        assert sum(1 for s, kw in rows if s["by_call"]) == 8 and {kw["n"] for s, kw in rows} == {1, 2, 3}
        assert all(kw["k"] == (3, 3) for s, kw in rows) if kernel == "dot4" else {kw["k"] for s, kw in rows} == set(ps.NHWC_WINDOWS)


# ------------------------------------------------------------------------------------------------ CPU: the oracle can tell results apart
def test_the_oracle_chain_of_conv_add_spreads_or_is_flat_by_record():
    import residual_cases as rc
    flat = 0
    for i in range(ps.FAMILIES["conv_add"]["n"]):
        case = ps.add_case(i)
        assert rc.fma_div_of(case) == int(not ps.residual_strata(i)["no_fma_div"])
        if rc.flat_by_record(case):
            flat += 1
        else:
            assert len(np.unique(rc.oracle_chain(case)["out"])) > 8, ps.describe("conv_add", i)
    assert flat <= ps.FAMILIES["conv_add"]["n"] // 8, flat


@pytest.mark.parametrize("family", ["conv_lut", "dw_lut"])
def test_the_convolution_outputs_exercise_the_permutation_table(family, standalone):
    import act_fuse_cases as ac
    import dw_act_cases as dc
    fe, hip, opt = standalone
    for i in range(ps.FAMILIES[family]["n"]):
        both = ps.lut_cases(i) if family == "conv_lut" else ps.dw_cases(i)
        conv = ac.oracle_chain(both[0])["conv"] if family == "conv_lut" else dc.oracle_chain(dict(both[0], table="identity"))
        assert len(np.unique(conv)) > 32, ps.describe(family, i)
        for cs in both:   # the backend's table builders (host code) against the reference's arithmetic, for this output record
            assert np.array_equal(ac.by_q(ac.device_table(opt, cs)), ac.oracle_table(cs)), (cs["name"], ps.describe(family, i))
        ps.forget(i, family)


def test_a_failing_case_is_reported_with_its_keywords_and_seed(monkeypatch):
    import act_fuse_cases as ac
    import residual_cases as rc

    def wrong_flavour(hip, *args):
        hip.flavour_ran = "tile/128x128/pipe4/utap/epi0+add"

    def wrong_bytes(hip, *args):
        hip.flavour_ran = ps.flavour_of(ps.draw(family, i), ps.case_env(family, i), ps.POST[family])
        raise AssertionError("fused differs from the oracle chain on 3 of 100 outputs (max 1)")

    def refused(hip, *args):   # what cases.pkg.check raises on a status other than OK
        hip.flavour_ran = ps.flavour_of(ps.draw(family, i), ps.case_env(family, i), ps.POST[family])
        raise RuntimeError("conv_add_forward failed (-3): not supported")
    for family, i, module in (("conv_add", 17, rc), ("conv_lut", 60, ac)):
        for stub, text in ((wrong_flavour, "flavour_of says"), (wrong_bytes, "differs from the oracle chain"), (refused, "failed (-3)")):
            monkeypatch.setattr(module, "check_case", stub)
            with pytest.raises(AssertionError) as e:
                ps.run_case(None, None, None, family, i)
            assert repr(ps.draw(family, i)) in str(e.value) and str(ps.case_seed(family, i)) in str(e.value) and text in str(e.value)
            assert str(ps.BASE_SEED) in str(e.value)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu(standalone):
    from cases import HipDevice, pkg
    fe, hip, opt = standalone
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    return hip, opt, HipDevice(hip)


@pytest.mark.gpu
@pytest.mark.parametrize("family,indices", ps.chunks(), ids=["%s-%d" % (f, idx[0]) for f, idx in ps.chunks()])
def test_post_op_chunk_in_the_test_process(gpu, family, indices, monkeypatch):
    hip, opt, dev = gpu
    for name in [k for k in os.environ if k.startswith("SHL_MI355X_")]:
        monkeypatch.delenv(name)
    monkeypatch.setenv("SHL_MI355X_TUNE", "0")   # read per plan: no timing runs at conv_plan_create
    for i in indices:
        for k, v in ps.case_env(family, i).items():
            monkeypatch.setenv(k, v)
        ps.run_case(hip, opt, dev, family, i)


CHILDREN = [(f, k) for k in range(len(ps.child_envs())) for f in CONV] + [("dw_lut", 0)]
A_CHILD_DIED = []


def child_env_of(family, k):
    return dict(ps.DW_CHILD_ENV) if family == "dw_lut" else dict(ps.child_envs()[k])


@pytest.mark.gpu
@pytest.mark.parametrize("family,k", CHILDREN,
                         ids=["%s-%s" % (f, "-".join("%s=%s" % (n[11:], v) for n, v in sorted(child_env_of(f, k).items()))) for f, k in CHILDREN])
def test_post_op_cases_of_an_environment_in_a_child_process(family, k):
    """the flavour switches of the tile kernel and SHL_MI355X_DWMFMA are read once per process"""
    assert not A_CHILD_DIED, "not started: an earlier child ended by a signal or at its time limit: %r" % A_CHILD_DIED
    env = {n: v for n, v in os.environ.items() if not n.startswith("SHL_MI355X_")}
    env.update(child_env_of(family, k))
    count = sum(1 for i in range(ps.FAMILIES[family]["n"]) if ps.child_index(family, i) == k)
    assert count >= 8
    try:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "post_op_sweeps.py"), family], capture_output=True, text=True,
                             timeout=300, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        A_CHILD_DIED.append((family, k, "time limit"))
        raise AssertionError("the child ran into its time limit: %r" % ((e.stdout or b"")[-2000:],))
    if res.returncode < 0:
        A_CHILD_DIED.append((family, k, "signal %d" % -res.returncode))
    assert res.returncode == 0 and "child ok %d" % count in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])

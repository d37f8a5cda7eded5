"""Seeded sweeps (tests/tail_sweeps.py) over the kernels behind the convolutions -- pool_softmax.hip (global_avgpool2d's two
kernel forms, softmax), elementwise.hip (relu / relu6 int8 and binary16, add), conv_gemv.hip:pool_gemv_i8_kernel -- and the
softmax scan on crafted sums (tests/softmax_sum_cases.py).

CPU: the draws are reproducible, fill every stratum and stay inside the form they name; the oracle equals the genuine
reference on the binary16 special values (tests/golden/tail_sweep_specials.npz, and the live library where it is built); the
crafted sums hold the ties and binade exits they claim, at every place of a round of the scan.
GPU: every case through csinn_* in layer mode on device tensors (one round of the strata host-staged as well) and again
through the C-ABI into a buffer with 4 KiB of 0x5A on either side: zero bytes (binary16: words outside the NaN places, and
the same NaN places) differ from the oracle, the two runs agree, the bands are untouched.  The cases beyond the grid caps of
elementwise.hip run through the C-ABI only.  pool + classifier in one launch against the two launches and the oracle chain.
Both forms of the running sum against the plain numpy loop, bit for bit."""
import collections
import ctypes as C
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import cases
import softmax_sum_cases as sc
import tail
import tail_sweeps as ts
from cases import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
SISO = ("gap", "softmax", "relu", "add")
GOLD = np.load(os.path.join(HERE, "golden", "tail_sweep_specials.npz"))
GOLD_SEED = int(GOLD["seed"])


def draws(family):
    return [ts.draw(family, i) for i in range(ts.FAMILIES[family]["n"])]


def count(family, key):
    return collections.Counter(key(d) for d in draws(family))


# ------------------------------------------------------------------------------------------------ CPU: the draws
def test_draws_are_reproducible_and_the_seed_moves_only_the_free_parameters():
    assert [ts.FAMILIES[f]["n"] for f in ts.FAMILIES] == [56, 56, 32, 32, 32]
    moved = 0
    for f in ts.FAMILIES:
        for i in range(ts.FAMILIES[f]["n"]):
            a, b = ts.draw(f, i), ts.draw(f, i, seed=ts.BASE_SEED + 1)
            assert a == ts.draw(f, i), (f, i)
            s = ts.STRATA[f](i)
            assert all(a[k] == v and b[k] == v for k, v in s.items()), (f, i)   # the strata hold for every seed
            moved += a != b
    assert moved > 100
    one, two = ts.build("softmax", 5), ts.build("softmax", 5)
    assert np.array_equal(one["x"].view(np.uint16), two["x"].view(np.uint16))


def test_gap_strata_and_forms():
    ds = draws("gap")
    combos = count("gap", lambda d: (d["dtype"], d["layout"]))
    assert len(combos) == 4 and min(combos.values()) == 14
    pxc = lambda p: "1" if p == 1 else "2to63" if p < 64 else "64" if p == 64 else "65" if p == 65 else "66to200"
    for d in ds:
        assert d["h"] * d["w"] == d["px"] <= 200 and pxc(d["px"]) == d["px_class"] and 1 <= d["n"] <= 5
        # shl_mi355x_global_avgpool2d's choice, restated from the drawn numbers alone
        fast = d["dtype"] == "int8" and d["layout"] == "NHWC" and d["c"] % 4 == 0 and d["px"] <= 64
        assert d["fast"] == fast and ts._nc_ok(d["nc_rule"], d["n"] * d["c"])
        assert fast == d["nc_rule"].startswith("fast") or d["nc_rule"] in ("lt64", "free"), d
    per_combo = collections.defaultdict(collections.Counter)
    for d in ds:
        per_combo[(d["dtype"], d["layout"])][d["px_class"]] += 1
    assert all(len(v) == 5 and min(v.values()) >= 2 for v in per_combo.values()), per_combo
    nhwc = [d for d in ds if d["dtype"] == "int8" and d["layout"] == "NHWC"]
    for px in (1, 64, 65):
        assert sum(1 for d in nhwc if d["px"] == px and d["c"] % 4 == 0) >= 2, px
    # C % 4 != 0 with at most 64 pixels: the general kernel, and both kernels on either side of 64 pixels
    assert sum(1 for d in nhwc if d["c"] % 4 and d["px"] <= 64 and not d["fast"]) >= 2
    assert sum(1 for d in nhwc if d["fast"]) >= 8 and sum(1 for d in nhwc if not d["fast"] and d["c"] % 4 == 0) >= 3
    # n * C against the block: 64 lanes in the fast form (0, 4, 60: the module's docstring), 256 in the general one
    fast_res = collections.Counter(d["n"] * d["c"] % 64 for d in nhwc if d["fast"] and d["n"] * d["c"] > 64)
    assert min(fast_res[0], fast_res[4], fast_res[60]) >= 2, fast_res
    assert sum(1 for d in nhwc if d["fast"] and d["n"] * d["c"] < 64) >= 2
    fast_px = collections.Counter(d["px_class"] for d in nhwc if d["fast"])
    assert min(fast_px["1"], fast_px["2to63"], fast_px["64"]) >= 2, fast_px
    gen = [d for d in ds if not d["fast"]]
    gen_res = collections.Counter(d["n"] * d["c"] % 256 for d in gen if d["n"] * d["c"] > 256)
    assert min(gen_res[0], gen_res[1], gen_res[255]) >= 2 and sum(1 for d in gen if d["n"] * d["c"] < 64) >= 2, gen_res
    assert sum(1 for d in ds if d["h"] != d["w"]) > len(ds) // 2
    assert sum(1 for d in ds if d["h"] == 1 and d["w"] > 1) >= 2 and sum(1 for d in ds if d["w"] == 1 and d["h"] > 1) >= 2
    assert set(d["n"] for d in ds) == {1, 2, 3, 4, 5}
    i8 = [d for d in ds if d["dtype"] == "int8"]
    assert len(set(d["pow2"] for d in i8)) == 2
    assert {-128, 127} <= set(d["in_q"][1] for d in i8) and {-128, 127} <= set(d["out_q"][1] for d in i8)
    sat = [i for i in range(56) if ts.draw("gap", i)["saturate"]]
    assert len(sat) >= 4
    for i in sat:   # both ends saturate
        out = tail.siso_oracle(ts.build("gap", i))
        assert out.min() == -128 and out.max() == 127, i
    spec = collections.Counter(d["special"] for d in ds if d["special"])
    assert spec == {"big": 2, "inf": 2, "inf_pair": 2, "nan": 2}
    for i in range(56):
        d = ts.draw("gap", i)
        if d["special"]:
            case = ts.build("gap", i)
            x, out = case["x"].astype(np.float32), tail.siso_oracle(case).astype(np.float32)
            if d["special"] == "big":
                axes = (1, 2) if d["layout"] == "NHWC" else (2, 3)
                assert np.abs(x.sum(axis=axes)).max() > 65504 or d["px"] == 1
                assert np.isfinite(out).all() and np.abs(out).max() == 65504
            elif d["special"] == "inf":
                assert (out == 65504).sum() == 1 and not np.isnan(out).any()   # (the reference's conversion saturates +inf)
            else:
                assert np.isnan(out).sum() == 1 and not np.isinf(out).any()


def test_softmax_strata_and_launch_forms():
    ds = draws("softmax")
    cc = lambda c: [k for k, (lo, hi) in ts.SM_COUNT.items() if lo <= c <= hi][0]
    ic = lambda c: [k for k, (lo, hi) in ts.SM_INNER.items() if lo <= c <= hi][0]
    for d in ds:
        assert cc(d["count"]) == d["count_class"] and ic(d["inner"]) == d["inner_class"] and d["rows"] == d["outer"] * d["inner"]
        assert 1 <= d["count"] <= ts.SM_MAX_CNT and 1 <= d["rows"] <= 310
        # shl_mi355x_softmax: the dynamic-LDS opt-in, restated
        assert d["lds_opt_in"] == (9 * d["count"] + 5376 > 48 * 1024) == (d["count"] >= ts.SM_LDS_OPT_IN)
        assert ts.softmax_lds_bytes(d["count"]) <= 96 * 1024
    combos = count("softmax", lambda d: (d["dtype"], d["inner_class"], d["count_class"]))
    assert len(combos) == 48, len(combos)
    assert min(count("softmax", lambda d: (d["dtype"], d["count_class"])).values()) >= 2
    for dtype in ("int8", "f16"):
        mine = [d for d in ds if d["dtype"] == dtype]
        assert {4864, 4865, 8192} <= set(d["count"] for d in mine), dtype
        assert any(d["count"] == 8192 and d["inner"] > 1 for d in mine)
    assert min(d["rows"] for d in ds) == 1 and max(d["rows"] for d in ds) >= 200
    assert sum(d["outer"] * d["count"] * d["inner"] for d in ds) < 2e6
    i8 = [d for d in ds if d["dtype"] == "int8"]
    assert set(d["in_q"][0] for d in i8) == set(float(np.float32(s)) for s in ts.SM_IN_SCALES)
    assert min(collections.Counter(d["out_q"] for d in i8).values()) >= 4 and len(set(d["out_q"] for d in i8)) == 3
    kinds = collections.Counter(d["row_kind"] for d in ds if d["dtype"] == "f16")
    assert set(kinds) == set(ts.SM_F16_ROWS) and min(kinds.values()) >= 2, kinds


def test_softmax_special_rows_behave_as_the_issue_states():
    """the oracle on this CPU: a 0 for every -inf entry of an otherwise finite row; every other special row is NaN throughout;
    the rows next to a special row do not feel it"""
    seen = collections.Counter()
    for i in range(1, 56, 2):
        d = ts.draw("softmax", i)
        if d["row_kind"] not in ts.SM_SPECIAL_ROWS:
            continue
        case = ts.build("softmax", i)
        x3 = case["x"].reshape(d["outer"], d["count"], d["inner"]).astype(np.float32)
        o3 = tail.siso_oracle(case).reshape(x3.shape).astype(np.float32)
        for o in range(d["outer"]):
            for k in range(d["inner"]):
                xr, yr = x3[o, :, k], o3[o, :, k]
                marked = (o, k) in ((0, 0), (d["outer"] - 1, d["inner"] - 1))
                if not marked:
                    assert np.isfinite(xr).all() and np.isfinite(yr).all()
                elif d["row_kind"] == "some_ninf" and d["count"] > 1:
                    assert np.isneginf(xr).any() and np.all(yr[np.isneginf(xr)] == 0) and np.isfinite(yr).all() and yr.max() > 0
                    seen["zeros"] += 1
                elif d["row_kind"] != "some_ninf":
                    assert np.isnan(yr).all(), (i, d["row_kind"])
                    seen[d["row_kind"]] += 1
    assert seen["zeros"] >= 2 and all(seen[k] >= 2 for k in ts.SM_SPECIAL_ROWS[1:]), seen


def test_relu_strata_and_grids():
    ds = draws("relu")
    assert len(count("relu", lambda d: (d["dtype"], d["relu6"]))) == 4
    i8, f16 = [d for d in ds if d["dtype"] == "int8"], [d for d in ds if d["dtype"] == "f16"]
    c8, c16 = collections.Counter(d["count"] for d in i8), collections.Counter(d["count"] for d in f16)
    assert all(c8[c] >= 2 for c in ts.RELU_I8_COUNTS) and c8[ts.RELU_I8_BIG] == 1
    assert all(c16[c] >= 2 for c in (1, 255, 256, 257)) and c16[ts.ELT_F16_BIG] == 1
    for d in ds:
        # shl_mi355x_relu_i8 / shl_mi355x_relu_f16's grids, restated
        if d["dtype"] == "int8":
            blocks = min(max((d["count"] // 16 + 255) // 256, 1), 2048)
            second = d["count"] // 16 > blocks * 256
        else:
            blocks = min((d["count"] + 255) // 256, 4096)
            second = d["count"] > blocks * 256
        assert d["blocks"] == blocks and (d["passes"] > 1) == second == d["abi_only"]
    assert sum(1 for d in i8 if d["abi_only"]) == 1 and sum(1 for d in f16 if d["abi_only"]) == 1
    assert any(d["blocks"] > 1 and not d["abi_only"] for d in i8) and any(d["count"] < 16 for d in i8)
    # where the dequantised 6.0 lands in the output record
    where = collections.Counter()
    for d in i8:
        so, zo = d["out_q"]
        q6 = float(np.rint(np.float32(6.0) / np.float32(so))) + zo
        where["inside" if q6 < 127 else "edge" if q6 == 127 else "beyond"] += 1
        if d["out"][0] == "tie":   # 6 / scale is rint's tie and rounds away from what one float below 6 gives
            assert np.float32(6.0) / np.float32(so) == 1.5 and np.rint(np.float32(5.9999995) / np.float32(so)) == 1.0
    assert min(where["inside"], where["edge"], where["beyond"]) >= 4, where
    ragged6 = [d for d in i8 if d["relu6"] and d["out"][0] == "tie" and d["count"] % 16 and d["in_zp_class"] == "mid"]
    assert len(ragged6) >= 2   # relu6's clamp decides the ragged tail's last byte
    assert {-128, 127} <= set(d["in_q"][1] for d in i8)
    out_zps = collections.Counter(d["out_q"][1] for d in i8)
    assert min(out_zps[-128], out_zps[127]) >= 2, out_zps


def test_add_strata_and_planted_pairs():
    ds = draws("add")
    for dtype in ("int8", "f16"):
        cnt = collections.Counter(d["count"] for d in ds if d["dtype"] == dtype)
        assert all(cnt[c] >= 2 for c in ts.ADD_COUNTS) and cnt[ts.ELT_F16_BIG] == 1, cnt
    for d in ds:   # shl_mi355x_add's grid, restated
        blocks = min((d["count"] + 255) // 256, 4096)
        assert d["blocks"] == blocks and d["abi_only"] == (d["count"] > blocks * 256)
    i8 = [d for d in ds if d["dtype"] == "int8"]
    assert len(set((d["pow2"], d["saturate"]) for d in i8)) == 4
    assert all(len({d["in_q"], d["in1_q"], d["out_q"]}) == 3 for d in i8 if not d["pow2"])
    for i in range(0, 32, 2):
        if ts.draw("add", i)["saturate"] and ts.draw("add", i)["count"] > 255:
            out = tail.siso_oracle(ts.build("add", i))
            assert out.min() == -128 and out.max() == 127, i
    # binary16: every pair of the planted values, and what the reference makes of the named ones
    f = lambda w: np.array([w], dtype=np.uint16).view(np.float16)[0]
    assert len(ts.ADD_PAIRS) == len(ts.ADD_PLANTS) ** 2
    case = ts.build("add", 3)   # 255 elements
    out = tail.siso_oracle(case).view(np.uint16).ravel()
    xs, ys = case["x"].view(np.uint16).ravel(), case["y"].view(np.uint16).ravel()
    got = {(int(a), int(b)): int(o) for a, b, o in zip(xs[:144], ys[:144], out[:144])}
    assert set(got) == set(ts.ADD_PAIRS)
    assert got[(0x7BFF, 0x7BFF)] == 0x7BFF and got[(0xFC00, 0xFC00)] == 0xFBFF and (got[(0x7C00, 0xFC00)] & 0x7FFF) > 0x7C00
    assert got[(0x0001, 0x0001)] == 0x0002
    # (the ties 1 + 2^-11 and (1 + 2^-10) + 2^-11 go the way the reference's own conversion sends them: the fixture holds it)
    assert got[(0x3C00, 0x1000)] in (0x3C00, 0x3C01) and got[(0x3C01, 0x1000)] in (0x3C01, 0x3C02)
    assert f(0x1000) == 2.0 ** -11 and f(0x4C00) == 16 and f(0x0001) == 2.0 ** -24
    big = ts.build("add", 31)
    assert ts.specials(big).max() == big["x"].size - 1 and ts.specials(big).size == 288


def test_pool_gemv_strata_and_admissibility():
    ds = draws("pool_gemv")
    for key, values in (("px", ts.PG_PX), ("c", ts.PG_C), ("co", ts.PG_CO)):
        cnt = collections.Counter(d[key] for d in ds)
        assert set(cnt) == set(values) and min(cnt.values()) >= 2, (key, cnt)
    for d in ds:
        assert d["h"] * d["w"] == d["px"] and 1 <= d["n"] <= 8
        # launch_pool_gemv and pool_gemv_pick, restated
        assert d["instance"] == (16 if d["px"] <= 16 else 64)
        assert d["px"] <= 64 and d["c"] % 16 == 0 and ts.pool_gemv_admissible(d["n"], d["px"], d["c"])
    assert len(set((d["instance"], d["c"] > 1024) for d in ds)) == 4
    images = collections.Counter(d["n"] for d in ds)
    assert set(images) == set(range(1, 9)) and min(images.values()) >= 2, images
    assert len(set((d["act"], d["exact"]) for d in ds)) == 6
    assert len(set(d["per_channel"] for d in ds)) == 2


# ------------------------------------------------------------------------------------------------ CPU: oracle vs the reference
def operands_crc(case):
    crc = zlib.crc32(np.ascontiguousarray(case["x"]).tobytes())
    return zlib.crc32(np.ascontiguousarray(case["y"]).tobytes(), crc) if "y" in case else crc


def test_oracle_equals_the_reference_fixture_on_every_binary16_special_case():
    listed = ts.special_cases()
    assert collections.Counter(f for f, _ in listed) == {"gap": 8, "softmax": 10, "add": 16}
    assert sorted(k.split("/")[0] for k in GOLD.files if k.endswith("/out")) == sorted("%s_%02d" % fi for fi in listed)
    for fam, i in listed:
        case = ts.build(fam, i, seed=GOLD_SEED)
        name = case["name"]
        assert int(GOLD[name + "/x_crc"]) == operands_crc(case), name + ": the fixture's operands drifted"
        words = ts.canonical_f16(tail.siso_oracle(case))
        want = GOLD[name + "/out"]
        at = ts.specials(case)
        bad = np.flatnonzero(words[at] != want)
        assert bad.size == 0, "%s: %d planted words differ, first at %d: oracle %#06x reference %#06x" % (
            name, bad.size, int(at[bad[0]]), int(words[at][bad[0]]), int(want[bad[0]]))
        assert zlib.crc32(words.tobytes()) == int(GOLD[name + "/out_crc"]), name + ": differs outside the planted words"


LIVE = r"""
import sys
sys.path.insert(0, %r)
import numpy as np, cases, tail, tail_sweeps as ts
from cases import pkg
fe = cases.load_reference_frontend()
bad = []
for fam in ("gap", "softmax", "relu", "add"):
    for i in range(ts.FAMILIES[fam]["n"]):
        case = ts.build(fam, i)
        want = tail.siso_run(fe, pkg.API_REF, case)
        got = tail.siso_oracle(case)
        if case["dtype"] == "int8":
            ok = np.array_equal(got.view(np.uint8), want.view(np.uint8))
        else:
            ok = ts.f16_same(got, want) == (True, 0)
        if not ok:
            bad.append(case["name"])
print("LIVE_OK" if not bad else "LIVE_FAIL " + " ".join(bad))
"""


@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_oracle_against_the_live_reference_on_every_sweep_case():
    res = subprocess.run([sys.executable, "-c", LIVE % HERE], capture_output=True, text=True, timeout=600)
    assert "LIVE_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ CPU: the crafted sums
@functools.lru_cache(maxsize=None)
def sum_rows():
    return [(name, terms, sc.reference(terms)) for name, terms in sc.rows()]


SUM_GROUPS = ("tie_", "ties_", "exit_", "1e300_", "inf_", "nan_", "subnormal_", "exp_")


def test_crafted_sums_hold_ties_and_exits_at_every_place_of_a_round():
    rows = sum_rows()
    assert all(name.startswith(SUM_GROUPS) for name, _, _ in rows) and len(set(n for n, _, _ in rows)) == len(rows)
    ties, exits = [], []
    for name, terms, _ in rows:
        assert 1 <= terms.size <= 8192 and not (terms < 0).any()   # non-negative, +inf or NaN: what softmax produces
        for s in sc.classify(terms):
            (ties if s["tie"] else exits).append(s)
    assert len(ties) >= 1000 and len(exits) >= 100, (len(ties), len(exits))
    assert sum(1 for s in ties if s["up"]) >= 100 and sum(1 for s in ties if not s["up"]) >= 100
    for what, steps in (("ties", ties), ("exits", exits)):
        off = [s["offset"] for s in steps]
        assert {o % 4 for o in off} == {0, 1, 2, 3}, what
        assert any(o // 4 == 0 for o in off) and any(o // 4 == 63 for o in off), what
    # the planted tie of a tie row sits where its name says
    for name, terms, _ in rows:
        if name.startswith("tie_") and int(name.rsplit("pos", 1)[1]) < 256:
            pos = int(name.rsplit("pos", 1)[1])
            assert any(s["tie"] and s["index"] == pos + 1 and s["offset"] == pos for s in sc.classify(terms)), name
    special = [t for n, t, _ in rows if n.startswith(("1e300_", "inf_", "nan_"))]
    assert len(special) == 3 * len(sc.EXIT_POS) and all(not np.isfinite(sc.reference(t)) for t in special)
    assert sorted(set(t.size for n, t, _ in rows if n.startswith("exp_"))) == list(sc.EXP_LENGTHS)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt


BAND = 4096


def abi_run(hip, dev, case):
    """the op through the C-ABI into the middle of a buffer filled with 0x5A -> (output, the two bands are untouched)"""
    x = np.ascontiguousarray(case["x"])
    shape = tail.out_shape_of(case)
    nbytes = int(np.prod(shape)) * x.itemsize
    d_in, d_buf = dev.alloc(x.nbytes), dev.alloc(nbytes + 2 * BAND)
    dev.upload(d_in, x)
    dev.upload(d_buf, np.full(nbytes + 2 * BAND, 0x5A, dtype=np.uint8))
    d_out = d_buf + BAND
    dt = pkg.SHL_I8 if case["dtype"] == "int8" else pkg.SHL_F16
    (si, zi), (so, zo) = case["in_q"], case["out_q"]
    kind, d_y = case["kind"], None
    if kind == "pool":
        nhwc = case["layout"] == "NHWC"
        n, h, w, c = x.shape if nhwc else (x.shape[0], x.shape[2], x.shape[3], x.shape[1])
        rc = hip.shl_mi355x_global_avgpool2d(d_in, d_out, dt, pkg.SHL_NHWC if nhwc else pkg.SHL_NCHW, n, c, h * w, si, zi, so, zo, None)
    elif kind == "softmax":
        ax = case["axis"]
        outer, inner = int(np.prod(x.shape[:ax], dtype=np.int64)), int(np.prod(x.shape[ax + 1:], dtype=np.int64))
        rc = hip.shl_mi355x_softmax(d_in, d_out, dt, outer, x.shape[ax], inner, si, zi, so, zo, None)
    elif kind == "add":
        y = np.ascontiguousarray(case["y"])
        d_y = dev.alloc(y.nbytes)
        dev.upload(d_y, y)
        rc = hip.shl_mi355x_add(d_in, d_y, d_out, x.size, dt, si, zi, case["in1_q"][0], case["in1_q"][1], so, zo, None)
    elif case["dtype"] == "int8":
        rc = hip.shl_mi355x_relu_i8(d_in, d_out, x.size, si, zi, so, zo, int(kind == "relu6"), None)
    else:
        rc = hip.shl_mi355x_relu_f16(d_in, d_out, x.size, int(kind == "relu6"), None)
    pkg.check(rc, hip, case["name"])
    raw = dev.download(d_buf, (nbytes + 2 * BAND,), np.uint8)
    for p in (d_in, d_buf, d_y):
        if p is not None:
            dev.free(p)
    clean = bool(np.all(raw[:BAND] == 0x5A) and np.all(raw[BAND + nbytes:] == 0x5A))
    return raw[BAND:BAND + nbytes].view(x.dtype).reshape(shape), clean


def differing(got, want, dtype):
    """number of differing bytes (int8) / words outside the NaN places (binary16; differing NaN places count as well)"""
    if dtype == "int8":
        return int((np.asarray(got).view(np.uint8) != np.asarray(want).view(np.uint8)).sum())
    same_nan, words = ts.f16_same(got, want)
    return words + (0 if same_nan else 1)


CHUNKS = [(f, c) for f in SISO for c in range(0, ts.FAMILIES[f]["n"], ts.CHUNK)]


@pytest.mark.gpu
@pytest.mark.parametrize("family,first", CHUNKS, ids=["%s_%02d" % fc for fc in CHUNKS])
def test_sweep_chunk_equals_the_oracle_through_csinn_and_through_the_c_abi(gpu, family, first):
    fe, hip, _ = gpu
    dev = cases.HipDevice(hip)
    bad = []
    for i in range(first, min(first + ts.CHUNK, ts.FAMILIES[family]["n"])):
        case = ts.build(family, i)
        want = tail.siso_oracle(case)
        abi, clean = abi_run(hip, dev, case)
        runs = [("c-abi", abi)]
        if not case["draw"].get("abi_only"):
            runs.append(("csinn, device tensors", tail.siso_run(fe, pkg.API_MI355X, case, device=dev)))
            if i < ts.FAMILIES[family]["host"]:
                runs.append(("csinn, host-staged", tail.siso_run(fe, pkg.API_MI355X, case)))
        for how, got in runs:
            n = differing(got, want, case["dtype"])
            if n:
                bad.append("%s via %s: %d of %d outputs differ from the oracle (%s)" % (case["name"], how, n, want.size, case["draw"]))
            if differing(got, abi, case["dtype"]):
                bad.append("%s: %s and the C-ABI run disagree" % (case["name"], how))
        if not clean:
            bad.append("%s: the C-ABI run wrote outside its output" % case["name"])
    assert not bad, "\n".join(bad)


PG_CHUNKS = list(range(0, ts.FAMILIES["pool_gemv"]["n"], ts.CHUNK))


@pytest.mark.gpu
@pytest.mark.parametrize("first", PG_CHUNKS)
def test_pool_gemv_chunk_equals_the_two_launches_and_the_oracle_chain(gpu, first, monkeypatch):
    import golden_util
    monkeypatch.setenv("SHL_MI355X_POOLGEMV", "1")   # (read per call)
    fe, hip, opt = gpu
    dev = cases.HipDevice(hip)
    for i in range(first, first + ts.CHUNK):
        case = ts.build("pool_gemv", i)
        n, px, c, co, x, in_q = case["n"], case["px"], case["c"], case["co"], case["x"], case["in_q"]
        conv = cases.make_case(ts.case_seed("pool_gemv", i), **case["conv_kw"])
        mid_q = (float(conv["in_scale"]), int(conv["in_zp"]))
        pooled = tail.siso_oracle(dict(kind="pool", x=x, dtype="int8", layout="NHWC", axis=1, in_q=in_q, out_q=mid_q))
        conv["input"] = np.ascontiguousarray(pooled.reshape(conv["in_shape"]))
        want = cases.oracle_run(conv, "ref")
        kept = []
        two = cases.csinn_run(fe, pkg.API_MI355X, conv, device=dev, keep_params=kept)   # the stand-alone GEMV on the oracle's pooled map
        plan = opt.shl_mi355x_registry_get(kept[0][0])
        what = "%s %s" % (case["name"], case["draw"])
        assert hip.shl_mi355x_pool_conv_fusable(plan, n, px) == 1, what
        nout = n * co
        d_x, d_mid, d_a, d_b = dev.alloc(x.nbytes), dev.alloc(n * c), dev.alloc(nout), dev.alloc(nout + 2 * BAND)
        dev.upload(d_x, x)
        dev.upload(d_b, np.full(nout + 2 * BAND, 0x5A, dtype=np.uint8))
        pkg.check(hip.shl_mi355x_global_avgpool2d(d_x, d_mid, pkg.SHL_I8, pkg.SHL_NHWC, n, c, px, in_q[0], in_q[1], mid_q[0], mid_q[1], None), hip, "avgpool")
        pkg.check(hip.shl_mi355x_conv_forward(plan, d_mid, d_a, n, None), hip, "conv_forward")
        # refusals first: too many pixels, a pooled record that is not the convolution's -- the output stays as it was
        assert hip.shl_mi355x_pool_conv_fusable(plan, n, 65) == 0
        assert hip.shl_mi355x_pool_conv_forward(plan, d_x, d_b + BAND, n, 65, in_q[0], in_q[1], mid_q[0], mid_q[1], None) == -3
        assert hip.shl_mi355x_pool_conv_forward(plan, d_x, d_b + BAND, n, px, in_q[0], in_q[1], mid_q[0], mid_q[1] + 1, None) == -3
        assert np.all(dev.download(d_b, (nout + 2 * BAND,), np.uint8) == 0x5A), what + ": a refused call wrote"
        pkg.check(hip.shl_mi355x_pool_conv_forward(plan, d_x, d_b + BAND, n, px, in_q[0], in_q[1], mid_q[0], mid_q[1], None), hip, "pool_conv_forward")
        sep = dev.download(d_a, conv["out_shape"], np.int8)
        raw = dev.download(d_b, (nout + 2 * BAND,), np.uint8)
        fused = raw[BAND:BAND + nout].view(np.int8).reshape(conv["out_shape"])
        assert np.all(raw[:BAND] == 0x5A) and np.all(raw[BAND + nout:] == 0x5A), what + ": wrote outside the output"
        assert np.array_equal(dev.download(d_mid, (n, c), np.int8).reshape(-1), pooled.reshape(-1)), what + ": stand-alone pooling vs the oracle"
        assert np.array_equal(fused, sep), "%s: fused launch vs the two launches: %d differ" % (what, int((fused != sep).sum()))
        if conv["exact"]:
            assert np.array_equal(fused, want) and np.array_equal(two, want), what
        else:
            golden_util.compare(conv, fused, want, what)
        for p in (d_x, d_mid, d_a, d_b):
            dev.free(p)
        opt.shl_mi355x_release_params(kept[0][0])


@pytest.mark.gpu
def test_pool_gemv_is_refused_for_channel_counts_off_the_16_byte_chunk(gpu, monkeypatch):
    monkeypatch.setenv("SHL_MI355X_POOLGEMV", "1")
    fe, hip, opt = gpu
    dev = cases.HipDevice(hip)
    for c, fusable in ((20, 0), (24, 0), (32, 1)):
        conv = cases.make_case(77, n=2, h=1, w=1, c=c, co=10, k=(1, 1), pad=(0, 0, 0, 0))
        kept = []
        cases.csinn_run(fe, pkg.API_MI355X, conv, device=dev, keep_params=kept)
        plan = opt.shl_mi355x_registry_get(kept[0][0])
        assert hip.shl_mi355x_pool_conv_fusable(plan, 2, 9) == fusable, c
        if not fusable:
            d_x, d_o = dev.alloc(2 * 9 * c), dev.alloc(64)
            dev.upload(d_o, np.full(64, 0x5A, dtype=np.uint8))
            assert hip.shl_mi355x_pool_conv_forward(plan, d_x, d_o, 2, 9, 0.05, 1, float(conv["in_scale"]), int(conv["in_zp"]), None) == -3
            assert np.all(dev.download(d_o, (64,), np.uint8) == 0x5A)
            dev.free(d_x)
            dev.free(d_o)
        opt.shl_mi355x_release_params(kept[0][0])


@pytest.mark.gpu
def test_softmax_refuses_an_axis_of_8193_and_leaves_the_output_alone(gpu):
    fe, hip, _ = gpu
    dev = cases.HipDevice(hip)
    for dt, size in ((pkg.SHL_I8, 1), (pkg.SHL_F16, 2)):
        n = (ts.SM_MAX_CNT + 1) * size
        d_in, d_out = dev.alloc(n), dev.alloc(n)
        dev.upload(d_in, np.zeros(n, dtype=np.uint8))
        dev.upload(d_out, np.full(n, 0x5A, dtype=np.uint8))
        assert hip.shl_mi355x_softmax(d_in, d_out, dt, 1, ts.SM_MAX_CNT + 1, 1, 0.1, 0, 1.0 / 256, -128, None) == -3   # SHL_MI355X_ENOTSUP
        assert b"8193" in hip.shl_mi355x_last_error()
        assert np.all(dev.download(d_out, (n,), np.uint8) == 0x5A)
        dev.free(d_in)
        dev.free(d_out)


FIRST_LAUNCH = r"""
import sys
sys.path.insert(0, %r)
import numpy as np, cases, tail, tail_sweeps as ts
from cases import pkg
fe = pkg.load_frontend("standalone")
hip, opt = pkg.load_backend(fe)
dev = cases.HipDevice(hip)
bad = 0
for i in (15, 14):   # binary16, then int8: 8192 classes, inner > 1
    case = ts.build("softmax", i)
    assert case["draw"]["count"] == 8192
    x = np.ascontiguousarray(case["x"])
    d_in, d_out = dev.alloc(x.nbytes), dev.alloc(x.nbytes)
    dev.upload(d_in, x)
    d = case["draw"]
    rc = hip.shl_mi355x_softmax(d_in, d_out, pkg.SHL_I8 if i %% 2 == 0 else pkg.SHL_F16, d["outer"], d["count"], d["inner"],
                                d["in_q"][0], d["in_q"][1], d["out_q"][0], d["out_q"][1], None)
    assert rc == 0, hip.shl_mi355x_last_error()
    got = dev.download(d_out, x.shape, x.dtype)
    want = tail.siso_oracle(case)
    ok = np.array_equal(got, want) if i %% 2 == 0 else ts.f16_same(got, want) == (True, 0)
    print(case["name"], "ok" if ok else "DIFFERS")
    bad += int(not ok)
print("FIRST_OK" if bad == 0 else "FIRST_FAIL")
"""


@pytest.mark.gpu
def test_the_first_softmax_launch_of_a_process_may_be_the_longest_row():
    """the dynamic-LDS opt-in is a function-local static of shl_mi355x_softmax: everywhere else it follows small launches"""
    res = subprocess.run([sys.executable, "-c", FIRST_LAUNCH % HERE], capture_output=True, text=True, timeout=300)
    assert "FIRST_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("group", SUM_GROUPS)
def test_both_forms_of_the_running_sum_equal_the_plain_loop_bit_for_bit(gpu, group):
    _, hip, _ = gpu
    bad = []
    rows = [r for r in sum_rows() if r[0].startswith(group)]
    assert rows
    for name, terms, want in rows:
        for literal in (0, 1):
            got = np.zeros(1, dtype=np.float32)
            pkg.check(hip.shl_mi355x_debug_running_sum(terms.ctypes.data, terms.size, literal, got.ctypes.data), hip, name)
            same = (np.isnan(got[0]) and np.isnan(want)) or got.view(np.uint32)[0] == np.float32(want).view(np.uint32)
            if not same:
                bad.append("%s %s: %r (%#010x), the loop gives %r (%#010x)" % (
                    name, "literal" if literal else "scan", float(got[0]), int(got.view(np.uint32)[0]), float(want),
                    int(np.float32(want).view(np.uint32))))
    assert not bad, "%d of %d sums differ:\n%s" % (len(bad), 2 * len(rows), "\n".join(bad[:20]))
    one = np.zeros(1, dtype=np.float32)
    assert hip.shl_mi355x_debug_running_sum(rows[0][1].ctypes.data, 0, 0, one.ctypes.data) == -2
    assert hip.shl_mi355x_debug_running_sum(rows[0][1].ctypes.data, 8193, 0, one.ctypes.data) == -2

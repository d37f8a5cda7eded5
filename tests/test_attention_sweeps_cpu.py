"""attention_sweeps.all_cases() without a GPU: a pass on each case means something (the fused kernel exists for it, rows of p
that are peaked but not one-hot, an output that spreads, scores off the rails), the int8 mfma form's formula against the oracle
chain -- bit for bit inside the plan-time proof, inside DESIGN's gate outside it --, and the list holds what it was written to
hold: every d, dv, key count, offset and p record, both sides of the table boundary, the three wave counts, the proof's two
sides in every stratum, and a default class that the library itself calls the default class."""
import ctypes as C

import numpy as np
import pytest

import attention_cases as ac
import attention_sweeps as sw
import matmul_cases as mc
from cases import pkg
from test_attention_cpu import FAR, waves_of

CASES = sw.all_cases()
IDS = [sw.case_id(c) for c in CASES]
TABLE_ABOVE = 256  # csrc/attention_canon.h:ATT_TABLE_ABOVE


@pytest.fixture(scope="module")
def chains():
    return {c["name"]: ac.oracle_chain(c) for c in CASES}


def row_spread(case, chain):
    """the distinct values of every row of p"""
    p = mc.bits(chain["p"]).reshape(-1, case["t"])
    return np.array([np.unique(row).size for row in p])


def halved(case):
    """p under 2^-7: half the levels of the other records"""
    return case["dtype"] == "int8" and case["p_q"][0] == 2.0 ** -7


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_pass_on_this_case_means_something(case, chains):
    chain = chains[case["name"]]
    assert ac.expect_fused(case)
    outs = np.unique(mc.bits(chain["out"])).size
    assert outs > 8, "the output holds %d distinct values" % outs
    rows = row_spread(case, chain)
    low, median, few = int(rows.min()), float(np.median(rows)), float(np.mean(rows <= 4))
    print("%s: rows of p hold at least %d, in the median %g distinct values; %.3f of them 4 or fewer; the output %d"
          % (case["name"], low, median, few, outs))
    if case["d"] in (1, 3):  # rank-1 and rank-3 scores: a few rows are nearly flat whatever the records
        assert median > 8 and few <= 0.20, (median, few)
    elif halved(case):
        assert low >= 5, low
    else:
        assert case["d"] >= 7
        assert low >= 5 and median > 8, (low, median)
    if case["dtype"] != "int8":
        return
    assert np.mean((chain["s"] == 127) | (chain["s"] == -128)) < 0.02  # (no row of scores is flat because the record clamped it)
    formula = ac.device_formula(case)
    if ac.both_exact(case):
        for key in ("s", "p", "out"):
            mc.assert_same(formula[key], chain[key], "%s: %s by the mfma form's formula vs the oracle chain" % (case["name"], key))
    else:
        mc.assert_within_gate(formula["out"], chain["out"], case["name"] + ": the mfma form's formula vs the oracle chain")


def test_the_list_covers_what_it_must():
    assert 80 <= len(CASES) <= 120
    for dtype in ("int8", "f16"):
        cs = [c for c in CASES if c["dtype"] == dtype]
        assert {1, 3, 7, 8, 15, 16, 17, 24, 31, 32, 33, 48, 63} <= {c["d"] for c in cs}, dtype
        assert {1, 3, 5, 7, 8, 16, 17, 31, 32, 33, 63, 65, 130} <= {c["dv"] for c in cs}, dtype
        default = [c for c in cs if c["stratum"] == "default"]
        assert set(sw.DEFAULT_D) <= {c["d"] for c in default} and set(sw.DVS) <= {c["dv"] for c in default}, dtype
        assert {768, 769, 800, 850, 1023} == set(sw.DEFAULT_T) <= {c["t"] for c in default}, dtype
        for c in default:
            assert c["batches"] == 1 and sw.min_rows(c["t"]) <= c["s"] <= sw.min_rows(c["t"]) + 11 and (c["s"] + 31) // 32 >= 3
            assert c["s"] % 32 != 0, "the last row tile is ragged"
        assert {(c["has_scale"], c["has_scale"] and c["scale_first"]) for c in default} == {(True, False), (True, True), (False, False)}
        plain = [c for c in default if (c["s"], c["t"], c["d"], c["dv"]) == (86, 768, 32, 32)]
        assert {c["regime"] for c in plain} == ({"pow2", "conv"} if dtype == "int8" else {"f16"})
        small = [c for c in cs if c["stratum"] == "small"]
        assert {33, 48, 63} <= {c["d"] for c in small if 768 <= c["t"] <= 1023}
        assert any((c["d"], c["dv"], c["s"], c["t"]) == (33, 7, 257, 257) for c in small)
        short = {(c["batches"], c["s"], c["t"], c["d"], c["dv"]) for c in cs if c["stratum"] == "short"}
        assert {(24, 33, 97, 32, 32), (70, 17, 65, 16, 8), (9, 65, 130, 7, 5), (40, 33, 65, 1, 1)} <= short and any(k[3] == 3 for k in short)
        # every offset on every operand, one operand at a time; all four at once; on four shapes
        es = 1 if dtype == "int8" else 2
        off = [c for c in cs if c["stratum"] == "unaligned"]
        assert all(c.get("offsets") for c in off) and all("offsets" not in c for c in cs if c["stratum"] != "unaligned")
        single = {next(iter(c["offsets"].items())) for c in off if len(c["offsets"]) == 1}
        assert single == {(operand, o) for operand in ("q", "k", "v", "out") for o in (es, 4, 8)}, dtype
        assert any(len(c["offsets"]) == 4 for c in off)
        shapes = {(c["s"], c["t"], c["d"], c["dv"]) for c in off}
        assert {(64, 64, 64, 64), (86, 768, 32, 32), (33, 65, 64, 64), (33, 64, 64, 130)} <= shapes
        # whole rows of 16-byte pieces gathered element by element, and an output off the grid
        assert any(c["d"] * es % 16 == 0 and c["offsets"].get(operand, 0) % 16 for c in off for operand in ("q", "k"))
        assert any(c["dv"] * es % 16 == 0 and c["offsets"].get("v", 0) % 16 for c in off)
        # the wave counts and both softmax paths
        assert {waves_of(dtype, c["batches"], c["s"], c["t"]) for c in cs} == {16, 8, 4}, dtype
    i8 = [c for c in CASES if c["dtype"] == "int8"]
    assert {c["t"] > TABLE_ABOVE for c in i8} == {True, False}
    assert {c["regime"] for c in i8} == {"pow2", "conv"}
    assert all(c["d"] > 3 for c in i8 if c["t"] > 130), "int8 heads of 1 and 3 stay on short rows"
    for key in ("q_q", "k_q", "v_q"):
        assert {-128, 0, 127} <= {c[key][1] for c in i8 if c["stratum"] in ("default", "small", "short")}, key
    # the probability records: each on a short row, on 97 keys with converter scales and zv = 4, and on the default class
    for _, p_q in sw.P_RECORDS:
        cs = [c for c in i8 if c["stratum"] == "p_record" and c["p_q"] == p_q]
        assert {65, 97, 768} <= {c["t"] for c in cs}, p_q
        assert any(c["t"] == 97 and c["regime"] == "conv" and c["v_q"][1] == 4 for c in cs), p_q
        assert any((c["s"], c["t"], c["d"], c["dv"]) == (86, 768, 32, 32) for c in cs), p_q
    assert {c["p_q"] for c in i8} == {ac.P_Q} | {p_q for _, p_q in sw.P_RECORDS}
    assert any(c["p_q"][1] == 0 and c["v_q"][1] != 0 for c in i8), "the p_zp == 0 side of the correction with a row-sum term"
    assert any(c["p_q"][1] == 0 and c["t"] > TABLE_ABOVE for c in i8) and any(c["p_q"][1] == 0 and c["t"] <= TABLE_ABOVE for c in i8)
    for stratum in ("default", "small", "short", "unaligned", "p_record"):
        assert {ac.both_exact(c) for c in i8 if c["stratum"] == stratum} == {True, False}, stratum


def test_the_default_class_is_what_the_library_fuses_unasked(built, monkeypatch):
    hip = pkg.load_hip()
    monkeypatch.delenv("SHL_MI355X_MATMUL_FORM", raising=False)
    for c in CASES:
        want = int(c["d"] <= 32 and c["t"] >= 768)
        assert want or c["stratum"] != "default"
        assert hip.shl_mi355x_attention_by_default(*FAR, C.byref(ac.desc(c))) == want, c["name"]

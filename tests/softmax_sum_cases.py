"""Crafted terms for softmax's float running sum  acc = (float)((double)acc + e[j])  (csrc/pool_softmax.hip:
running_sum_exact and running_sum_literal, both reachable through shl_mi355x_debug_running_sum).

After exp() a step whose double sum lies exactly half-way between two floats happens about once per 2^29 elements, and a
wrong tie moves a binary16 softmax output about once per 2^13 elements: softmax outputs cannot show a fault of the scan's
tie branch.  These rows can: every one is built so that a stop of the scan (a tie, a sum that leaves its binade, an inf or
NaN term, a subnormal sum) falls on a chosen element, i.e. on a chosen lane and a chosen place inside the lane.

  rows()            [(name, float64 terms)], the same for every run (seeded by SHL_TEST_FUZZ_SEED)
  reference(terms)  the plain loop, as float32
  classify(terms)   the steps of that loop: ties (and which way they went), binade exits, and where in a round of the
                    scan each of them falls

Pure Python, no GPU, no package import.
"""
import os

import numpy as np

BASE_SEED = int(os.environ.get("SHL_TEST_FUZZ_SEED", "20261018"))

TIE_K = (0, 1, 2, 7)
TIE_S = (1.0, 1.0 + 2.0 ** -23, 3.5, 2.0 ** -100, float(np.float32(1e30)), 2.0 ** -126)
# the issue's positions and 2, 6 and 254: its list holds no position with pos % 4 == 2
TIE_POS = (0, 1, 2, 3, 4, 5, 6, 63, 64, 200, 254, 255, 256, 300)
EXIT_POS = tuple(range(0, 260, 7))
EXP_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 1000, 2000, 8192)
MAX_TERMS = 8192


def f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float32(x))


def ulp(s):
    """the spacing of floats in s's binade (s a positive normal float)"""
    return 2.0 ** (int(np.floor(np.log2(s))) - 23)


def reference(terms):
    acc = 0.0
    for e in np.asarray(terms, dtype=np.float64).tolist():
        acc = f32(acc + e)
    return np.float32(acc)


def _exponent(f):
    return (int(np.float32(f).view(np.uint32)) >> 23) & 0xFF


def classify(terms):
    """-> list of dict(index, offset, tie, up, exit) for the steps of the plain loop that are a tie or a binade exit.
    offset: the element's distance from the start of its round of the scan (pool_softmax.hip:running_sum_exact: a round
    takes 256 elements, lane l the four from 4 l on, and ends behind the first tie or exit; a sum that is zero,
    subnormal, inf or NaN takes single steps), so lane = offset // 4 and the place inside the lane = offset % 4.
    Every value comes from the plain loop; only the round's start is bookkeeping."""
    out = []
    acc, start = 0.0, 0
    for i, e in enumerate(np.asarray(terms, dtype=np.float64).tolist()):
        ea = _exponent(acc)
        d = acc + e  # the double sum (rounded to double, as in the reference)
        nxt = f32(d)
        if ea == 0 or ea == 0xFF:  # no round: a literal step
            acc, start = nxt, i + 1
            continue
        if i - start == 256:
            start = i
        tie = up = False
        if np.isfinite(d) and np.isfinite(nxt) and nxt != d:
            other = float(np.nextafter(np.float32(nxt), np.float32(np.inf if d > nxt else -np.inf)))
            tie = np.isfinite(other) and (nxt + other) / 2 == d  # (both exact in double)
            up = nxt > d
        leaves = _exponent(nxt) > ea
        if tie or leaves:
            out.append(dict(index=i, offset=i - start, tie=bool(tie), up=bool(up), exit=bool(leaves)))
            start = i + 1
        acc = nxt
    return out


def _fill(rng, n, u):
    """n small terms for a sum whose ulp is u: below one ulp and a few ulps, never a multiple of u / 2"""
    t = np.where(rng.random(n) < 0.5, rng.random(n), 8.0 * rng.random(n)) * u
    return t.tolist()


def _sum(terms):
    return float(reference(terms))


def rows():
    rng = np.random.default_rng([BASE_SEED, 4242])
    out = []
    # a tie on a chosen element: s, `pos` small terms, (k + 1/2) ulp, a short tail
    for si, s in enumerate(TIE_S):
        u = ulp(s)
        for k in TIE_K:
            for pos in TIE_POS:
                t = [s] + _fill(rng, pos, u) + [(k + 0.5) * u] + _fill(rng, int(rng.integers(3, 40)), u)
                out.append(("tie_s%d_k%d_pos%d" % (si, k, pos), t))
    # runs of ties back to back, odd and even sums, every k
    for si, s in enumerate(TIE_S):
        u = ulp(s)
        for n in (2, 5, 64, 300):
            ks = rng.choice(TIE_K, n)
            out.append(("ties_s%d_n%d" % (si, n), [s] + ((ks + 0.5) * u).tolist() + _fill(rng, 7, u)))
    # the sum leaves its binade on a chosen element: it lands exactly on 2^(E+1), or stops one ulp short of it and
    # leaves on the next element; through many small terms, or through one large term
    for s in (1.75, 2.0 ** -100 * 1.9375, float(np.float32(1e30))):
        u = ulp(s)
        top = 2.0 ** 24 * u  # 2^(E+1)
        for pos in EXIT_POS:
            head = [s] + _fill(rng, pos, u)
            acc = _sum(head)
            assert s <= acc < top - 8 * u
            out.append(("exit_on_s%g_pos%d" % (s, pos), head + [top - acc] + _fill(rng, 9, 2 * u)))
            out.append(("exit_short_s%g_pos%d" % (s, pos), head + [top - u - acc, 0.75 * u] + _fill(rng, 9, 2 * u)))
    for pos in EXIT_POS:
        head = [1.0] + _fill(rng, pos, 2.0 ** -23)
        out.append(("exit_big_pos%d" % pos, head + [float(rng.integers(3, 4000)) + rng.random()] + _fill(rng, 9, 2.0 ** -12)))
    # terms that end every round for good: overflow, inf, NaN
    for pos in EXIT_POS:
        head = [1.0] + _fill(rng, pos, 2.0 ** -23)
        for name, v in (("1e300", 1e300), ("inf", np.inf), ("nan", np.nan)):
            out.append(("%s_pos%d" % (name, pos), head + [v] + _fill(rng, 5, 1.0)))
    # a subnormal start: single steps until the sum is normal, then rounds; and a sum that never gets there
    for n in (1, 3, 64, 300):
        t = (rng.integers(1, 2000, n) * 2.0 ** -149).tolist()
        out.append(("subnormal_start_n%d" % n, t + [2.0 ** -126] + _fill(rng, 70, 2.0 ** -149) + [1.5 * 2.0 ** -149, 0.5 * 2.0 ** -149]))
        out.append(("subnormal_only_n%d" % n, (rng.integers(1, 3, n) * 2.0 ** -149).tolist()))
    # what softmax itself produces
    for n in EXP_LENGTHS:
        x = rng.standard_normal(n) * 4
        out.append(("exp_normal_n%d" % n, np.exp(x - x.max()).tolist()))
        out.append(("exp_rising_n%d" % n, np.exp(np.linspace(-60, 0, n)).tolist()))
        out.append(("exp_plateau_n%d" % n, np.ones(n).tolist()))
    res = [(name, np.asarray(t, dtype=np.float64)) for name, t in out]
    assert all(1 <= t.size <= MAX_TERMS for _, t in res)
    return res

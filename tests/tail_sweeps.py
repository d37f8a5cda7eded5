"""Seeded, stratified draws for the kernels behind the convolutions -- pool_softmax.hip (global_avgpool2d in its two kernel
forms, softmax), elementwise.hip (relu / relu6 int8 and binary16, add) and conv_gemv.hip:pool_gemv_i8_kernel -- in the idiom
of family_sweeps.py.

  draw(family, i)        the description of case i: shapes, records, the strata it fills (no arrays)
  case_seed(family, i)   the seed of its operands
  build(family, i)       the problem itself: a tail.siso_oracle / tail.siso_run case ("pool_gemv": keywords for
                         cases.make_case and the pooling's operands)
  specials(case)         index of the elements that hold planted binary16 specials (None: an ordinary case)

Pure Python, no GPU, no package import: tests/test_tail_sweeps.py checks the draws on any machine and runs them on the
device.  The strata (filled round-robin by the case index, so they hold for every seed) come from the host code; each rule
restated here names the function it restates.  Free parameters are random: SHL_TEST_FUZZ_SEED moves them.

What the strata cannot hold, by arithmetic: global_avgpool_nhwc_i8_kernel runs only where C % 4 == 0, so n * C is a
multiple of 4 and never 1 or 63 modulo its block of 64; the draws take the nearest residues, 4 and 60.
"""
import os

import numpy as np

BASE_SEED = int(os.environ.get("SHL_TEST_FUZZ_SEED", "20261018"))  # (a one-off run elsewhere: set the variable)

FAMILIES = {
    "gap": dict(n=56, offset=1100, host=20),       # host: the cases that also run host-staged (one round of the strata)
    "softmax": dict(n=56, offset=1200, host=48),
    "relu": dict(n=32, offset=1300, host=16),
    "add": dict(n=32, offset=1400, host=10),
    "pool_gemv": dict(n=32, offset=1500, host=0),
}
CHUNK = 8   # cases per GPU test


def case_seed(family, i):
    return 930000 + FAMILIES[family]["offset"] * 10 + i


def _rng(family, i, seed):
    return np.random.default_rng([(BASE_SEED if seed is None else seed) + FAMILIES[family]["offset"], i])


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _q(scale, zp):
    return (float(np.float32(scale)), int(zp))


def _general_scale(rng, lo, hi):
    return float(np.float32(lo + (hi - lo) * rng.random()))


def _factor_map(rng, px, force):
    """(h, w) with h * w == px: force 0 -> H == 1, 1 -> W == 1, else a random non-square pair where one exists"""
    if force == 0:
        return 1, px
    if force == 1:
        return px, 1
    pairs = [(h, px // h) for h in range(1, px + 1) if px % h == 0]
    odd = [p for p in pairs if p[0] != p[1] and 1 not in p] or [p for p in pairs if p[0] != p[1]] or pairs
    return _pick(rng, odd)


# ------------------------------------------------------------------------------------------------ global_avgpool2d
GAP_COMBOS = (("int8", "NHWC"), ("int8", "NCHW"), ("f16", "NHWC"), ("f16", "NCHW"))
GAP_PX = {"1": (1, 1), "2to63": (2, 63), "64": (64, 64), "65": (65, 65), "66to200": (66, 200)}
# int8 NHWC, the only combination with two kernels: (pixel class, C % 4 == 0, rule for n * C)
# (14 cases: the fast form twice below its block of 64 and twice on each residue, in three pixel classes)
GAP_I8_NHWC = (("1", True, "lt64"), ("64", True, "fast0"), ("65", True, "gen0"), ("2to63", False, "gen1"),
               ("1", True, "fast4"), ("64", True, "fast60"), ("65", True, "free"), ("64", False, "gen255"),
               ("2to63", True, "fast60"), ("66to200", True, "free"), ("1", True, "fast0"), ("66to200", False, "gen255"),
               ("2to63", True, "fast4"), ("64", True, "lt64"))
GAP_NC = ("lt64", "gen0", "gen1", "gen255", "free")
GAP_F16_SPECIAL = {1: "big", 3: "inf", 5: "inf_pair", 7: "nan"}   # by the case's index inside its combination


def gap_fast_form(dtype, layout, c, px):
    """pool_softmax.hip:shl_mi355x_global_avgpool2d: global_avgpool_nhwc_i8_kernel, else global_avgpool_kernel"""
    return dtype == "int8" and layout == "NHWC" and c % 4 == 0 and px <= 64


def gap_strata(i):
    combo, j = i % 4, i // 4
    dtype, layout = GAP_COMBOS[combo]
    if combo == 0:
        pxc, c4, nc = GAP_I8_NHWC[j % 14]
    else:
        pxc, c4 = list(GAP_PX)[(j + combo) % 5], None
        nc = GAP_NC[(j + j // 5 + combo) % 5]
    special = GAP_F16_SPECIAL.get(j) if dtype == "f16" else None
    if special == "inf_pair" and pxc == "1":
        pxc = "2to63"   # (the pair needs two pixels of one channel)
    # records (int8): power-of-two and general scales, zero points at both ends, four cases that saturate at both ends
    return dict(dtype=dtype, layout=layout, px_class=pxc, c4=c4, nc_rule=nc, special=special,
                pow2=j % 2 == 0, saturate=dtype == "int8" and j in (2, 9), map_force={0: 0, 3: 1}.get(i % 6))


def _nc_ok(rule, nc):
    return {"lt64": nc < 64, "fast0": nc >= 64 and nc % 64 == 0, "fast4": nc > 64 and nc % 64 == 4,
            "fast60": nc > 64 and nc % 64 == 60, "gen0": nc > 256 and nc % 256 == 0, "gen1": nc > 256 and nc % 256 == 1,
            "gen255": nc > 256 and nc % 256 == 255, "free": True}[rule]


def _draw_gap(i, rng):
    s = gap_strata(i)
    px = int(rng.integers(*GAP_PX[s["px_class"]], endpoint=True))
    h, w = _factor_map(rng, px, s["map_force"])
    cmax = max(64, min(1400, 260000 // px))
    while True:
        n = int(rng.integers(1, 6))
        cs = [c for c in range(1, cmax + 1) if _nc_ok(s["nc_rule"], n * c) and (s["c4"] is None or (c % 4 == 0) == s["c4"])]
        if cs:
            break
    c = int(_pick(rng, cs))
    if s["dtype"] == "int8":
        zps = (-128, 127, int(rng.integers(-20, 21)))
        zi = int(rng.integers(-20, 21)) if s["saturate"] else zps[(i // 4) % 3]
        zo = int(rng.integers(-20, 21)) if s["saturate"] else zps[(i // 4 + 1) % 3]
        si = 2.0 ** -int(rng.integers(2, 6)) if s["pow2"] else _general_scale(rng, 0.02, 0.12)
        if s["saturate"]:
            so = si * (2.0 ** -7 if s["pow2"] else 0.0091)
        else:
            so = si * (2.0 ** int(rng.integers(-1, 2)) if s["pow2"] else _general_scale(rng, 0.5, 1.9))
        in_q, out_q = _q(si, zi), _q(so, zo)
    else:
        in_q = out_q = _q(1.0, 0)
    return dict(s, n=n, c=c, h=h, w=w, px=px, in_q=in_q, out_q=out_q, fast=gap_fast_form(s["dtype"], s["layout"], c, px))


def _build_gap(d, rng):
    n, h, w, c = d["n"], d["h"], d["w"], d["c"]
    spec = None
    if d["dtype"] == "int8":
        x = rng.integers(-128, 128, (n, h, w, c), dtype=np.int8)
    else:
        x = (3.0 * rng.standard_normal((n, h, w, c))).astype(np.float16)
        if d["special"]:
            cc = int(rng.integers(0, c))
            if d["special"] == "big":       # the fp32 sum leaves binary16's range, the average comes back into it
                x[0, :, :, cc] = np.float16(65504.0)
                if c > 1:
                    x[n - 1, :, :, (cc + 1) % c] = np.float16(-65504.0)
            elif d["special"] == "inf":
                x[0, h - 1, w - 1, cc] = np.float16(np.inf)
            elif d["special"] == "inf_pair":
                x[0, 0, 0, cc], x[0, h - 1, w - 1, cc] = np.float16(np.inf), np.float16(-np.inf)
            else:
                x[n - 1, h // 2, w // 2, cc] = np.float16(np.nan)
            spec = np.arange(n * c)   # (the whole output: tens to thousands of words)
    if d["layout"] == "NCHW":
        x = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    return dict(kind="pool", x=x, dtype=d["dtype"], layout=d["layout"], axis=1, in_q=d["in_q"], out_q=d["out_q"], special=spec)


# ------------------------------------------------------------------------------------------------ softmax
SM_INNER = {"1": (1, 1), "2to7": (2, 7), "64to300": (64, 300)}
SM_COUNT = {"1": (1, 1), "2to63": (2, 63), "64": (64, 64), "65to255": (65, 255), "256": (256, 256), "257to1023": (257, 1023),
            "1024to4864": (1024, 4864), "4865to8192": (4865, 8192)}
SM_IN_SCALES = (2.0 ** -7, 2.0 ** -3, 0.083, 1.0, 0.31)       # 2^-7: a nearly flat row; 1.0: most exponentials underflow
SM_OUT_Q = ((1.0 / 256, -128), (1.0 / 128, -128), (0.0047, -101))  # 1/128: saturates at the top
SM_F16_ROWS = ("normal", "rising", "falling", "plateau", "dominant", "pm65504",
               "some_ninf", "all_ninf", "one_pinf", "two_pinf", "one_nan")
SM_SPECIAL_ROWS = SM_F16_ROWS[6:]
SM_MAX_CNT = 8192            # pool_softmax.hip:SOFTMAX_MAX_CNT
SM_LDS_OPT_IN = 4865         # pool_softmax.hip:shl_mi355x_softmax: 9 * count + 5376 > 48 KiB


def softmax_lds_bytes(count):
    """pool_softmax.hip:shl_mi355x_softmax: e[count + 256] | red[256] | lut_e[256] | lut_q[256] | xb[count]"""
    return (count + 256) * 8 + 256 * 4 + 256 * 8 + 256 + count


def softmax_strata(i):
    """dtype = i % 2; the pair index p = i // 2 walks (count class, inner class) with periods 8 and 3: all 24 combinations,
    each in both dtypes.  The exact counts 4864, 4865 and 8192 sit on fixed pairs (8192 with inner > 1)."""
    p = i // 2
    cc, ic = list(SM_COUNT)[p % 8], list(SM_INNER)[p % 3]
    exact = {6: 4864, 7: 8192, 15: 4865}.get(p)
    return dict(dtype="int8" if i % 2 == 0 else "f16", count_class=cc, inner_class=ic, exact_count=exact,
                row_kind=SM_F16_ROWS[p % 11] if i % 2 else None, in_scale=SM_IN_SCALES[p % 5], out_rec=SM_OUT_Q[(p + p // 3) % 3])


def _draw_softmax(i, rng):
    s = softmax_strata(i)
    lo, hi = SM_COUNT[s["count_class"]]
    count = s["exact_count"] or int(rng.integers(lo, min(hi, lo + 500), endpoint=True))
    ilo, ihi = SM_INNER[s["inner_class"]]
    inner = int(rng.integers(ilo, ihi, endpoint=True))
    budget = 40000                                         # (the family's outputs stay under 2e6)
    if inner >= 64 and count * inner > budget:
        inner = int(rng.integers(64, max(64, budget // count), endpoint=True))
    omax = max(1, min(300 // inner, budget // (count * inner)))
    outer = 1 if (i // 2) % 4 == 0 else int(rng.integers(1, omax, endpoint=True))
    if s["dtype"] == "int8":
        in_q, out_q = _q(s["in_scale"], (-128, 127, int(rng.integers(-30, 31)))[(i // 2) % 3]), _q(*s["out_rec"])
    else:
        in_q = out_q = _q(1.0, 0)
    return dict(s, count=count, inner=inner, outer=outer, rows=outer * inner, in_q=in_q, out_q=out_q,
                lds_opt_in=softmax_lds_bytes(count) > 48 * 1024)


def _f16_row(kind, rng, n):
    if kind in ("normal",) + SM_SPECIAL_ROWS:
        r = 2.0 * rng.standard_normal(n)          # N(0, 4)
    elif kind == "rising":
        r = np.linspace(-60, 0, n)
    elif kind == "falling":
        r = np.linspace(0, -60, n)
    elif kind == "plateau":
        r = np.full(n, float(rng.integers(-8, 9)))
    elif kind == "dominant":
        r = rng.standard_normal(n) * 0.01 - 30
        r[int(rng.integers(0, n))] = 0
    else:  # pm65504
        r = np.where(rng.random(n) < 0.5, 65504.0, -65504.0)
        r[int(rng.integers(0, n))] = 65504.0
    r = r.astype(np.float16)
    pos = rng.permutation(n)
    if kind == "some_ninf":
        r[pos[:max(1, n // 3)] if n > 1 else []] = -np.inf
    elif kind == "all_ninf":
        r[:] = -np.inf
    elif kind == "one_pinf":
        r[pos[0]] = np.inf
    elif kind == "two_pinf":
        r[pos[:2]] = np.inf
    elif kind == "one_nan":
        r[pos[0]] = np.nan
    return r


def _build_softmax(d, rng):
    outer, count, inner = d["outer"], d["count"], d["inner"]
    shape = (outer, count) if inner == 1 else (outer, count, inner)
    spec = None
    if d["dtype"] == "int8":
        x = rng.integers(-128, 128, shape, dtype=np.int8)
    else:
        kind = d["row_kind"]
        x3 = np.empty((outer, count, inner), dtype=np.float16)
        special = kind in SM_SPECIAL_ROWS
        # a special sits in the first and the last row only: the rows between them must not feel it
        marked = {(0, 0), (outer - 1, inner - 1)}
        for o in range(outer):
            for k in range(inner):
                x3[o, :, k] = _f16_row(kind if not special or (o, k) in marked else "normal", rng, count)
        x = x3.reshape(shape)
        if special:
            idx = np.arange(x3.size).reshape(x3.shape)
            rows = [idx[o, :, k] for o, k in sorted(marked)]
            if outer * inner > 2:   # and one ordinary row next to them
                rows.append(idx[0, :, 1] if inner > 1 else idx[1, :, 0])
            spec = np.concatenate(rows)
    return dict(kind="softmax", x=x, dtype=d["dtype"], layout="NHWC", axis=1, in_q=d["in_q"], out_q=d["out_q"], special=spec)


# ------------------------------------------------------------------------------------------------ relu / relu6
RELU_I8_COUNTS = (1, 15, 16, 17, 4095, 4096, 4097)
RELU_I8_BIG = 8388608 + 87      # elementwise.hip:shl_mi355x_relu_i8: 2048 blocks x 256 lanes x 16 bytes, and a ragged tail
RELU_F16_COUNTS = (1, 255, 256, 257, 511, 4099, 65537)
ELT_F16_BIG = 1048576 + 300     # elementwise.hip:shl_mi355x_relu_f16 / shl_mi355x_add: 4096 blocks x 256 lanes
# output records by where the dequantised 6.0 lands: (class, scale, zero point)
#   tie      6 / 4 = 1.5 exactly: rint's tie, one float below 6 rounds the other way
#   edge     6 / scale + zp = 127 exactly
#   beyond   6 / scale + zp > 127: relu6's clamp is hidden behind the saturation
#   inside   a general scale
RELU_OUT = (("tie", 4.0, -3), ("edge", 6.0 / 255.0, -128), ("beyond", 0.011, 0), ("inside", 0.0731, -128 + 9))


def relu_grid(dtype, count):
    """elementwise.hip:shl_mi355x_relu_i8 / shl_mi355x_relu_f16 -> (blocks, passes of the grid-stride loop)"""
    if dtype == "int8":
        blocks = max(1, min((count // 16 + 255) // 256, 2048))
        return blocks, -(-(count // 16) // (blocks * 256))
    blocks = min((count + 255) // 256, 4096)
    return blocks, -(-count // (blocks * 256))


def relu_strata(i):
    a = i // 2                     # the case's index inside its dtype
    relu6, slot = a % 2 == 1, a // 2
    if i % 2 == 0:
        count = RELU_I8_COUNTS[slot] if slot < 7 else (RELU_I8_BIG if relu6 else 65537)
        out = RELU_OUT[slot % 4]
        if out[0] == "beyond" and not relu6:   # the output zero point at the top: whatever relu gives saturates
            out = ("beyond", out[1], 127)
        return dict(dtype="int8", relu6=relu6, count=count, out=out, in_zp_class=("min", "mid", "max", "mid")[(slot + a) % 4])
    count = RELU_F16_COUNTS[slot] if slot < 7 else (ELT_F16_BIG if relu6 else 1000)
    return dict(dtype="f16", relu6=relu6, count=count, out=None, in_zp_class=None)


def _draw_relu(i, rng):
    s = relu_strata(i)
    if s["dtype"] == "int8":
        zi = {"min": -128, "max": 127, "mid": int(rng.integers(-40, 41))}[s["in_zp_class"]]
        si = float(np.float32(_pick(rng, (0.5, 0.25, 0.173))))   # the top of the range dequantises well beyond 6 (not with zp 127: all <= 0)
        in_q, out_q = _q(si, zi), _q(s["out"][1], s["out"][2])
    else:
        in_q = out_q = _q(1.0, 0)
    blocks, passes = relu_grid(s["dtype"], s["count"])
    return dict(s, in_q=in_q, out_q=out_q, blocks=blocks, passes=passes, abi_only=passes > 1)


F16_RELU_PLANTS = (0x8000, 0x0000, 0x0001, 0x8001, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x4600, 0x4601, 0x45FF, 0x7BFF, 0xFBFF)


def _build_relu(d, rng):
    n = d["count"]
    if d["dtype"] == "int8":
        x = rng.integers(-128, 128, (1, n), dtype=np.int8)
        x[0, -1] = 127                # (the ragged tail's last byte: the largest value there is)
        if n > 2:
            x[0, 0], x[0, n // 2] = -128, 127
    else:
        x = (4.0 * rng.standard_normal((1, n))).astype(np.float16)
        v = x.view(np.uint16)
        k = min(n, len(F16_RELU_PLANTS))   # -0, subnormals, inf, NaN, 6 and its neighbours, +-65504: at both ends
        start = int(rng.integers(0, len(F16_RELU_PLANTS)))
        plants = np.roll(np.array(F16_RELU_PLANTS, dtype=np.uint16), -start)
        v[0, :k] = plants[:k]
        v[0, n - k:] = plants[:k]
    return dict(kind="relu6" if d["relu6"] else "relu", x=x, dtype=d["dtype"], layout="NHWC", axis=1, in_q=d["in_q"],
                out_q=d["out_q"], special=None)


# ------------------------------------------------------------------------------------------------ add
ADD_COUNTS = (1, 255, 256, 257, 65537)
# binary16 operands whose sums meet every branch of the reference's rounding: inf - inf, NaN, signed zeros, the overflow
# that saturates (65504 + 65504, 65504 + 16: the tie at the top), the subnormal sum 2^-24 + 2^-24, the ties 1 + 2^-11
# (to even: down) and (1 + 2^-10) + 2^-11 (to even: up)
ADD_PLANTS = (0x7C00, 0xFC00, 0x7E00, 0x0000, 0x8000, 0x7BFF, 0xFBFF, 0x4C00, 0x0001, 0x3C00, 0x1000, 0x3C01)
ADD_PAIRS = [(a, b) for a in ADD_PLANTS for b in ADD_PLANTS]


def add_grid(count):
    """elementwise.hip:shl_mi355x_add -> (blocks, passes of the grid-stride loop)"""
    blocks = min((count + 255) // 256, 4096)
    return blocks, -(-count // (blocks * 256))


def add_strata(i):
    slot = i // 2
    count = ADD_COUNTS[slot % 5] if slot < 15 else ELT_F16_BIG
    # int8: exact (power-of-two) and general records; "saturate": a small output scale, both ends
    return dict(dtype="int8" if i % 2 == 0 else "f16", count=count, pow2=slot % 2 == 0, saturate=slot % 3 == 1)


def _draw_add(i, rng):
    s = add_strata(i)
    if s["dtype"] == "int8":
        def rec(lo, hi):
            sc = 2.0 ** -int(rng.integers(2, 7)) if s["pow2"] else _general_scale(rng, lo, hi)
            zps = (-128, 127, int(rng.integers(-30, 31)), int(rng.integers(-30, 31)))
            return _q(sc, zps[2] if s["saturate"] else _pick(rng, zps))
        in_q, in1_q = rec(0.02, 0.09), rec(0.02, 0.09)
        so = max(in_q[0], in1_q[0]) * (0.25 if s["saturate"] else 2.0) * (1.0 if s["pow2"] else 1.037)
        out_q = _q(so, int(rng.integers(-20, 21)) if s["saturate"] else _pick(rng, (-128, 127, int(rng.integers(-30, 31)))))
    else:
        in_q = in1_q = out_q = _q(1.0, 0)
    blocks, passes = add_grid(s["count"])
    return dict(s, in_q=in_q, in1_q=in1_q, out_q=out_q, blocks=blocks, passes=passes, abi_only=passes > 1)


def _build_add(d, rng, i):
    n = d["count"]
    spec = None
    if d["dtype"] == "int8":
        x, y = rng.integers(-128, 128, (1, n), dtype=np.int8), rng.integers(-128, 128, (1, n), dtype=np.int8)
        for a in (x, y):
            a[0, 0], a[0, -1] = (-128, 127) if n > 1 else (127, 127)
    else:
        x, y = (5.0 * rng.standard_normal((1, n))).astype(np.float16), (5.0 * rng.standard_normal((1, n))).astype(np.float16)
        pairs = np.array(ADD_PAIRS, dtype=np.uint16)
        if n >= len(pairs):     # every pair, at the front; behind the grid's first pass too where there is one
            at = [0] + ([n - len(pairs)] if n >= 2 * len(pairs) else [])
        else:                   # (one element: the pairs go round with the case index)
            pairs, at = pairs[[(7 * i + 3) % len(ADD_PAIRS)]][:n], [0]
        for a0 in at:
            x.view(np.uint16)[0, a0:a0 + len(pairs)] = pairs[:, 0]
            y.view(np.uint16)[0, a0:a0 + len(pairs)] = pairs[:, 1]
        spec = np.concatenate([np.arange(a0, a0 + len(pairs)) for a0 in at])
    return dict(kind="add", x=x, y=y, dtype=d["dtype"], layout="NHWC", axis=1, in_q=d["in_q"], in1_q=d["in1_q"],
                out_q=d["out_q"], special=spec)


# ------------------------------------------------------------------------------------------------ pool + classifier
PG_PX = (1, 2, 15, 16, 17, 63, 64)
PG_C = (16, 48, 1008, 1024, 1040, 2048, 4096)
PG_CO = (1, 3, 4, 5, 63, 64, 65, 129, 1000)


def pool_gemv_instance(px):
    """conv_gemv.hip:launch_pool_gemv: pool_gemv_i8_kernel<16> up to 16 pixels, <64> beyond"""
    return 16 if px <= 16 else 64


def pool_gemv_admissible(n, px, c):
    """conv_gemv.hip:pool_gemv_pick (with conv_gemv_pick for a 1 x 1 map of n images)"""
    return 1 <= n <= 8 and 1 <= px <= 64 and c % 16 == 0 and c <= 32768 and px * c < (1 << 31)


def pool_gemv_strata(i):
    """periods 7 (pixels), 7 shifted by the round (C), 9 (Co) and 8 (images: grid.y): every value at least three times in 32
    cases, and each template instance with C on both sides of the GEMV's 1024-lane chunk"""
    return dict(px=PG_PX[i % 7], c=PG_C[(i + i // 7 + 3) % 7], co=PG_CO[i % 9], n=1 + i % 8)


def _draw_pool_gemv(i, rng):
    s = pool_gemv_strata(i)
    h, w = _factor_map(rng, s["px"], {0: 0, 3: 1}.get(i % 6))
    return dict(s, h=h, w=w, instance=pool_gemv_instance(s["px"]), act=(i // 2) % 3, exact=i % 2 == 0,
                per_channel=(i // 6) % 2 == 1, in_q=_q(_general_scale(rng, 0.02, 0.07), int(rng.integers(-20, 20))))


def _build_pool_gemv(d, rng):
    x = rng.integers(-128, 128, (d["n"], d["h"], d["w"], d["c"]), dtype=np.int8)
    conv_kw = dict(n=d["n"], h=1, w=1, c=d["c"], co=d["co"], k=(1, 1), pad=(0, 0, 0, 0), act=d["act"], exact=d["exact"],
                   per_channel=d["per_channel"])
    return dict(kind="pool_gemv", x=x, in_q=d["in_q"], conv_kw=conv_kw, n=d["n"], px=d["px"], c=d["c"], co=d["co"])


# ------------------------------------------------------------------------------------------------ entry points
_DRAW = {"gap": _draw_gap, "softmax": _draw_softmax, "relu": _draw_relu, "add": _draw_add, "pool_gemv": _draw_pool_gemv}
STRATA = {"gap": gap_strata, "softmax": softmax_strata, "relu": relu_strata, "add": add_strata, "pool_gemv": pool_gemv_strata}


def draw(family, i, seed=None):
    return _DRAW[family](i, _rng(family, i, seed))


def build(family, i, seed=None):
    """the operands come from case_seed alone; the shapes and records from draw()"""
    d = draw(family, i, seed)
    rng = np.random.default_rng(case_seed(family, i))
    if family == "add":
        case = _build_add(d, rng, i)
    else:
        case = {"gap": _build_gap, "softmax": _build_softmax, "relu": _build_relu, "pool_gemv": _build_pool_gemv}[family](d, rng)
    case.update(name="%s_%02d" % (family, i), family=family, index=i, draw=d)
    return case


def specials(case):
    return case.get("special")


def special_cases(seed=None):
    """(family, i) of every binary16 case of gap, softmax and add that holds planted specials"""
    out = []
    for fam in ("gap", "softmax", "add"):
        for i in range(FAMILIES[fam]["n"]):
            s = STRATA[fam](i)
            if s["dtype"] == "f16" and (fam == "add" or (fam == "gap" and s["special"]) or
                                        (fam == "softmax" and s["row_kind"] in SM_SPECIAL_ROWS)):
                out.append((fam, i))
    return out


def f16_same(got, want):
    """the rule of test_f16_special_values.py: NaN in the same places (the sign of a NaN is the host's, not the operation's),
    the same words everywhere else.  -> (NaN places equal, number of differing words outside them)"""
    g, e = np.ascontiguousarray(got).view(np.uint16).ravel(), np.ascontiguousarray(want).view(np.uint16).ravel()
    g_nan, e_nan = (g & 0x7FFF) > 0x7C00, (e & 0x7FFF) > 0x7C00
    return bool(np.array_equal(g_nan, e_nan)), int(((g != e) & ~e_nan).sum())


def canonical_f16(a):
    """binary16 words with every NaN as 0x7E00 (for fixtures)"""
    v = np.ascontiguousarray(a).view(np.uint16).ravel().copy()
    v[(v & 0x7FFF) > 0x7C00] = 0x7E00
    return v

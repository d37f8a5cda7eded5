"""Seeded, stratified cases for the fused attention core (shl_mi355x_attention) where attention_cases.all_cases() has none:
heads shorter than one 64-byte slab of k, odd and tiny d and dv, operands off the 16-byte grid, and probability records other
than (1 / 256, -128).  Built on attention_cases._add, every case seeded by crc32(name); case["stratum"] names its stratum.

  default     the only class a session fuses unasked (csrc/attention_canon.h:att_default: d <= 32 on t >= 768 keys): d in
              1 (binary16), 8, 15, 16, 17, 24, 31, 32 on 768, 769, 800, 850, 1023 keys, dv a seeded permutation of 1, 3, 7, 16,
              17, 31, 32, 33, 63, 65; s = ceil(65537 / t) + a seeded 0 .. 11 is the fewest rows at which Q K^T is the mfma
              form's: three or four row tiles, the last one ragged; the multiply absent, second, first in turns, the regimes in
              turns, zero points cycling through the ends and small values; the plain s = 86, t = 768, d = dv = 32 in both regimes;
              one int8 case with p at zero point 0, which P V's plan-time proof admits up to 1023 keys
  small       d in 33, 48, 63 on 769 .. 1023 keys (outside the class: one slab of k with a zero-filled tail), and d = 33,
              dv = 7 on s = t = 257
  short       small heads on short rows, the mfma form reached through the batch count (the grid-size wave rule stays in
              play): d = 32, 16, 7, 3, 1; 520 workgroups get 4 waves.  int8 d = 1 and 3 live here only: rank-1 scores on a
              thousand keys give int8 rows of one to three distinct values
  unaligned   q, k, v and the output moved off the grid by one element, 4 and 8 bytes, one operand at a time, the twelve
              (operand, offset) pairs dealt over four shapes -- the base, the plain default-class case, s = 33 on t = 65, and
              dv = 130 --, and on two of the shapes all four at once: att_vec takes the load width from the pointer, so whole
              pieces of a row of d * es % 16 == 0 bytes are gathered element by element
  p_record    int8: p under (1 / 255 as float32, -128), (2^-8, 0), (2^-7, 0), (2^-7, 5), each on t = 65, on t = 97 with
              converter scales and zv = 4, and on the plain default-class case: p_zp == 0 is the other side of the P V
              column-sum correction, and the record goes through requant_i8 in the per-element and the per-row-table softmax
"""
import attention_cases as ac
from attention_cases import _rng
from pool_cases import _q

DEFAULT_D = (8, 15, 16, 17, 24, 31, 32)
DEFAULT_T = (768, 769, 800, 850, 1023)
DVS = (1, 3, 7, 16, 17, 31, 32, 33, 63, 65)
# (d, t) of the default class: every d twice or so, every t
DEFAULT_GRID = ((8, 768), (15, 769), (16, 800), (17, 850), (24, 1023), (31, 768), (32, 769), (8, 1023), (15, 850), (17, 800), (31, 1023),
                (32, 850))
MULS = (dict(), dict(has_scale=False), dict(scale_first=True))
# (zq, zk, zv): at the ends one operand of Q K^T at a time (the other centred, so that the scores do not saturate), small on all
ZERO_POINTS = ((0, 0, 0), (-128, 0, 127), (0, 127, -128), (5, -3, 4), (127, 0, 0), (0, -128, 0), (0, 0, 4))
OFFSETS = ("element", 4, 8)
OPERANDS = ("q", "k", "v", "out")
P_RECORDS = (("p255", _q(1.0 / 255, -128)), ("p2-8_z0", _q(2.0 ** -8, 0)), ("p2-7_z0", _q(2.0 ** -7, 0)), ("p2-7_z5", _q(2.0 ** -7, 5)))
# cases whose first seed missed test_attention_sweeps_cpu.py's conditions (one row of 94 with 4, one of 90 with 3 distinct values
# of p: its scores sat on a rail), seeded again under another name
RESEEDED = {("int8", 8, 768): "_b", ("int8", 17, 800): "_b"}
PLAIN = dict(s=86, t=768, d=32, dv=32)


def min_rows(t):
    """the fewest query rows at which one batch's Q K^T with k < 64 is the mfma form's (matmul_cases.expected_form)"""
    return -(-65537 // t)


def _sweep(out, stratum, name, dtypes=("int8", "f16"), **kw):
    for dtype in dtypes:
        kw_d = dict(kw)
        if dtype == "f16":  # binary16 has no records
            for key in ("zq", "zk", "zv", "p_q", "regime"):
                kw_d.pop(key, None)
        if "offsets" in kw_d:
            es = 1 if dtype == "int8" else 2
            kw_d["offsets"] = {k: (es if v == "element" else v) for k, v in kw_d["offsets"].items()}
        ac._add(out, name, dtype, **kw_d)
        out[-1]["stratum"] = stratum


def _default_class(out):
    for dtype in ("int8", "f16"):
        dvs = _rng("attention sweep dv " + dtype).permutation(DVS)
        for i, (d, t) in enumerate(DEFAULT_GRID):
            name = "def_d%d_t%d" % (d, t) + RESEEDED.get((dtype, d, t), "")
            rng = _rng("attention sweep " + name + dtype)
            zq, zk, zv = ZERO_POINTS[i % len(ZERO_POINTS)]
            _sweep(out, "default", name, (dtype,), s=min_rows(t) + int(rng.integers(12)), t=t, d=d, dv=int(dvs[i % len(DVS)]),
                   regime=("pow2", "conv")[i % 2], zq=zq, zk=zk, zv=zv, **MULS[i % 3])
    _sweep(out, "default", "def_plain", **PLAIN)
    _sweep(out, "default", "def_plain_conv", ("int8",), regime="conv", **PLAIN)
    _sweep(out, "default", "def_d1_t800", ("f16",), s=min_rows(800) + 5, t=800, d=1, dv=17)
    # p at zero point 0: 128 x 128 x 1023 < 2^24, so this one lies inside the proof for both products
    _sweep(out, "default", "def_d16_t800_p0", ("int8",), s=min_rows(800) + 3, t=800, d=16, dv=33, p_q=_q(2.0 ** -8, 0))


def _small_heads(out):
    _sweep(out, "small", "small_d33_t769", s=min_rows(769) + 2, t=769, d=33, dv=31, regime="conv", zq=5, zk=-3, zv=4)
    _sweep(out, "small", "small_d48_t850", s=min_rows(850) + 7, t=850, d=48, dv=17, has_scale=False)
    _sweep(out, "small", "small_d63_t1023", s=min_rows(1023), t=1023, d=63, dv=3, scale_first=True, zv=127)
    _sweep(out, "small", "small_d33_dv7_t257", s=257, t=257, d=33, dv=7)


def _short_rows(out):
    _sweep(out, "short", "short_b24_d32", batches=24, s=33, t=97, d=32, dv=32)
    _sweep(out, "short", "short_b70_d16_dv8", batches=70, s=17, t=65, d=16, dv=8, regime="conv", zq=5, zk=-3, zv=4)
    _sweep(out, "short", "short_b9_d7_dv5", batches=9, s=65, t=130, d=7, dv=5, has_scale=False)
    _sweep(out, "short", "short_b40_d1_dv1", batches=40, s=33, t=65, d=1, dv=1)
    _sweep(out, "short", "short_b30_d3_dv3", batches=30, s=33, t=70, d=3, dv=3, regime="conv", scale_first=True)
    _sweep(out, "short", "short_b520_d16", batches=520, s=2, t=65, d=16, dv=16, zv=-128)  # 520 workgroups: 4 waves each


def _unaligned(out):
    shapes = (("base", dict()), ("plain", dict(PLAIN)), ("s33_t65", dict(s=33, t=65, regime="conv")), ("dv130", dict(s=33, dv=130)))
    pairs = [(operand, offset) for operand in OPERANDS for offset in OFFSETS]
    for j, (operand, offset) in enumerate(pairs):
        tag, kw = shapes[j % len(shapes)]
        _sweep(out, "unaligned", "off_%s_%s%s" % (tag, operand, offset), offsets={operand: offset}, **kw)
    for (tag, kw), offsets in ((shapes[0], dict(q="element", k=4, v=8, out="element")), (shapes[1], dict(q=8, k="element", v=4, out=4))):
        _sweep(out, "unaligned", "off_%s_all" % tag, offsets=offsets, **kw)


def _p_records(out):
    for tag, p_q in P_RECORDS:
        _sweep(out, "p_record", "%s_t65" % tag, ("int8",), t=65, p_q=p_q)
        _sweep(out, "p_record", "%s_t97_conv_zv4" % tag, ("int8",), t=97, regime="conv", zv=4, p_q=p_q)
        _sweep(out, "p_record", "%s_plain" % tag, ("int8",), p_q=p_q, **PLAIN)


def all_cases():
    out = []
    _default_class(out)
    _small_heads(out)
    _short_rows(out)
    _unaligned(out)
    _p_records(out)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    assert 80 <= len(out) <= 120, len(out)
    return out


case_id = ac.case_id

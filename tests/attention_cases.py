"""Shared helpers for the fused attention core (shl_mi355x_attention): scores = Q K^T, [scores * a one-element constant],
softmax over the keys, P V as one launch.

  all_cases()     deterministic problems, seeded by crc32(name): the smallest shapes at which a kernel of 32 query rows per
                  workgroup, 128 keys / output columns per pass and 64-byte slabs of k can still go wrong -- the square base
                  (S = T = d = dv = 64), a ragged key block and a zero-padded K tail in P V (T = 65, 97), a ragged row tile and
                  a second one (S = 1, 33), 3 batches, an int8 K tail inside a slab and two slabs (d = 72, 128), dv = 40, the
                  boundary between the per-element and the per-row-table exponentials (T = 257, 320), the cap with S = 32,
                  grids of 260 and 520 workgroups (which get 8 and 4 waves each instead of 16);
                  with and without the multiply, the constant on either side; int8 records in powers of two and converter
                  scales, zero points 0, -128 and 127, p at (1 / 256, -128); binary16 data whose first sums are exact, and one
                  case with an inf and a NaN in q
  oracle_chain    the four layers through their oracles: matmul_cases.chain_ref, eltwise_cases.eltwise_numpy, tail.siso_oracle
  device_formula  int8 only: the chain with both products through matmul_cases.exact_ref -- what the mfma form computes
  both_exact      the plan-time proof (matmul_cases.is_exact) for both products
  desc / unfused_descs   the C ABI's descriptors: the fused call's, and the four unfused calls'
  run_both        (-m gpu) the fused launch and the four unfused calls on the same device buffers, with every intermediate
attention_sweeps.py builds its seeded strata on _add (a p record and byte offsets of the operands are its to choose).
The records are chosen so that rows are peaked, not flat: the softmax's input has a standard deviation of one to three units,
more for longer rows, and the case builder's conditions (test_attention_cpu.py) ask every row of p and the output for more than
8 distinct values.
"""
import ctypes as C
import math
import zlib

import numpy as np

import eltwise_cases
import matmul_cases as mc
import tail
from cases import pkg
from pool_cases import _q

CAP = pkg.ATTENTION_MAX_KEYS
P_Q = _q(1.0 / 256, -128)
NAN_P, INF_P = 0x7E00, 0x7C00
SPECIAL_ROWS = (3, 7)  # the query rows that hold the inf and the NaN of the one binary16 case with them


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _target_std(t):
    """the spread of the softmax's input: longer rows need more of it to stay peaked under p's 8 bits"""
    return 1.2 + 0.4 * max(0.0, math.log2(t / 64.0))


def _i8_records(c, regime, zq, zk, zv, p_q=P_Q):
    """records under which int8 data uniform over the whole range gives peaked rows: the true scores have a standard deviation
    of target * sqrt(d) with the multiply (the constant then is about 1 / sqrt(d)), of target without; the scores and the scaled
    scores spread over about 40 LSB each"""
    d, t = c["d"], c["t"]
    target = _target_std(t)
    # uniform bytes have a standard deviation of 73.9.  A far zero point of q widens the spread of a row's scores; one of k only
    # moves the row as a whole (by -zk sum q), which the scores' record has to hold but the softmax does not see
    aq = math.sqrt(73.9 ** 2 + zq ** 2)
    ak_all = math.sqrt(73.9 ** 2 + zk ** 2)
    true_std = target * (math.sqrt(d) if c["has_scale"] else 1.0)
    prod = true_std / (aq * 73.9 * math.sqrt(d))  # q_scale * k_scale
    if regime == "pow2":
        e = round(math.log2(prod))
        sq, sk = 2.0 ** (e // 2), 2.0 ** (e - e // 2)
    else:
        sq = math.sqrt(prod) * 1.07
        sk = prod / sq
    row_std = aq * 73.9 * math.sqrt(d) * sq * sk
    std_s = aq * ak_all * math.sqrt(d) * sq * sk
    c["q_q"], c["k_q"] = _q(sq, zq), _q(sk, zk)
    c["s_q"] = _q(std_s / 40.0, 5 if regime == "conv" else 0)
    if c["has_scale"]:
        c_real = target / row_std  # about 1 / sqrt(d); it takes up what rounding the scales to powers of two did to the spread
        c["c_q"] = _q(c_real / 90.0, 0) if regime == "conv" else _q(2.0 ** round(math.log2(c_real / 90.0)), 3)
        c["c"] = np.array([int(np.clip(round(c_real / c["c_q"][0]) + c["c_q"][1], -128, 127))], np.int8)
        std_sc = std_s * (float(c["c"][0]) - c["c_q"][1]) * c["c_q"][0]
        c["sc_q"] = _q(std_sc / 40.0, -7) if regime == "conv" else _q(2.0 ** round(math.log2(std_sc / 40.0)), 4)
    c["p_q"] = p_q
    sv = 0.0219 if regime == "conv" else 2.0 ** -5
    c["v_q"] = _q(sv, zv)
    # the output is a weighted mean of v: under v's own scale it spreads as v does
    c["out_q"] = _q(sv * 1.13, int(np.clip(round(zv / 1.13), -128, 127))) if regime == "conv" else _q(sv, zv)


def _add(out, name, dtype, s=64, t=64, d=64, dv=64, batches=1, has_scale=True, scale_first=False, regime="pow2", zq=0, zk=0, zv=0,
         special=False, p_q=None, offsets=None):
    """p_q: the probabilities' int8 record (P_Q unless given).  offsets: bytes by which run_both moves q, k, v and the output
    off the allocator's grid, {"q": 4, ...}; a case without them has no such key"""
    full = "%s_%s" % (name, "f16" if dtype == "f16" else "i8")
    rng = _rng("attention " + full)
    c = dict(name=full, dtype=dtype, batches=batches, s=s, t=t, d=d, dv=dv, has_scale=has_scale, scale_first=scale_first,
             regime=regime if dtype == "int8" else "f16", special=special)
    shapes = ((batches, s, d), (batches, t, d), (batches, t, dv))
    if dtype == "int8":
        c["q"], c["k"], c["v"] = (rng.integers(-128, 128, sh, dtype=np.int8) for sh in shapes)
        _i8_records(c, regime, zq, zk, zv, P_Q if p_q is None else p_q)
    else:
        # multiples of 2^-3 in [-2, 2] (without the multiply: of 2^-4 in [-3/4, 3/4]): every partial sum of q k^T is exact in
        # float32, so the scores are the same bits in any order of summation; v is non-negative, so nothing behind the softmax cancels
        # (integers -lo .. lo times the step have a standard deviation of lo step / sqrt(3); a score's is sqrt(d) times its square)
        step = 1.0 / 8 if has_scale else 1.0 / 16
        std = math.sqrt(_target_std(t)) if has_scale else math.sqrt(_target_std(t) / math.sqrt(d))
        lo = max(4, round(std * math.sqrt(3.0) / step))
        c["q"] = (rng.integers(-lo, lo + 1, shapes[0]) * step).astype(np.float16)
        c["k"] = (rng.integers(-lo, lo + 1, shapes[1]) * step).astype(np.float16)
        c["v"] = (rng.integers(0, 33, shapes[2]) / 16.0).astype(np.float16)
        one = _q(1.0, 0)
        for key in ("q_q", "k_q", "v_q", "s_q", "c_q", "sc_q", "p_q", "out_q"):
            c[key] = one
        if has_scale:
            c["c"] = np.array([0.17578125 * 8 / math.sqrt(d)], np.float16)
        if special:  # an infinity and a NaN in q: SPECIAL_ROWS of batch 0
            qu = c["q"].view(np.uint16)
            qu[0, SPECIAL_ROWS[0], 5], qu[0, SPECIAL_ROWS[1], 2] = INF_P, NAN_P
    if not has_scale:
        c["c"], c["c_q"], c["sc_q"] = None, _q(1.0, 0), _q(1.0, 0)
    if offsets:
        assert set(offsets) <= {"q", "k", "v", "out"} and all(0 <= o < 16 and o % c["q"].itemsize == 0 for o in offsets.values())
        c["offsets"] = dict(offsets)
    out.append(c)


def _both(out, name, **kw):
    for dtype in ("int8", "f16"):
        _add(out, name, dtype, **kw)


def all_cases():
    out = []
    _both(out, "base")
    _both(out, "base_const_first", scale_first=True)
    _both(out, "base_no_mul", has_scale=False)
    _both(out, "t65", t=65, regime="conv")
    _both(out, "t97", t=97)
    _both(out, "t97_no_mul", t=97, has_scale=False, regime="conv")
    _both(out, "s1", s=1)
    _both(out, "s33", s=33, regime="conv", scale_first=True)
    _both(out, "batches3", batches=3, s=33, t=65)
    _both(out, "d72", d=72)
    _both(out, "d128", d=128, regime="conv")
    _both(out, "dv40", dv=40)
    _both(out, "dv130", dv=130, s=33)  # a second pass over the output's columns
    _both(out, "t257", t=257, s=33)
    _both(out, "t256", t=256, s=33, regime="conv")  # the last length of the per-element exponentials
    _both(out, "t320", t=320, s=33)
    _both(out, "cap", s=32, t=CAP)
    # the workgroup's wave count (16 above, 8 at the cap for the LDS): 8 and 4 for the size of the grid
    _both(out, "groups260", batches=130, s=33, t=65, regime="conv")
    _both(out, "groups520", batches=520, s=1)
    # int8 zero points at the ends of the range, one operand at a time (the other centred, so that the scores do not saturate),
    # and small ones on both (both sum corrections at once)
    _add(out, "zq-128_zv127", "int8", zq=-128, zv=127)
    _add(out, "zk127_zv-128", "int8", zk=127, zv=-128, regime="conv")
    _add(out, "zq127", "int8", zq=127, t=97, scale_first=True)
    _add(out, "zk-128", "int8", zk=-128, s=33, has_scale=False)
    _add(out, "zq5_zk-3_zv4", "int8", zq=5, zk=-3, zv=4, d=72)
    _add(out, "zq5_zk-3_zv4_conv", "int8", zq=5, zk=-3, zv=4, regime="conv", dv=40)
    _add(out, "inf_nan", "f16", s=33, t=65, special=True)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def case_id(case):
    return case["name"]


# ------------------------------------------------------------------------------------ the chain on the CPU
def _qk_case(c):
    return dict(dtype=c["dtype"], a=c["q"], b=c["k"], a_q=c["q_q"], b_q=c["k_q"], out_q=c["s_q"], trans_a=False, trans_b=True,
                out_shape=(c["batches"], c["s"], c["t"]), k=c["d"], m=c["s"], n=c["t"], batches=c["batches"])


def _pv_case(c, p):
    return dict(dtype=c["dtype"], a=p, b=c["v"], a_q=c["p_q"], b_q=c["v_q"], out_q=c["out_q"], trans_a=False, trans_b=False,
                out_shape=(c["batches"], c["s"], c["dv"]), k=c["t"], m=c["s"], n=c["dv"], batches=c["batches"])


def both_exact(c):
    """the plan-time proof holds for Q K^T and for P V"""
    return mc.is_exact(_qk_case(c)) and mc.is_exact(_pv_case(c, None))


def _chain(c, product):
    s = product(_qk_case(c))
    x, x_q = s, c["s_q"]
    if c["has_scale"]:
        x = eltwise_cases.eltwise_numpy(dict(op="mul", dtype=c["dtype"], x=s, y=c["c"], in_q=c["s_q"], in1_q=c["c_q"], out_q=c["sc_q"],
                                             small_first=c["scale_first"]))
        x_q = c["sc_q"]
    p = tail.siso_oracle(dict(kind="softmax", x=x, dtype=c["dtype"], layout="NCHW", axis=2, in_q=x_q, out_q=c["p_q"]))
    return dict(s=s, x=x, p=p, out=product(_pv_case(c, p)))


def oracle_chain(c):
    """every intermediate and the output as the reference computes them"""
    return _chain(c, mc.chain_ref)


def device_formula(c):
    """int8: the chain with both products as the mfma form computes them (S exact, one float32 product, requantised)"""
    assert c["dtype"] == "int8"
    return _chain(c, mc.exact_ref)


def spread_report(c, chain):
    """(the fewest distinct values a row of p holds, distinct values of the output); the rows of a case's inf and NaN aside"""
    p = mc.bits(chain["p"]).reshape(-1, c["t"])
    rows = [r for r in range(p.shape[0]) if not (c["special"] and r in SPECIAL_ROWS)]
    return min(np.unique(p[r]).size for r in rows), np.unique(mc.bits(chain["out"])).size


# ------------------------------------------------------------------------------------ the C ABI's descriptors
def _raw(c):
    if not c["has_scale"]:
        return 0
    return int(c["c"][0]) if c["dtype"] == "int8" else int(c["c"].view(np.uint16)[0])


def desc(c):
    d = pkg.AttentionDesc()
    d.dtype = pkg.SHL_I8 if c["dtype"] == "int8" else pkg.SHL_F16
    d.batches, d.s, d.t, d.d, d.dv = c["batches"], c["s"], c["t"], c["d"], c["dv"]
    d.has_scale, d.scale_is_first, d.scale_raw = int(c["has_scale"]), int(c["has_scale"] and c["scale_first"]), _raw(c)
    for key in ("q", "k", "v", "s", "c", "sc", "p", "out"):
        scale, zp = c[key + "_q"]
        setattr(d, key + "_scale", scale)
        setattr(d, key + "_zp", zp)
    return d


def unfused_descs(c):
    """(matmul q k^T, mul or None, matmul p v) descriptors; the softmax call takes plain arguments"""
    dt = pkg.SHL_I8 if c["dtype"] == "int8" else pkg.SHL_F16
    b, s, t, d, dv = c["batches"], c["s"], c["t"], c["d"], c["dv"]
    qk = pkg.matmul_desc(dt, (b, s, d), (b, t, d), False, True, c["q_q"], c["k_q"], c["s_q"])
    pv = pkg.matmul_desc(dt, (b, s, t), (b, t, dv), False, False, c["p_q"], c["v_q"], c["out_q"])
    mul = None
    if c["has_scale"]:
        mul = eltwise_cases.mul_desc(dict(dtype=c["dtype"], in_q=c["s_q"], in1_q=c["c_q"], out_q=c["sc_q"], small_first=c["scale_first"]),
                                     (b, s, t), (1,))
    return qk, mul, pv


POISON = 0x5A
GUARD = 64
SLACK = 16  # room behind every buffer for a case's byte offsets (below 16 each)


def run_both(hip, dev, c):
    """(the fused launch's output, the four unfused calls' output, their probabilities, their scores, their softmax's input),
    all from the device; the bytes around the fused output are poisoned and must stay.  A case's "offsets" move q, k, v and
    the output (the fused one and the chain's alike) that many bytes off the allocator's grid: the unfused calls receive the
    same pointers"""
    b, s, t, dv = c["batches"], c["s"], c["t"], c["dv"]
    es = c["q"].itemsize
    dt = pkg.SHL_I8 if c["dtype"] == "int8" else pkg.SHL_F16
    off = c.get("offsets", {})
    room, bufs = [], {}

    def alloc(nbytes):
        room.append(dev.alloc(nbytes + SLACK))
        return room[-1]
    for key in ("q", "k", "v") + (("c",) if c["has_scale"] else ()):
        bufs[key] = alloc(c[key].nbytes) + off.get(key, 0)
        dev.upload(bufs[key], c[key])
    for key in ("s", "x", "p"):
        bufs[key] = alloc(b * s * t * es)
    out_bytes = b * s * dv * es
    frame = np.full(out_bytes + 2 * GUARD + SLACK, POISON, np.uint8)
    for key in ("chain", "fused"):
        bufs[key] = alloc(frame.nbytes)
        dev.upload(bufs[key], frame)
    first = GUARD + off.get("out", 0)  # the output's first byte in its frame
    p_chain, p_fused = bufs["chain"] + first, bufs["fused"] + first
    qk, mul, pv = unfused_descs(c)
    assert hip.shl_mi355x_matmul_kernel_name(bufs["q"], bufs["k"], bufs["s"], C.byref(qk)).decode() == pkg.MATMUL_MFMA
    assert hip.shl_mi355x_matmul_kernel_name(bufs["p"], bufs["v"], p_chain, C.byref(pv)).decode() == pkg.MATMUL_MFMA
    pkg.check(hip.shl_mi355x_matmul(bufs["q"], bufs["k"], bufs["s"], C.byref(qk), None), hip, "shl_mi355x_matmul (q k^T)")
    x, x_q = bufs["s"], c["s_q"]
    if c["has_scale"]:
        pkg.check(hip.shl_mi355x_mul(bufs["s"], bufs["c"], bufs["x"], C.byref(mul), None), hip, "shl_mi355x_mul")
        x, x_q = bufs["x"], c["sc_q"]
    pkg.check(hip.shl_mi355x_softmax(x, bufs["p"], dt, b * s, t, 1, x_q[0], x_q[1], c["p_q"][0], c["p_q"][1], None), hip,
              "shl_mi355x_softmax")
    pkg.check(hip.shl_mi355x_matmul(bufs["p"], bufs["v"], p_chain, C.byref(pv), None), hip, "shl_mi355x_matmul (p v)")
    d = desc(c)
    assert hip.shl_mi355x_attention_kernel_name(bufs["q"], bufs["k"], bufs["v"], p_fused, C.byref(d)).decode() == pkg.ATTENTION_MFMA
    pkg.check(hip.shl_mi355x_attention(bufs["q"], bufs["k"], bufs["v"], p_fused, C.byref(d), None), hip, "shl_mi355x_attention")
    got = dev.download(bufs["fused"], frame.shape, np.uint8)
    assert np.all(got[:first - GUARD] == POISON), "wrote in front of the output's guard"
    got = got[first - GUARD:]  # from the guard on: the frame of a case without offsets
    assert np.all(got[:GUARD] == POISON) and np.all(got[GUARD + out_bytes:] == POISON), "wrote outside the output"
    view = lambda raw, shape: raw.view(c["q"].dtype)[:int(np.prod(shape))].reshape(shape)
    fused = view(got[GUARD:GUARD + out_bytes].copy(), (b, s, dv))
    chain = view(dev.download(bufs["chain"], frame.shape, np.uint8)[first:first + out_bytes].copy(), (b, s, dv))
    p = dev.download(bufs["p"], (b, s, t), c["q"].dtype)
    scores = dev.download(bufs["s"], (b, s, t), c["q"].dtype)
    x_in = dev.download(x, (b, s, t), c["q"].dtype)
    for ptr in room:
        dev.free(ptr)
    return fused, chain, p, scores, x_in


def expect_fused(c, force=None):
    """the documented rule (csrc/attention_canon.h): the fused kernel exists where matmul's form rule takes the mfma form for
    both products"""
    return all(mc.expected_form(x, force) == pkg.MATMUL_MFMA for x in (_qk_case(c), _pv_case(c, None)))

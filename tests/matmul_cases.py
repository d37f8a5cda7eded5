"""Shared helpers for matmul (CSINN_OP_MATMUL): batched, both transposes, the reference's "dense" broadcast.

  all_cases()        deterministic single-op problems, seeded by crc32(name) and stratified: the smallest shapes at which a
                     64 x 64 tile kernel over 64-byte slabs of K can still go wrong (1, 2, around 32 and 64 in M and N; 1, 3,
                     around 32 and 64, and 130 in K; 1 .. 3 batches; four transposes; the broadcast; differing dim counts; odd
                     M K and K N with batches, which put a batch on an odd byte), zero points at the ends of the int8 range on
                     either operand and on the output, power-of-two and converter scales, binary16 inputs whose float32 sums
                     are exact, non-negative ones, and rows with inf, NaN and saturating sums
  chain_ref          numpy restatement of the reference (source/reference/matmul.c behind shl_ref_diso_callback_base):
                     dequantise both operands, ONE sequential float32 loop over k per output -- one fused
                     multiply-add per step, as the reference's build contracts it --, requantise
  exact_ref          the int8 mfma form's formula: S = sum (qa - za)(qb - zb) exactly, f = (float)S * fl(sa sb), requantise
  is_exact           the plan-time proof that the two agree for every input, restated
  assert_within_gate DESIGN's gate between them where the proof fails: every |difference| <= 1 LSB, at most
                     max(2, 2e-4 n) outputs differ
  layer_run          csinn_matmul_init + csinn_matmul through a front-end (layer mode)
  cabi_desc          the C ABI's descriptor of a case
  MatmulNet, attention_block(), classifier_tail()   small networks through the csinn session API (graph mode) with an oracle
                     replay
The genuine library's outputs for the cases live in tests/golden/matmul_cases.npz (make_matmul_golden.py).
"""
import ctypes as C
import math
import os
import zlib

import numpy as np

import pool_cases
from cases import pkg
from pool_cases import _q, assert_same, bits  # noqa: F401
from reduce_cases import _DEFAULT_NAN, _requantise

MS = NS = (1, 2, 31, 32, 33, 64, 65)
KS = (1, 3, 31, 32, 33, 63, 64, 65, 130)
BATCHES = (1, 2, 3)
OTHERS = (2, 31, 33)  # what a sweep over one of M, N draws the other from: the goldens stay small
TRANSPOSES = ((0, 0), (0, 1), (1, 0), (1, 1))
ZPS = (-128, 0, 5, 127)
Q_POW2 = (_q(2.0 ** -4, 0), _q(2.0 ** -6, 0))     # (scales of) mat0 and mat1 under which the proof holds up to K = 130
Q_CONV = (_q(0.0473, 0), _q(0.0219, 0))           # converter scales: the proof fails for every K
FMA_WITNESSES = (42, 116, 219)
NAN_P, NAN_N, INF_P, INF_N = 0x7E00, 0xFE00, 0x7C00, 0xFC00


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ------------------------------------------------------------------------------------ cases
def _shapes(batch_a, batch_b, m, n, k, ta, tb):
    return tuple(batch_a) + ((k, m) if ta else (m, k)), tuple(batch_b) + ((n, k) if tb else (k, n))


def out_record(k, a_q, b_q, name):
    """an int8 output record under which the outputs of random data spread over the int8 range instead of saturating: the
    scale follows the spread of the sums (no power of two), the zero point is seeded from the strata"""
    spread = 74.0 * 74.0 * math.sqrt(k) * a_q[0] * b_q[0] / 40.0
    return _q(np.float32(spread), int(_rng("zp " + name).choice(ZPS)))


def _f16_data(rng, shape, kind):
    if kind == "exact":  # multiples of 2^-4 in [-4, 4]: products are multiples of 2^-8 below 16, 130 of them sum exactly
        return (rng.integers(-64, 65, shape) / 16.0).astype(np.float16)
    return rng.uniform(0.0, 2.0, shape).astype(np.float16)  # non-negative: no cancellation


def _add(out, name, dtype, m, n, k, batch_a=(), batch_b=None, ta=0, tb=0, regime="pow2", za=None, zb=None, zo=None,
         f16_kind="exact", a=None, b=None):
    full = "%s_%s" % (name, "f16" if dtype == "f16" else "i8")
    rng = _rng("matmul " + full)
    batch_b = batch_a if batch_b is None else batch_b
    sa, sb = _shapes(batch_a, batch_b, m, n, k, ta, tb)
    c = dict(name=full, dtype=dtype, trans_a=bool(ta), trans_b=bool(tb), m=m, n=n, k=k, regime=regime if dtype == "int8" else f16_kind)
    if dtype == "f16":
        c["a"] = _f16_data(rng, sa, f16_kind) if a is None else a
        c["b"] = _f16_data(rng, sb, f16_kind) if b is None else b
        c["a_q"] = c["b_q"] = c["out_q"] = _q(1.0, 0)
    else:
        c["a"], c["b"] = rng.integers(-128, 128, sa, dtype=np.int8), rng.integers(-128, 128, sb, dtype=np.int8)
        base = Q_POW2 if regime == "pow2" else Q_CONV
        za = int(rng.choice(ZPS)) if za is None else za
        zb = int(rng.choice(ZPS)) if zb is None else zb
        c["a_q"], c["b_q"] = _q(base[0][0], za), _q(base[1][0], zb)
        c["out_q"] = out_record(k, c["a_q"], c["b_q"], full)
        if zo is not None:
            c["out_q"] = _q(c["out_q"][0], zo)
    batches = int(np.prod(batch_a, dtype=np.int64))
    c["batches"] = batches
    c["out_shape"] = tuple(batch_a) + (m, n)
    out.append(c)


def _both(out, name, *args, **kw):
    for dtype in ("f16", "int8"):
        _add(out, name, dtype, *args, **kw)


def sweep_cases():
    """every M, every N and every K of the strata under two of the four transposes in turns, the other two extents, the batch count,
    the scale regime / binary16 stratum and the zero points drawn by the case's own seed"""
    out = []
    for which, values in (("m", MS), ("n", NS), ("k", KS)):
        for i, v in enumerate(values):
            for ta, tb in (TRANSPOSES[0::3], TRANSPOSES[1:3])[i % 2]:  # (none and both, or one of them: in turns)
                name = "%s%d_t%d%d" % (which, v, ta, tb)
                rng = _rng("sweep " + name)
                m = v if which == "m" else int(rng.choice(OTHERS))
                n = v if which == "n" else int(rng.choice(OTHERS))
                k = v if which == "k" else int(rng.choice(KS))
                nb = int(rng.choice(BATCHES))
                _both(out, name, m, n, k, batch_a=(nb,) if nb > 1 or rng.integers(2) else (), ta=ta, tb=tb,
                      regime=("pow2", "conv")[int(rng.integers(2))], f16_kind=("exact", "nonneg")[int(rng.integers(2))])
    return out


def batch_cases():
    out = []
    for nb in BATCHES:  # every batch count at a shape of more than one tile with ragged edges
        _both(out, "batches%d" % nb, 65, 33, 65, batch_a=(nb,), regime="conv", f16_kind="nonneg")
    # the "dense" broadcast: one mat1 for every batch of mat0, no transposes
    _both(out, "dense_2x33x65x31", 33, 31, 65, batch_a=(2,), batch_b=())
    _both(out, "dense_3x2x3x130", 2, 130 // 2, 3, batch_a=(3,), batch_b=(), regime="conv", f16_kind="nonneg")
    _both(out, "dense_3x64x64x64", 64, 64, 64, batch_a=(3,), batch_b=())
    # differing dim counts: [2, 3, M, K] x [K, N] (the broadcast again) and [6, M, K] x [2, 3, K, N]
    _both(out, "dims_2x3_by_none", 31, 33, 32, batch_a=(2, 3), batch_b=(), regime="conv", f16_kind="nonneg")
    _both(out, "dims_6_by_2x3", 9, 33, 63, batch_a=(6,), batch_b=(2, 3))
    _both(out, "dims_6_by_2x3_t11", 33, 9, 63, batch_a=(6,), batch_b=(2, 3), ta=1, tb=1, regime="conv")
    _both(out, "dims_1x1_by_1", 32, 32, 32, batch_a=(1, 1), batch_b=(1,))
    # odd M K and odd K N with batches: batch 1 of either operand starts on an odd byte, no 16-byte load stays aligned
    for ta, tb in TRANSPOSES:
        _both(out, "odd_3x33x5_t%d%d" % (ta, tb), 3, 5, 33, batch_a=(3,), ta=ta, tb=tb)
        _both(out, "odd_31x33x33_t%d%d" % (ta, tb), 31, 33, 33, batch_a=(2,), ta=ta, tb=tb, regime="conv", f16_kind="nonneg")
    return out


def record_cases():
    """zero points at -128, 0, 5 and 127 on either operand and on the output, in both scale regimes; and the three regimes at
    one ragged two-tile shape"""
    out = []
    for regime in ("pow2", "conv"):
        for za in ZPS:
            for zb in ZPS:
                zo = ZPS[(ZPS.index(za) + ZPS.index(zb)) % 4]
                _add(out, "zp_%s_%d_%d_%d" % (regime, za, zb, zo), "int8", 33, 34, 65, ta=za == 5, tb=zb == 5,
                     regime=regime, za=za, zb=zb, zo=zo)
    _add(out, "regime_pow2_k130", "int8", 64, 65, 130, regime="pow2")
    _add(out, "regime_conv_k3", "int8", 64, 65, 3, regime="conv")
    _add(out, "regime_conv_k130", "int8", 64, 65, 130, regime="conv")
    _add(out, "regime_conv_k130_t01", "int8", 65, 64, 130, batch_a=(2,), tb=1, regime="conv")
    # three seeds under which one output tells the reference's fused multiply-add from a rounded product followed by a rounded
    # sum (found by search: about one output in fifty thousand does)
    for seed in FMA_WITNESSES:
        _add(out, "fma_witness_%d" % seed, "int8", 33, 34, 65, regime="conv", za=5, zb=-128, zo=0)
    return out


def special_cases():
    """binary16 rows with a NaN of either sign, an infinity, inf + -inf and sums beyond the binary16 range (chain only: the
    mfma form's contract is about finite data).  A NaN sits in ONE operand, so that which one a product hands on is not in
    question"""
    out = []
    for ta, tb in ((0, 0), (1, 1)):
        m, n, k = 6, 5, 9
        rng = _rng("special %d%d" % (ta, tb))
        a = rng.uniform(0.5, 2.0, (m, k)).astype(np.float16)
        b = rng.uniform(0.5, 2.0, (k, n)).astype(np.float16)
        au = a.view(np.uint16)
        au[0, 4] = NAN_P
        au[1, 2] = INF_P
        au[2, 1], au[2, 7] = INF_P, INF_N  # inf + -inf: the default NaN, whose sign bit is set
        au[3, 8] = NAN_N
        a[4, :] = 60000.0                   # saturates: 0x7BFF
        a[5, :] = -60000.0
        _add(out, "special_t%d%d" % (ta, tb), "f16", m, n, k, ta=ta, tb=tb, f16_kind="special",
             a=np.ascontiguousarray(a.T) if ta else a, b=np.ascontiguousarray(b.T) if tb else b)
    return out


def all_cases():
    out = sweep_cases() + batch_cases() + record_cases() + special_cases()
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def case_id(case):
    return case["name"]


golden_key = case_id


def golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matmul_cases.npz")
    blob = np.load(path)
    return {k: blob[k] for k in blob.files}


# ------------------------------------------------------------------------------------ numpy restatements
def _operands(case, a=None, b=None):
    """(A as [batches, M, K], B as [batches or 1, K, N]) in the operands' own dtype"""
    a = case["a"] if a is None else a
    b = case["b"] if b is None else b
    a3 = a.reshape((-1,) + a.shape[-2:])
    b3 = b.reshape((-1,) + b.shape[-2:])
    if case["trans_a"]:
        a3 = a3.transpose(0, 2, 1)
    if case["trans_b"]:
        b3 = b3.transpose(0, 2, 1)
    assert b3.shape[0] in (a3.shape[0], 1) and a3.shape[2] == b3.shape[1]
    return a3, b3


def _fma32(x, y, acc):
    """RN_float32(x * y + acc) with ONE rounding, for float32 arrays: the product of two float32 is exact in float64; the sum is
    taken in float64 rounded TO ODD (the round-to-nearest sum, moved to its odd neighbour on the side of TwoSum's error term
    when it is inexact and even), which a final rounding to float32 turns into the correctly rounded result (53 >= 2 * 24 + 2)"""
    p = x.astype(np.float64) * y.astype(np.float64)
    c = np.broadcast_to(acc.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # TwoSum: s + err == p + c exactly
    with np.errstate(invalid="ignore"):
        inexact = np.isfinite(s) & (err != 0)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(inexact & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def _fma_x86(x, y, acc):
    """total += a * b as the reference's build (-O3 -mfma: the product and the sum contracted into one vfmadd) computes it.  A
    NaN result: the accumulator's NaN is handed on, else an operand's, else (inf * 0, inf - inf) the default NaN, whose sign bit
    is set.  (float32_to_float16_base keeps a NaN's sign; the cases put a NaN into one operand only.)"""
    r = _fma32(x, y, acc)
    bad = np.isnan(r)
    if bad.any():
        r = np.where(bad, np.where(np.isnan(acc), acc, np.where(np.isnan(x), x, np.where(np.isnan(y), y, _DEFAULT_NAN))), r)
    return r.astype(np.float32)


def chain_ref(case, a=None, b=None):
    """the reference's literal loop: total = 0; for k: total += a * b in float32, k ascending -- as its build compiles it, ONE
    fused multiply-add per step"""
    a3, b3 = _operands(case, a, b)
    with np.errstate(all="ignore"):
        fa = np.ascontiguousarray(pool_cases.dequantise(a3, case["dtype"], case["a_q"]), dtype=np.float32)
        fb = np.ascontiguousarray(pool_cases.dequantise(b3, case["dtype"], case["b_q"]), dtype=np.float32)
        acc = np.zeros((a3.shape[0], a3.shape[1], b3.shape[2]), np.float32)
        for k in range(a3.shape[2]):
            x, y = fa[:, :, k, None], fb[:, k, None, :]
            acc = _fma_x86(x, y, acc)
        out = _requantise(np.ascontiguousarray(acc, dtype=np.float32), case["dtype"], case["out_q"])
    return np.ascontiguousarray(out).reshape(case["out_shape"])


def exact_ref(case, a=None, b=None):
    """the int8 mfma form: S exact, f = fl((float)S * fl(sa sb)), sat8(rint(f / s_out) + zp_out)"""
    assert case["dtype"] == "int8"
    a3, b3 = _operands(case, a, b)
    s = np.matmul(a3.astype(np.int64) - case["a_q"][1], b3.astype(np.int64) - case["b_q"][1])
    mult = np.float32(case["a_q"][0]) * np.float32(case["b_q"][0])
    f = (s.astype(np.float32) * mult).astype(np.float32)
    return pool_cases.requantise(f, "int8", case["out_q"]).reshape(case["out_shape"])


def _odd_mantissa(s):
    """a float32 scale as m 2^e with m odd; None for zero, NaN and infinities"""
    s = float(np.float32(s))
    if not (abs(s) > 0.0) or math.isinf(s) or math.isnan(s):
        return None
    f, e = math.frexp(abs(s))
    m = int(f * (1 << 53))
    e -= 53
    while m % 2 == 0:
        m //= 2
        e += 1
    return m, e


def is_exact(case):
    """k Aa Ab ma mb < 2^24 (csrc/matmul_canon.h:mm_is_exact): every dequantised value, product and partial sum of the chain,
    and (float)S * mult, then are exact"""
    if case["dtype"] != "int8":
        return False
    (sa, za), (sb, zb) = case["a_q"], case["b_q"]
    ma, mb = _odd_mantissa(sa), _odd_mantissa(sb)
    if ma is None or mb is None or not (-128 <= za <= 127 and -128 <= zb <= 127):
        return False
    (ma, ea), (mb, eb) = ma, mb
    if ea < -120 or eb < -120 or ea + eb < -120 or ea > 60 or eb > 60 or ea + eb > 60:
        return False
    aa, ab = max(127 - za, za + 128), max(127 - zb, zb + 128)
    return case["k"] * aa * ab * ma * mb < (1 << 24)


def gate_report(got, want):
    """(largest |difference| in LSB, number of differing outputs, how many may differ)"""
    d = np.abs(got.astype(np.int32).ravel() - want.astype(np.int32).ravel())
    return int(d.max(initial=0)), int(np.count_nonzero(d)), max(2, int(2e-4 * d.size))


def assert_within_gate(got, want, what):
    worst, differing, allowed = gate_report(got, want)
    assert worst <= 1 and differing <= allowed, "%s: %d outputs differ (allowed %d), the largest by %d LSB" % (what, differing, allowed, worst)


def assert_f16_gate(got, want, what):
    """the project's binary16 gate: |g - w| <= 1e-3 max(|w|, 1e-3)"""
    g, w = got.astype(np.float64).ravel(), want.astype(np.float64).ravel()
    bad = np.flatnonzero(~(np.abs(g - w) <= 1e-3 * np.maximum(np.abs(w), 1e-3)))
    assert bad.size == 0, "%s: %d outputs outside 1e-3, first at %d: got %r want %r" % (what, bad.size, bad[0], g[bad[0]], w[bad[0]])


def expected_form(case, force=None):
    """the documented form rule (csrc/matmul_canon.h:mm_form) for the dense tensors of a case"""
    if force == "chain":
        return pkg.MATMUL_CHAIN
    if case["dtype"] == "int8" and case["k"] > pkg.MATMUL_MFMA_MAX_K:
        return pkg.MATMUL_CHAIN
    if force == "mfma":
        return pkg.MATMUL_MFMA
    small = case["k"] < 64 and case["batches"] * case["m"] * case["n"] <= 65536  # less than one slab of k, one go of the chip's lanes
    return pkg.MATMUL_CHAIN if small else pkg.MATMUL_MFMA


def cabi_desc(case):
    return pkg.matmul_desc(pkg.SHL_I8 if case["dtype"] == "int8" else pkg.SHL_F16, case["a"].shape, case["b"].shape,
                           case["trans_a"], case["trans_b"], case["a_q"], case["b_q"], case["out_q"])


# ------------------------------------------------------------------------------------ through csinn_*
def _tensor_layout(ndim):
    return {1: pkg.LAYOUT_N, 2: pkg.LAYOUT_NC, 4: pkg.LAYOUT_NCHW}.get(ndim, pkg.LAYOUT_NCHW)


def layer_run(fe, api, case, device=None, poison=None, out_shape=None, perf=None, b_const=False, **kw):
    """layer mode through csinn_matmul (+ _init).  device: a cases.HipDevice -- all three tensors then are DMABUF tensors in
    HBM.  Returns the output, or (status, output) when `poison` (a byte the output is pre-filled with) is given.  kw: trans_a /
    trans_b overrides (refusal tests).  perf: a callable (callback block, mat0, mat1, output, params) run between init and exec"""
    keep = pkg.Keep()
    sess = pkg.layer_session(fe, api, keep)
    dt = pkg.DTYPE_INT8 if case["dtype"] == "int8" else pkg.DTYPE_FLOAT16
    a, b = case["a"], case["b"]
    o = np.zeros(out_shape or case["out_shape"], dtype=a.dtype)
    o.view(np.uint8)[...] = poison if poison is not None else 0
    allocs = []

    def place(arr):
        if device is None:
            return None
        p = device.alloc(arr.nbytes)
        device.upload(p, arr)
        allocs.append(p)
        return p
    t_a = pkg.make_tensor(fe, keep, a.shape, dt, _tensor_layout(a.ndim), data=a, scales=(case["a_q"][0],), zps=(case["a_q"][1],),
                          name=b"mat0", sess=sess, device_ptr=place(a))
    t_b = pkg.make_tensor(fe, keep, b.shape, dt, _tensor_layout(b.ndim), data=b, scales=(case["b_q"][0],), zps=(case["b_q"][1],),
                          name=b"mat1", sess=sess, device_ptr=place(b), is_const=1 if b_const else 0)
    p_out = place(o)
    t_o = pkg.make_tensor(fe, keep, o.shape, dt, _tensor_layout(o.ndim), data=o, scales=(case["out_q"][0],), zps=(case["out_q"][1],),
                          name=b"out", sess=sess, device_ptr=p_out)
    params = pkg.matmul_params(fe, keep, api, pkg.LAYOUT_NCHW, kw.get("trans_a", case["trans_a"]), kw.get("trans_b", case["trans_b"]), sess)
    args = (t_a, t_b, t_o, params)
    rc = fe.csinn_matmul_init(*args)
    if rc == pkg.CSINN_TRUE and perf is not None:
        perf(C.cast(params, C.POINTER(pkg.ParamsBase)).contents.cb, *args)
    if rc == pkg.CSINN_TRUE:
        rc = fe.csinn_matmul(*args)
    if device is not None:
        o = device.download(p_out, o.shape, o.dtype)
        for p in allocs:
            device.free(p)
    if poison is not None:
        return rc, o
    if rc != pkg.CSINN_TRUE:
        raise pkg.MI355XError("csinn_matmul returned %d" % rc)
    return o


# ------------------------------------------------------------------------------------ networks around matmul
import cases  # noqa: E402
import eltwise_cases  # noqa: E402
import move_cases  # noqa: E402
import tail  # noqa: E402


class MatmulNet(move_cases.MoveNet):
    """A small network given as a list of layers over named tensors (move_cases.MoveNet), run two ways: through the csinn
    session API in graph mode, and as an oracle chain -- convolutions through the C oracle, relu, add and softmax through the C
    oracle's restatements, transpose / reshape / flatten and mul through their numpy restatements, matmul through chain_ref.
    cut=True builds THE SAME GRAPH WITHOUT ITS MATMUL LAYERS: each one's activation inputs become graph outputs and its output
    a graph input, so that the fusion planner's counts can be compared (that graph is built, never run).

    layers: (kind, name, input or tuple of inputs, output, info) with MoveNet's kinds and matmul (info: trans_a, trans_b; a
    second input named in `consts` is a constant tensor), mulc (info: const, a one-element constant), softmax (info: axis),
    add.  consts: name -> (array, record)."""

    def __init__(self, dtype, layout, seed, in_name, tensors, layers, outputs, consts, cut=False, x_grid=(-32, 32, 1.0 / 16)):
        super().__init__(dtype, layout, seed, in_name, tensors, layers, outputs, cut=cut)
        self.consts, self.x_grid = consts, x_grid  # binary16 inputs: integers lo .. hi times a step

    def input(self, k):
        rng = np.random.default_rng(1300 + k)
        shape = self.shape(self.in_name)
        if self.dtype == "int8":
            return rng.integers(-100, 100, shape, dtype=np.int8)
        lo, hi, step = self.x_grid
        return (rng.integers(lo, hi + 1, shape) * step).astype(np.float16)  # few mantissa bits: the first sums are exact

    def crec(self, name):
        return self.consts[name][1] if self.dtype == "int8" else _q(1.0, 0)

    def _matmul_case(self, srcs, dst, info, a=None, b=None):
        b_q = self.crec(srcs[1]) if srcs[1] in self.consts else self.rec(srcs[1])
        b = self.consts[srcs[1]][0] if srcs[1] in self.consts else b
        return dict(dtype=self.dtype, a=a, b=b, a_q=self.rec(srcs[0]), b_q=b_q, out_q=self.rec(dst), out_shape=self.shape(dst),
                    trans_a=bool(info.get("trans_a")), trans_b=bool(info.get("trans_b")))

    def oracle(self, x):
        env = {self.in_name: x}
        form = "ref" if self.dtype == "int8" else "f16"
        for kind, name, src, dst, info in self.layers:
            srcs = src if isinstance(src, tuple) else (src,)
            a = env[srcs[0]]
            if kind == "conv":
                case = dict(self.cv[name])
                case["input"] = np.ascontiguousarray(a).reshape(case["in_shape"])
                env[dst] = cases.oracle_run(case, form).reshape(self.shape(dst))
            elif kind in self.MOVES:
                env[dst] = move_cases.move_numpy(self._move_case(kind, src, dst, info, a))
            elif kind == "matmul":
                env[dst] = chain_ref(self._matmul_case(srcs, dst, info, a, env.get(srcs[1])))
            elif kind == "mulc":
                y, y_q = self.consts[info["const"]][0], self.crec(info["const"])
                env[dst] = eltwise_cases.eltwise_numpy(dict(op="mul", dtype=self.dtype, x=a, y=y, in_q=self.rec(src), in1_q=y_q,
                                                            out_q=self.rec(dst)))
            elif kind == "add":
                env[dst] = tail.siso_oracle(dict(kind="add", x=a, y=env[srcs[1]], dtype=self.dtype, layout=self.layout, axis=1,
                                                 in_q=self.rec(srcs[0]), in1_q=self.rec(srcs[1]), out_q=self.rec(dst)))
            else:
                env[dst] = tail.siso_oracle(dict(kind=kind, x=a, dtype=self.dtype, layout=self.layout, axis=info.get("axis", 1),
                                                 in_q=self.rec(src), out_q=self.rec(dst)))
        return env

    def build(self, fe, api):
        keep = pkg.Keep()
        sess = fe.csinn_alloc_session()
        sc = sess.contents
        int8 = self.dtype == "int8"
        dt = pkg.DTYPE_INT8 if int8 else pkg.DTYPE_FLOAT16
        sc.base_api, sc.base_run_mode, sc.base_dtype = api, pkg.RM_CPU_GRAPH, dt
        sc.base_quant_type = pkg.QUANT_INT8_ASYM_W_SYM if int8 else pkg.QUANT_FLOAT16
        sc.debug_level = 0
        fe.csinn_session_init(sess)
        nhwc = self.layout == "NHWC"
        act_l = pkg.LAYOUT_NHWC if nhwc else pkg.LAYOUT_NCHW

        def T(dims, rec, name, data=None, const=0, layout=act_l, dtype=dt, scales=None):
            return pkg.make_tensor(fe, keep, dims, dtype, layout, data=data, is_const=const, name=name, sess=sess,
                                   scales=scales if scales is not None else (rec[0],), zps=(rec[1] if rec else 0,))

        def A(name):
            shape = self.shape(name)
            return T(shape, self.rec(name), name.encode(), layout={1: pkg.LAYOUT_N, 2: pkg.LAYOUT_NC}.get(len(shape), act_l))

        def K(name):  # a constant operand
            data = self.consts[name][0]
            return T(data.shape, self.crec(name), name.encode(), data, 1, {1: pkg.LAYOUT_N, 2: pkg.LAYOUT_NC}.get(data.ndim, act_l))
        env = {self.in_name: A(self.in_name)}
        ops, inputs, outputs = [], [env[self.in_name]], []
        cut_away = {self.in_name}
        for kind, name, src, dst, info in self.layers:
            srcs = src if isinstance(src, tuple) else (src,)
            env[dst] = A(dst)
            nm = name.encode()
            if kind == "matmul" and self.cut:
                for s in srcs:
                    if s not in self.consts and s not in cut_away and all(env[s] is not t for t in outputs):
                        outputs.append(env[s])
                inputs.append(env[dst])
                cut_away.add(dst)
            elif kind == "conv":
                case = self.cv[name]
                t_w = T(case["w_shape"], None, nm + b"_w", case["kernel"], 1, pkg.LAYOUT_OHWI if nhwc else pkg.LAYOUT_OIHW,
                        scales=tuple(case["k_scale"]))
                t_b = T((case["co"],), None, nm + b"_b", case["bias"], 1, pkg.LAYOUT_O, pkg.DTYPE_INT32 if int8 else dt,
                        scales=tuple(case["b_scale"]))
                p = pkg.conv_params(fe, keep, api, act_l, case["stride"], case["pad"], case["dilation"], case["group"], 0, sess, nm)
                ops.append(("csinn_conv2d" + ("_relu" if case["act"] else ""), (env[src], env[dst], t_w, t_b, p)))
            elif kind in self.MOVES:
                p = move_cases.op_params(fe, keep, api, self._move_case(kind, src, dst, info), sess, layout=act_l)
                ops.append(("csinn_" + kind, (env[src], env[dst], p)))
            elif kind == "matmul":
                second = K(srcs[1]) if srcs[1] in self.consts else env[srcs[1]]
                p = pkg.matmul_params(fe, keep, api, act_l, info.get("trans_a"), info.get("trans_b"), sess, nm)
                ops.append(("csinn_matmul", (env[srcs[0]], second, env[dst], p)))
            elif kind == "mulc":
                ops.append(("csinn_mul", (env[src], K(info["const"]), env[dst], pkg.siso_params(fe, keep, api, "mul", act_l, 1, sess, nm))))
            elif kind == "add":
                ops.append(("csinn_add", (env[srcs[0]], env[srcs[1]], env[dst], pkg.siso_params(fe, keep, api, "add", act_l, 1, sess, nm))))
            else:
                ops.append(("csinn_" + kind, (env[src], env[dst], pkg.siso_params(fe, keep, api, kind, act_l, info.get("axis", 1), sess, nm))))
        outputs.extend(env[o] for o in self.outputs if o not in cut_away and all(env[o] is not t for t in outputs))
        fe.csinn_set_input_number(len(inputs), sess)
        fe.csinn_set_output_number(len(outputs), sess)
        for stem, args in ops:
            assert getattr(fe, stem + "_init")(*args) == pkg.CSINN_TRUE, stem
        for i, t in enumerate(inputs):
            fe.csinn_set_tensor_entry(t, sess)
            fe.csinn_set_input(i, t, sess)
        for stem, args in ops:
            assert getattr(fe, stem)(*args) == pkg.CSINN_TRUE, stem
        for i, t in enumerate(outputs):
            fe.csinn_set_output(i, t, sess)
        rc = fe.csinn_session_setup(sess)
        assert rc == pkg.CSINN_TRUE or getattr(fe, "kind", "") == "reference"
        self._keep, self._sess, self.layer_count = keep, sess, len(ops)
        return sess


def _weights(rng, shape, dtype, grid=(-16, 16, 1.0 / 64)):
    if dtype == "int8":
        return rng.integers(-128, 128, shape, dtype=np.int8)
    lo, hi, step = grid
    return (rng.integers(lo, hi + 1, shape) * step).astype(np.float16)  # (multiples of 2^-6 in [-0.25, 0.25] unless told)


def attention_block(dtype="int8", layout="NCHW", cut=False):
    """one attention block on S = 17 tokens of C = 64 channels, 2 heads of 32: q, k, v = x Wq, x Wk, x Wv (three matmuls against
    constants) -> reshape to [1, 17, 2, 32] -> transpose to heads [1, 2, 17, 32] -> s = q k^T (matmul, trans_b, two
    activations) -> mul by a constant 1 / sqrt(32) -> softmax over the last axis -> o = p v (matmul) -> transpose and reshape
    back -> o Wo (matmul against a constant) -> add the residual x.  int8: every matmul's records are powers of two inside the
    plan-time proof, so the mfma form equals chain_ref bit for bit.  binary16: the mfma form adds in another order than
    chain_ref, and a softmax or a cancelling sum behind a one-ulp difference would carry it past 1e-3, so the data keep the
    difference out of where it would grow: x is a multiple of 1/4 in [0, 2] and Wq, Wk are -1/8, 0 or 1/8, so q, k (multiples of
    2^-5 below 16) are exact in binary16 and every partial sum of q k^T (a multiple of 2^-10 below 2^13) is exact in float32 --
    the scores and p are the same bits in either form; Wv and Wo are 0, 1/16 or 1/8, so everything behind the softmax is a sum
    of non-negative terms"""
    q = lambda s, z: _q(2.0 ** s, z)
    rng = np.random.default_rng(71)
    s, c, h, hd = 17, 64, 2, 32
    flat, split, heads = (1, s, c), (1, s, h, hd), (1, h, s, hd)
    t = {"x": (flat, q(-4, -5)), "out": (flat, q(-3, 7)), "proj": (flat, q(-5, 3)),
         "s": ((1, h, s, s), q(-1, 5)), "sc": ((1, h, s, s), q(-3, 5)), "p": ((1, h, s, s), _q(1.0 / 256, -128)),
         "oh": (heads, q(-4, 3)), "os": (split, q(-4, 3)), "o": (flat, q(-4, 3))}
    for n, zp in (("q", -3), ("k", 0), ("v", 3)):
        t[n] = (flat, q(-4, zp))
        t[n + "s"] = (split, q(-4, zp))
        t[n + "h"] = (heads, q(-4, zp))
    signed, positive = (-1, 1, 1.0 / 8), (0, 2, 1.0 / 16)
    consts = {"Wq": (_weights(rng, (c, c), dtype, signed), q(-10, 0)), "Wk": (_weights(rng, (c, c), dtype, signed), q(-10, 5)),
              "Wv": (_weights(rng, (c, c), dtype, positive), q(-10, 0)), "Wo": (_weights(rng, (c, c), dtype, positive), q(-10, -128)),
              "scale": (np.array([90], np.int8) if dtype == "int8" else np.array([0.17578125], np.float16), q(-9, 0))}
    L = []
    for n in "qkv":
        L += [("matmul", n, ("x", "W" + n), n, {}),
              ("reshape", n + "_split", n, n + "s", {}),
              ("transpose", n + "_heads", n + "s", n + "h", dict(perm=(0, 2, 1, 3)))]
    L += [("matmul", "qk", ("qh", "kh"), "s", dict(trans_b=True)),
          ("mulc", "scaled", "s", "sc", dict(const="scale")),
          ("softmax", "softmax", "sc", "p", dict(axis=3)),
          ("matmul", "pv", ("p", "vh"), "oh", {}),
          ("transpose", "o_tokens", "oh", "os", dict(perm=(0, 2, 1, 3))),
          ("reshape", "o_merge", "os", "o", {}),
          ("matmul", "proj", ("o", "Wo"), "proj", {}),
          ("add", "residual", ("proj", "x"), "out", {})]
    return MatmulNet(dtype, layout, 73, "x", t, L, ["out", "p"], consts, cut=cut, x_grid=(0, 8, 1.0 / 4))


def classifier_tail(dtype="int8", layout="NHWC", cut=False, classes=24):
    """8x8x16 -> conv1x1 (8) + a relu LAYER (which a session folds) -> flatten to [1, 512] -> matmul against a constant
    [512, classes]: a model whose classifier is exported as MatMul (M = 1: the default rule takes the chain)"""
    q = lambda s, z: _q(2.0 ** s, z)
    rng = np.random.default_rng(79)
    act = lambda ch: (1, 8, 8, ch) if layout == "NHWC" else (1, ch, 8, 8)
    t = {"data": (act(16), q(-4, -5)), "c1c": (act(8), q(-3, -100)), "c1": (act(8), q(-3, -100)), "flat": ((1, 512), q(-3, -100)),
         "logits": ((1, classes), q(-3, -11))}
    consts = {"W": (_weights(rng, (512, classes), dtype), q(-10, 0))}
    L = [("conv", "c1", "data", "c1c", dict(act=0)),
         ("relu", "c1_relu", "c1c", "c1", {}),
         ("flatten", "flat", "c1", "flat", {}),
         ("matmul", "classifier", ("flat", "W"), "logits", {})]
    return MatmulNet(dtype, layout, 83, "data", t, L, ["logits"], consts, cut=cut)


NETS = {"attention_block": attention_block, "classifier_tail": classifier_tail}
CUT_LAYERS = {"attention_block": 6, "classifier_tail": 1}

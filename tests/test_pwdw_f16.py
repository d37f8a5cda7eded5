"""The binary16 NCHW pointwise + depthwise pair kernel (csrc/pwdw_f16_nchw.hip), checked LAYER BY LAYER.

Its pointwise phase adds the K parts in another fp32 order than the stand-alone pointwise kernel, so the fused output cannot be
compared bit for bit with two stand-alone launches, and the intermediate tensor never leaves the chip.  It is read back from the
production kernel as it ships with one-hot depthwise PROBES: nine depthwise plans with the real layer's shape, stride and pads,
weight binary16 1.0 at one tap (zero elsewhere), bias 0, no activation.  The depthwise phase sums in fp32 from +0, a zero weight
gives a +-0 product, 1.0 * m is exact and a binary16 m rounds to itself, so probe t writes out[n, c, oy, ox] = mid[n, c,
oy * s - pt + ky, ox * s - pl + kx] wherever that position lies in the map.  The kernel's choice of geometry (rows per workgroup,
tiles, K parts, template instance) depends on shapes only: a probe launch runs the real launch's pointwise phase on the same data.

  L0  the pair runs fused (a pair that silently took two launches would test nothing);
  L1  the probed intermediate against the oracle's pointwise layer: 1e-3 relative (golden_util.compare_f16_tol), the bar of every
      stand-alone binary16 layer;
  L2  the fused output against the oracle's depthwise layer AND the stand-alone depthwise kernel fed that intermediate: bit for bit
      (+0 == -0).  Positions no probe saw are NaN, so L2 also proves that the outputs read nothing else;
  L3  two launches give the same bytes.
Every output buffer is filled with 0xFF bytes (binary16 NaN) before a launch: an output the kernel never writes fails.
SHL_MI355X_PWDW_F16_ROWS (rows per workgroup, read per call) forces multi-row workgroups; SHL_FUZZ_N seeded random pairs (default 8).
"""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import golden_util
import tail
from cases import pkg

ENOTSUP = -3
F16_NAN = 0x7E00


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    opt.shl_mi355x_registry_get.restype = C.c_void_p
    opt.shl_mi355x_registry_get.argtypes = [C.c_void_p]
    return fe, hip, opt, cases.HipDevice(hip)


def make_pwdw_f16(i, c, co, h, w, stride=1, pad=(1, 1, 1, 1), n=1, acts=(1, 1)):
    """test_fusion.make_pwdw in binary16 NCHW, non-square maps and independent pads"""
    pw = cases.make_case(1700 + i, layout=cases.NCHW, dtype="f16", n=n, h=h, w=w, c=c, co=co, k=(1, 1), pad=(0, 0, 0, 0),
                         act=acts[0])
    dw = cases.make_case(1750 + i, layout=cases.NCHW, dtype="f16", n=n, h=h, w=w, c=co, depthwise=True, stride=(stride, stride),
                         pad=tuple(pad), act=acts[1])
    return pw, dw


def plan_of(gpu, case, keep):
    """the plan csinn_<conv>_init made for `case` (the stand-alone layer runs once on the way); -> (plan, output)"""
    fe, hip, opt, dev = gpu
    out = cases.csinn_run(fe, pkg.API_MI355X, case, device=dev, keep_params=keep)
    return opt.shl_mi355x_registry_get(keep[-1][0]), out


def one_hot_probes(gpu, dw, keep):
    """nine depthwise plans with dw's geometry: weight 1.0 at tap t = 3 ky + kx in every channel, bias 0, no activation"""
    plans = []
    for t in range(9):
        k = np.zeros(dw["w_shape"], dtype=np.float16)
        k.reshape(-1, 9)[:, t] = 1.0
        plans.append(plan_of(gpu, dict(dw, kernel=k, bias=np.zeros_like(dw["bias"]), act=0), keep)[0])
    return plans


def read_set(dw):
    """(H, W) mask of the intermediate positions that some output of the depthwise layer reads"""
    (sh, sw), (pt, pl) = dw["stride"], dw["pad"][:2]
    rows = (np.arange(dw["ho"])[:, None] * sh - pt + np.arange(3)[None, :]).ravel()
    cols = (np.arange(dw["wo"])[:, None] * sw - pl + np.arange(3)[None, :]).ravel()
    r = np.zeros(dw["h"], bool)
    c = np.zeros(dw["w"], bool)
    r[rows[(rows >= 0) & (rows < dw["h"])]] = True
    c[cols[(cols >= 0) & (cols < dw["w"])]] = True
    return r[:, None] & c[None, :]


def launch(gpu, plan_pw, plan_dw, d_in, shape, n):
    """one pwdw_forward into a buffer of 0xFF bytes -> the output's binary16 words"""
    fe, hip, opt, dev = gpu
    nbytes = int(np.prod(shape)) * 2
    d_out = dev.alloc(nbytes)
    hip.shl_mi355x_memset(d_out, 0xFF, nbytes, None)
    pkg.check(hip.shl_mi355x_pwdw_forward(plan_pw, plan_dw, d_in, d_out, n, None), hip, "pwdw_forward")
    got = dev.download(d_out, shape, np.uint16)
    dev.free(d_out)
    return got


def plus_zero(u16):
    return np.where(u16 == 0x8000, np.uint16(0), u16)


def fused_intermediate(gpu, plan_pw, probes, pw, dw, d_in):
    """The pair's binary16 intermediate as its pointwise phase computed it, read through the nine probes -> (mid as float16
    [N, Co, H, W] with NaN where no output reads, (H, W) mask of the observed positions).  A position seen by several probes
    (halo rows are recomputed by the neighbouring workgroups, in other 4-pixel finishing blocks) must be the same word each time."""
    n, co, H, W = pw["n"], pw["co"], pw["h"], pw["w"]
    (sh, sw), (pt, pl) = dw["stride"], dw["pad"][:2]
    shape = (n, co, dw["ho"], dw["wo"])
    mid = np.full((n, co, H, W), F16_NAN, np.uint16)
    seen = np.zeros((H, W), bool)
    for t, probe in enumerate(probes):
        ky, kx = divmod(t, 3)
        got = launch(gpu, plan_pw, probe, d_in, shape, n)
        ys = np.arange(dw["ho"]) * sh - pt + ky
        xs = np.arange(dw["wo"]) * sw - pl + kx
        ry, rx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
        outside = ~(ry[:, None] & rx[None, :])
        # an output whose tap t lies in the padding sums nothing: +0 (bias 0), and it must have been written
        assert (plus_zero(got[:, :, outside]) == 0).all(), "probe %d: an output whose tap is padding is not +0 (%d words)" % (
            t, int((plus_zero(got[:, :, outside]) != 0).sum()))
        obs = got[:, :, ry][:, :, :, rx]
        assert not np.isnan(obs.view(np.float16)).any(), "probe %d: %d outputs unwritten or NaN" % (
            t, int(np.isnan(obs.view(np.float16)).sum()))
        ty, tx = ys[ry][:, None], xs[rx][None, :]
        again = seen[ty, tx]
        prev = mid[:, :, ty, tx]
        differ = (plus_zero(prev) != plus_zero(obs)) & again
        assert not differ.any(), "probe %d: %d intermediate words differ from another probe's view of the same position" % (
            t, int(differ.sum()))
        mid[:, :, ty, tx] = obs
        seen[ty, tx] = True
    want = read_set(dw)
    assert np.array_equal(seen, want), "observed %d intermediate positions, the outputs read %d" % (int(seen.sum()), int(want.sum()))
    return mid.view(np.float16), seen


def l1_worst(mid, want, seen):
    """worst relative error of the probed intermediate on values that are not small against the tensor"""
    g, e = mid[:, :, seen].astype(np.float64), want[:, :, seen].astype(np.float64)
    big = np.abs(e) >= 2.0 ** -8 * np.abs(e).max()
    return float((np.abs(g - e)[big] / np.abs(e)[big]).max()) if big.any() else 0.0


def check_layers(gpu, plan_pw, plan_dw, pw, dw, d_in, what, fused_out=None, keep=None):
    """L0 - L3 for one pair (with the chain's output given, L3 is the relaunch against it); -> L1 worst relative error"""
    fe, hip, opt, dev = gpu
    n = pw["n"]
    assert hip.shl_mi355x_pwdw_fusable(plan_pw, plan_dw, n) == 1, "%s: the pair does not run fused" % what       # L0
    shape = (n, pw["co"], dw["ho"], dw["wo"])
    got = launch(gpu, plan_pw, plan_dw, d_in, shape, n)
    if fused_out is not None:
        assert np.array_equal(plus_zero(got), plus_zero(np.asarray(fused_out).view(np.uint16))), "%s: a relaunch differs from the chain's output" % what
    else:
        assert np.array_equal(got, launch(gpu, plan_pw, plan_dw, d_in, shape, n)), "%s: two launches differ" % what  # L3
    own = [] if keep is None else keep
    probes = one_hot_probes(gpu, dw, own)
    mid, seen = fused_intermediate(gpu, plan_pw, probes, pw, dw, d_in)
    want_mid = cases.oracle_run(pw, "f16")                                                                        # L1
    golden_util.compare_f16_tol(mid[:, :, seen], want_mid[:, :, seen], "%s: L1 fused pointwise phase vs oracle" % what)
    dw_mid = dict(dw, input=np.ascontiguousarray(mid))                                                             # L2
    want = cases.oracle_run(dw_mid, "f16").view(np.uint16)
    bad = plus_zero(got) != plus_zero(want)
    assert not bad.any(), "%s: L2 fused output vs oracle depthwise fed the probed intermediate: %d of %d words differ" % (
        what, int(bad.sum()), got.size)
    alone = cases.csinn_run(fe, pkg.API_MI355X, dw_mid, device=dev, keep_params=own).view(np.uint16)
    bad = plus_zero(got) != plus_zero(alone)
    assert not bad.any(), "%s: L2 fused output vs stand-alone depthwise kernel on the probed intermediate: %d words differ" % (
        what, int(bad.sum()))
    if keep is None:
        for p, _ in own:
            opt.shl_mi355x_release_params(p)
    return l1_worst(mid, want_mid, seen)


def run_pair(gpu, pw, dw, what):
    """plans of both layers, the pair's input in HBM, L0 - L3; -> L1 worst relative error"""
    fe, hip, opt, dev = gpu
    keep = []
    plan_pw, mid_alone = plan_of(gpu, pw, keep)
    plan_dw, _ = plan_of(gpu, dict(dw, input=mid_alone), keep)
    d_in = dev.alloc(pw["input"].nbytes)
    dev.upload(d_in, pw["input"])
    try:
        return check_layers(gpu, plan_pw, plan_dw, pw, dw, d_in, what, keep=keep)
    finally:
        dev.free(d_in)
        for p, _ in keep:
            opt.shl_mi355x_release_params(p)


# (C, Co, H, W, depthwise stride, pads t, l, b, r, batch, activations pointwise / depthwise); comment: what the pair reaches
F16_PAIRS = [
    dict(c=32, co=64, h=16, w=16, stride=2, acts=(1, 1)),                            # one K part, NSW = 2 instance
    dict(c=64, co=128, h=12, w=12, acts=(2, 0)),                                     # one K part, NSW = 4
    dict(c=128, co=128, h=9, w=9, stride=2, acts=(0, 1)),                            # 2 K parts
    dict(c=256, co=64, h=7, w=7, acts=(1, 0)),                                       # 4 K parts
    dict(c=512, co=512, h=14, w=14, acts=(1, 2)),                                    # 8 K parts
    dict(c=512, co=1024, h=7, w=7, acts=(0, 2)),                                     # the widest slice count
    dict(c=512, co=96, h=14, w=14, stride=2, n=2, acts=(2, 1)),                      # stride 2, batch 2, Co not a power of two
    dict(c=32, co=32, h=33, w=33, n=3, acts=(1, 1)),                                 # sliding-window depthwise path (Wo > 16)
    dict(c=64, co=64, h=8, w=8, stride=2, pad=(0, 0, 1, 1), acts=(1, 1)),            # TF-style stride-2 pads
    dict(c=64, co=32, h=5, w=5, pad=(2, 2, 2, 2), acts=(0, 0)),                      # pad 2: windows mostly padding
    dict(c=128, co=160, h=13, w=17, pad=(1, 0, 2, 1), n=2, acts=(2, 2)),             # asymmetric pads, non-square map
    dict(c=32, co=224, h=1, w=1, n=4, acts=(1, 0)),                                  # 1 x 1 map, batch 4: tensor-end pieces
    dict(c=256, co=32, h=10, w=10, stride=2, pad=(0, 0, 0, 0), acts=(0, 1)),         # pad 0, stride 2: unread last row
    dict(c=64, co=32, h=5, w=6, pad=(1, 1, 3, 3), acts=(1, 2)),                      # bottom / right pad 3: rows in the padding
    dict(c=128, co=64, h=6, w=21, stride=2, pad=(0, 1, 1, 0), n=3, acts=(2, 0)),     # rows not 8-element multiples
    dict(c=512, co=512, h=14, w=14, n=8, acts=(1, 1)),                               # multi-row workgroups by the rule (7 rows)
    dict(c=128, co=256, h=28, w=28, n=4, acts=(1, 1)),                               # multi-row workgroups by the rule (4 rows)
]
# forced rows per workgroup (SHL_MI355X_PWDW_F16_ROWS) on pairs above: (pair, rows)
F16_FORCED = [(0, 3), (1, 5), (6, 2), (7, 2), (7, 4), (10, 4), (12, 3), (13, 3), (14, 2)]


def pair_id(p):
    pad = p.get("pad", (1, 1, 1, 1))
    return "c%d_co%d_%dx%d_s%d_p%s_n%d_a%d%d" % (p["c"], p["co"], p["h"], p["w"], p.get("stride", 1), "".join(map(str, pad)),
                                               p.get("n", 1), *p.get("acts", (1, 1)))


def ragged(i, rows):
    p = F16_PAIRS[i]
    pad, s = p.get("pad", (1, 1, 1, 1)), p.get("stride", 1)
    ho = cases.out_size(p["h"], 3, s, pad[0], pad[2], 1)
    return ho % rows != 0


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(F16_PAIRS)), ids=[pair_id(p) for p in F16_PAIRS])
def test_fp16_pair_layer_by_layer(gpu, i, monkeypatch):
    monkeypatch.delenv("SHL_MI355X_PWDW_F16_ROWS", raising=False)
    pw, dw = make_pwdw_f16(i, **F16_PAIRS[i])
    worst = run_pair(gpu, pw, dw, pair_id(F16_PAIRS[i]))
    print("%s: ran fused, L1 worst relative error %.2e" % (pair_id(F16_PAIRS[i]), worst))


@pytest.mark.gpu
@pytest.mark.parametrize("i,rows", F16_FORCED, ids=["%s_rows%d" % (pair_id(F16_PAIRS[i]), r) for i, r in F16_FORCED])
def test_fp16_pair_with_forced_rows_per_workgroup(gpu, i, rows, monkeypatch):
    monkeypatch.setenv("SHL_MI355X_PWDW_F16_ROWS", str(rows))
    pw, dw = make_pwdw_f16(i, **F16_PAIRS[i])
    worst = run_pair(gpu, pw, dw, "%s rows %d" % (pair_id(F16_PAIRS[i]), rows))
    print("%s: ran fused with %d rows per workgroup%s, L1 worst relative error %.2e" % (
        pair_id(F16_PAIRS[i]), rows, " (ragged last row block)" if ragged(i, rows) else "", worst))


def draw_pair(rng):
    """one seeded random pair with at least one output"""
    while True:
        kw = dict(c=int(rng.choice([32, 64, 128, 256, 512])), co=32 * int(rng.integers(1, 33)), h=int(rng.integers(1, 49)),
                  w=int(rng.integers(1, 49)), stride=int(rng.integers(1, 3)), pad=tuple(int(v) for v in rng.integers(0, 3, 4)),
                  n=int(rng.integers(1, 4)), acts=(int(rng.integers(0, 3)), int(rng.integers(0, 3))))
        rows = int(rng.integers(2, 6)) if rng.integers(0, 3) == 0 else 0
        pad, s = kw["pad"], kw["stride"]
        if cases.out_size(kw["h"], 3, s, pad[0], pad[2], 1) >= 1 and cases.out_size(kw["w"], 3, s, pad[1], pad[3], 1) >= 1:
            return kw, rows


@pytest.mark.gpu
def test_random_fp16_pairs(gpu, monkeypatch):
    """SHL_FUZZ_N seeded draws (default 8): each runs fused and passes L0 - L3, or is refused -- and then pwdw_forward says
    ENOTSUP and leaves the output alone.  At least three quarters must run fused."""
    fe, hip, opt, dev = gpu
    rng = np.random.default_rng(20261016)
    draws = int(os.environ.get("SHL_FUZZ_N", "8"))
    fused, forced = 0, set()
    for k in range(draws):
        kw, rows = draw_pair(rng)
        if rows:
            monkeypatch.setenv("SHL_MI355X_PWDW_F16_ROWS", str(rows))
        else:
            monkeypatch.delenv("SHL_MI355X_PWDW_F16_ROWS", raising=False)
        pw, dw = make_pwdw_f16(100 + k, **kw)
        what = "draw %d %s rows %d" % (k, kw, rows)
        keep = []
        plan_pw, mid_alone = plan_of(gpu, pw, keep)
        plan_dw, _ = plan_of(gpu, dict(dw, input=mid_alone), keep)
        d_in = dev.alloc(pw["input"].nbytes)
        dev.upload(d_in, pw["input"])
        if hip.shl_mi355x_pwdw_fusable(plan_pw, plan_dw, pw["n"]) == 1:
            check_layers(gpu, plan_pw, plan_dw, pw, dw, d_in, what, keep=keep)
            fused += 1
            if rows:
                forced.add(rows)
        else:
            nbytes = pw["n"] * pw["co"] * dw["ho"] * dw["wo"] * 2
            d_out = dev.alloc(nbytes)
            hip.shl_mi355x_memset(d_out, 0xFF, nbytes, None)
            assert hip.shl_mi355x_pwdw_forward(plan_pw, plan_dw, d_in, d_out, pw["n"], None) == ENOTSUP, what
            assert (dev.download(d_out, (nbytes,), np.uint8) == 0xFF).all(), "%s: a refused pair wrote its output" % what
            dev.free(d_out)
        dev.free(d_in)
        for p, _ in keep:
            opt.shl_mi355x_release_params(p)
    print("random binary16 pairs: %d of %d ran fused (forced rows among them: %s)" % (fused, draws, sorted(forced)))
    assert fused * 4 >= draws * 3, "only %d of %d draws ran fused" % (fused, draws)


# pairs outside the kernel's form: (what, pointwise overrides, depthwise overrides)
F16_REFUSED = [
    ("C 96: six K sub-steps in one part", dict(c=96), {}),
    ("C 160: five K sub-steps per part", dict(c=160), {}),
    ("C 384: six K sub-steps per part", dict(c=384), {}),
    ("C 1024 > 512", dict(c=1024), {}),
    ("C 48 not a multiple of 32", dict(c=48), {}),
    ("Co 48 not a multiple of 32", dict(co=48), {}),
    ("depthwise dilation 2", {}, dict(dilation=(2, 2), pad=(2, 2, 2, 2))),
    ("depthwise stride 3", {}, dict(stride=(3, 3))),
    ("depthwise top pad 3", {}, dict(pad=(3, 1, 1, 1))),
    ("depthwise left pad 3", {}, dict(pad=(1, 3, 1, 1))),
    ("pointwise stride 2", dict(stride=(2, 2)), {}),
    ("pointwise padding 1", dict(pad=(1, 1, 1, 1)), {}),
    ("pointwise output scale 2", dict(out_scale=2.0), {}),
    ("depthwise output scale 0.5", {}, dict(out_scale=0.5)),
]


def refused_pair(i, pw_kw, dw_kw):
    kw = dict(layout=cases.NCHW, dtype="f16", n=2, h=9, w=11, c=64, co=64, k=(1, 1), pad=(0, 0, 0, 0), act=1)
    scale = pw_kw.pop("out_scale", None)
    kw.update(pw_kw)
    pw = cases.make_case(1900 + i, **kw)
    dkw = dict(layout=cases.NCHW, dtype="f16", n=2, h=pw["ho"], w=pw["wo"], c=pw["co"], depthwise=True, act=1)
    dscale = dw_kw.pop("out_scale", None)
    dkw.update(dw_kw)
    dw = cases.make_case(1950 + i, **dkw)
    if scale is not None:
        pw["out_scale"] = scale
    if dscale is not None:
        dw["out_scale"] = dscale
    return pw, dw


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(F16_REFUSED)), ids=[r[0].split(":")[0].replace(" ", "_") for r in F16_REFUSED])
def test_fp16_pairs_outside_the_form_are_refused_and_run_as_two_launches(gpu, i, monkeypatch):
    monkeypatch.delenv("SHL_MI355X_PWDW_F16_ROWS", raising=False)
    fe, hip, opt, dev = gpu
    what, pw_kw, dw_kw = F16_REFUSED[i]
    pw, dw = refused_pair(i, dict(pw_kw), dict(dw_kw))
    keep = []
    plan_pw, mid = plan_of(gpu, pw, keep)
    golden_util.compare_f16_tol(mid, cases.oracle_run(pw, "f16"), "%s: stand-alone pointwise vs oracle" % what)
    dw["input"] = mid
    plan_dw, out = plan_of(gpu, dw, keep)
    golden_util.compare_f16_tol(out, cases.oracle_run(dw, "f16"), "%s: stand-alone depthwise vs oracle (fed the GPU's intermediate)" % what)
    assert hip.shl_mi355x_pwdw_fusable(plan_pw, plan_dw, pw["n"]) == 0, what
    d_in, d_out = dev.alloc(pw["input"].nbytes), dev.alloc(out.nbytes)
    dev.upload(d_in, pw["input"])
    hip.shl_mi355x_memset(d_out, 0xFF, out.nbytes, None)
    assert hip.shl_mi355x_pwdw_forward(plan_pw, plan_dw, d_in, d_out, pw["n"], None) == ENOTSUP, what
    assert (dev.download(d_out, (out.nbytes,), np.uint8) == 0xFF).all(), "%s: a refused pair wrote its output" % what
    dev.free(d_in)
    dev.free(d_out)
    for p, _ in keep:
        opt.shl_mi355x_release_params(p)


@pytest.mark.gpu
def test_fp16_two_layer_session_with_an_output_scale_keeps_two_launches(gpu):
    """csinn_session_setup on pointwise -> depthwise: with the depthwise layer's output scale 1 the session fuses the pair; with
    0.5 it keeps two launches -- and then equals the two stand-alone launches bit for bit, each within 1e-3 of the oracle."""
    fe, hip, opt, dev = gpu
    pw = cases.make_case(1990, layout=cases.NCHW, dtype="f16", h=10, w=10, c=64, co=64, k=(1, 1), pad=(0, 0, 0, 0), act=1)
    dw = cases.make_case(1991, layout=cases.NCHW, dtype="f16", h=10, w=10, c=64, depthwise=True, act=1)
    got = None
    for scale in (1.0, 0.5):
        dw["out_scale"] = scale
        net = tail.MiniNet("f16", "NCHW", hw=10, c0=64)
        net.layers = [("conv", "pw", pw), ("conv", "dw", dw)]
        sess = net.build(fe, pkg.API_MI355X)
        assert opt.shl_mi355x_session_is_device_resident(sess) == 2
        assert opt.shl_mi355x_session_fused_pairs(sess) == (1 if scale == 1.0 else 0), "output scale %g" % scale
        got = net.run(fe, pw["input"])
        net.close(fe)
    keep = []
    mid = cases.csinn_run(fe, pkg.API_MI355X, pw, device=dev, keep_params=keep)
    golden_util.compare_f16_tol(mid, cases.oracle_run(pw, "f16"), "stand-alone pointwise vs oracle")
    dw["input"] = mid
    want = cases.csinn_run(fe, pkg.API_MI355X, dw, device=dev, keep_params=keep)
    golden_util.compare_f16_tol(want, cases.oracle_run(dw, "f16"), "stand-alone depthwise vs oracle (fed the GPU's intermediate)")
    for p, _ in keep:
        opt.shl_mi355x_release_params(p)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), "session vs the two stand-alone launches: %d words differ" % (
        int((got.view(np.uint16) != want.view(np.uint16)).sum()))

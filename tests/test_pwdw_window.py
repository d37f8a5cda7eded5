"""The fused pointwise + depthwise pair (csrc/pwdw_fused.hip) computes only the in-image WINDOW of a workgroup's patch -- patch pixels
outside the image are the depthwise layer's padding, written to LDS up front -- and its rectangle grids may have border rectangles
one pixel wider than the interior ones (their patch has a row / column of padding).  Checked here:

  * the fused launch against the two stand-alone launches, bit for bit, on maps where border and interior rectangles differ
    (14, 7, 13, 15, 28), strides 1 and 2, paddings 0 / 1 / 2 and two asymmetric ones, batches 1 and 3, K = 256 and 512, power-of-two
    and converter scales -- every pair asserted to run the latency form;
  * a uniform grid forced through SHL_MI355X_PWDW_TILE gives the same bytes as the grid the library chooses;
  * MobileNetV1's two 14 x 14 stride-1 pairs run ONE 32-pixel tile per workgroup on a 4 x 4 grid of rectangles 4 / 3 / 3 / 4 wide and
    high, 256 workgroups (shl_mi355x_pwdw_geometry).
"""
import ctypes as C

import numpy as np
import pytest

import cases
from cases import pkg
from test_fusion import make_pwdw

MAPS = [14, 7, 13, 15, 28]
PADS = [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (0, 1, 2, 1), (2, 0, 1, 2)]
GEOMETRY_FIELDS = 12  # shl_mi355x_pwdw_geometry: ny, nx, bh, bw, ey_lo, ey_hi, ex_lo, ex_hi, tiles, K split, window pixels, workgroups


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    opt.shl_mi355x_registry_get.restype = C.c_void_p
    opt.shl_mi355x_registry_get.argtypes = [C.c_void_p]
    return fe, hip, opt


class Pair:
    """a pointwise + depthwise pair with its two plans and the stand-alone launches' result"""

    def __init__(self, gpu, seed, **kw):
        self.fe, self.hip, self.opt = gpu
        self.dev = cases.HipDevice(self.hip)
        self.pw, self.dw = make_pwdw(seed, **kw)
        self.keep = []
        mid = cases.csinn_run(self.fe, pkg.API_MI355X, self.pw, device=self.dev, keep_params=self.keep)
        self.dw["input"] = mid
        self.want = cases.csinn_run(self.fe, pkg.API_MI355X, self.dw, device=self.dev, keep_params=self.keep)
        self.plan_pw, self.plan_dw = (self.opt.shl_mi355x_registry_get(p) for p, _ in self.keep)
        self.n = self.pw["n"]

    def form(self):
        return self.hip.shl_mi355x_pwdw_form(self.plan_pw, self.plan_dw, self.n)

    def geometry(self):
        g = (C.c_int32 * GEOMETRY_FIELDS)()
        pkg.check(self.hip.shl_mi355x_pwdw_geometry(self.plan_pw, self.plan_dw, self.n, g, GEOMETRY_FIELDS), self.hip, "pwdw_geometry")
        return list(g)

    def fused(self):
        hip, dev = self.hip, self.dev
        d_in, d_out = dev.alloc(self.pw["input"].nbytes), dev.alloc(self.want.nbytes)
        dev.upload(d_in, self.pw["input"])
        hip.shl_mi355x_memset(d_out, 0x55, self.want.nbytes, None)
        pkg.check(hip.shl_mi355x_pwdw_forward(self.plan_pw, self.plan_dw, d_in, d_out, self.n, None), hip, "pwdw_forward")
        got = dev.download(d_out, self.want.shape, np.int8).copy()
        dev.free(d_in)
        dev.free(d_out)
        return got

    def release(self):
        for p, _ in self.keep:
            self.opt.shl_mi355x_release_params(p)


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("hw", MAPS)
def test_fused_pair_equals_the_two_launches_where_border_and_interior_rectangles_differ(gpu, hw, stride, monkeypatch):
    monkeypatch.delenv("SHL_MI355X_PWDW_TILE", raising=False)
    seed = 0
    for pad in PADS:
        for n in (1, 3):
            for c in (256, 512):
                for exact in (True, False):
                    seed += 1
                    # (the run-time form on every fourth pair: same semantics, eight-wave capable, its own index arithmetic)
                    monkeypatch.setenv("SHL_MI355X_PWDW_GENERIC", "1" if seed % 4 == 0 else "0")
                    what = "hw %d stride %d pad %s n %d K %d exact %d" % (hw, stride, pad, n, c, exact)
                    pair = Pair(gpu, 100 * hw + 50 * stride + seed, c=c, co=512, hw=hw, stride=stride, n=n, exact=exact, pad=pad)
                    assert pair.form() == 1, what + ": the pair does not run the fused latency form"
                    got = pair.fused()
                    bad, worst = cases.mismatch_report(got, pair.want)
                    assert bad == 0, "%s (geometry %s): fused vs stand-alone: %d mismatches (max |d| %d)" % (what, pair.geometry(), bad, worst)
                    pair.release()


@pytest.mark.gpu
@pytest.mark.parametrize("hw,tile", [(14, "4x4"), (14, "2x7"), (7, "2x4"), (15, "3x5")])
def test_forced_uniform_grid_gives_the_same_bytes(gpu, hw, tile, monkeypatch):
    monkeypatch.setenv("SHL_MI355X_PWDW_GENERIC", "0")
    monkeypatch.delenv("SHL_MI355X_PWDW_TILE", raising=False)
    pair = Pair(gpu, 900 + hw, c=512, co=512, hw=hw, stride=1, n=1, exact=True, pad=(1, 1, 1, 1))
    assert pair.form() == 1
    chosen = pair.fused()
    bad, worst = cases.mismatch_report(chosen, pair.want)
    assert bad == 0, "chosen grid %s: %d mismatches (max |d| %d)" % (pair.geometry(), bad, worst)
    monkeypatch.setenv("SHL_MI355X_PWDW_TILE", tile)
    assert pair.form() == 1, "the forced grid %s does not fit" % tile
    g = pair.geometry()
    bh, bw = (int(v) for v in tile.split("x"))
    assert g[2:8] == [bh, bw, 0, 0, 0, 0], "SHL_MI355X_PWDW_TILE=%s must mean a uniform grid, got %s" % (tile, g)
    assert g[0:2] == [(hw + bh - 1) // bh, (hw + bw - 1) // bw]
    forced = pair.fused()
    assert np.array_equal(forced, chosen), "forced uniform grid %s and the chosen grid differ" % tile
    pair.release()


@pytest.mark.gpu
@pytest.mark.parametrize("c", [256, 512])
def test_the_14x14_stride_1_pairs_run_one_tile_on_a_4_3_3_4_grid(gpu, c, monkeypatch):
    monkeypatch.setenv("SHL_MI355X_PWDW_GENERIC", "0")
    monkeypatch.delenv("SHL_MI355X_PWDW_TILE", raising=False)
    pair = Pair(gpu, 950 + c, c=c, co=512, hw=14, stride=1, n=1, exact=True, pad=(1, 1, 1, 1))
    assert pair.form() == 1
    ny, nx, bh, bw, ey_lo, ey_hi, ex_lo, ex_hi, tiles, ks, nwin, wgs = pair.geometry()
    print("geometry:", pair.geometry())
    assert (ny, nx) == (4, 4), "a 4 x 4 grid of rectangles"
    assert [bh + ey_lo, bh, bh, bh + ey_hi] == [4, 3, 3, 4] and [bw + ex_lo, bw, bw, bw + ex_hi] == [4, 3, 3, 4]
    assert tiles == 1 and nwin == 25, "every rectangle's window is 5 x 5 pixels: one 32-pixel tile"
    assert ks == 4 and wgs == 256
    bad, worst = cases.mismatch_report(pair.fused(), pair.want)
    assert bad == 0, "%d mismatches (max |d| %d)" % (bad, worst)
    pair.release()

"""The fused pointwise + depthwise pair (csrc/pwdw_fused.hip) on windows whose tile count is no multiple of the wave groups: the
NT forms (pwdw_fused_nt_kernel<NSW, KS, NT>) have that count compiled in -- every tile's patch slot is computed in the MFMAs' block
and the finishing between the two barriers is straight-line code (profiles/pwdw_nt_notes.md).  Checked here, for every
instantiated (NSW, KS, NT) on the smallest map that reaches it under a forced uniform grid (SHL_MI355X_PWDW_TILE, the harness of
test_pwdw_window.py):

  * the geometry (tiles, K split) and the form that would launch (shl_mi355x_pwdw_launch_form) are the expected ones;
  * the fused launch equals the two stand-alone launches bit for bit, and the oracle chain where the scales are exact;
  * SHL_MI355X_PWDW_GENERIC=1 (the run-time form) gives the same bytes.

Each map has interior rectangles with the widest window and clipped border rectangles whose windows are narrower than the
launch's row pitch: their unused MFMA rows go to the plane's spare slot -- the case the compile-time slots can get wrong.

  form (1, 1, 5): 17 x 41 x 32, depthwise stride 2 pad 1 -> 9 x 21, 4x7 rectangles: the middle rectangle's window is 9 x 15 = 135
                  pixels, 5 tiles; the last rectangle row is one output row long.
  form (2, 1, 3): 21 x 21 x 64, stride 1 pad 1 -> 21 x 21, 7x7 rectangles: the middle window is 9 x 9 = 81 pixels, 3 tiles.
  form (2, 2, 3): 25 x 25 x 128, stride 2 pad 1 -> 13 x 13, 4x4 rectangles: middle windows 9 x 9, 3 tiles, K split 2; the last
                  rectangle of an axis is one pixel long and sticks out of the map.

Flavours: (3, 3) power-of-two scales, (0, 0) converter scales, (-1, -1) the run-time flavour -- reached with one layer of each kind
(cases.make_case draws no activation whose clamp form fails, which is the other way into that flavour).
"""
import ctypes as C

import numpy as np
import pytest

import cases
from cases import pkg
from test_pwdw_window import Pair

LAUNCH_FIELDS = 5  # shl_mi355x_pwdw_launch_form: kind, K sub-steps per wave, K split, tiles per wave, tiles per window
LAUNCH_RUNTIME, LAUNCH_NT = 0, 3  # include/shl_mi355x.h

#  (NSW, KS, NT): input h, w, c, depthwise stride, SHL_MI355X_PWDW_TILE
FORMS = {
    (1, 1, 5): dict(h=17, w=41, c=32, stride=2, tile="4x7"),
    (2, 1, 3): dict(h=21, w=21, c=64, stride=1, tile="7x7"),
    (2, 2, 3): dict(h=25, w=25, c=128, stride=2, tile="4x4"),
}
#  flavour: the two layers' `exact` (power-of-two output scale)
FLAVOURS = {3: (True, True), 0: (False, False), -1: (True, False)}


class NtPair(Pair):
    """test_pwdw_window.Pair on a map that need not be square, the two layers' scales chosen apart"""

    def __init__(self, gpu, seed, h, w, c, co, stride, n, relu, exact):
        self.fe, self.hip, self.opt = gpu
        self.dev = cases.HipDevice(self.hip)
        self.pw = cases.make_case(700 + seed, n=n, h=h, w=w, c=c, co=co, k=(1, 1), pad=(0, 0, 0, 0), act=relu, exact=exact[0])
        self.dw = cases.make_case(750 + seed, n=n, h=h, w=w, c=co, depthwise=True, stride=(stride, stride), act=relu, exact=exact[1])
        self.dw["in_scale"], self.dw["in_zp"] = self.pw["out_scale"], self.pw["out_zp"]
        self.dw["b_scale"] = (np.float32(self.dw["in_scale"]) * self.dw["k_scale"]).astype(np.float32)
        self.keep = []
        self.mid = cases.csinn_run(self.fe, pkg.API_MI355X, self.pw, device=self.dev, keep_params=self.keep)
        self.dw["input"] = self.mid
        self.want = cases.csinn_run(self.fe, pkg.API_MI355X, self.dw, device=self.dev, keep_params=self.keep)
        self.plan_pw, self.plan_dw = (self.opt.shl_mi355x_registry_get(p) for p, _ in self.keep)
        self.n = n

    def launch_form(self):
        v = (C.c_int32 * LAUNCH_FIELDS)()
        pkg.check(self.hip.shl_mi355x_pwdw_launch_form(self.plan_pw, self.plan_dw, self.n, v, LAUNCH_FIELDS), self.hip, "pwdw_launch_form")
        return list(v)

    def oracle(self):
        o_mid = cases.oracle_run(self.pw, "exact")
        o_dw = dict(self.dw)
        o_dw["input"] = o_mid
        return cases.oracle_run(o_dw, "exact")


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    opt.shl_mi355x_registry_get.restype = C.c_void_p
    opt.shl_mi355x_registry_get.argtypes = [C.c_void_p]
    return fe, hip, opt


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", sorted(FLAVOURS, reverse=True), ids=lambda f: "flavour%d" % f)
@pytest.mark.parametrize("key", sorted(FORMS), ids=lambda k: "nsw%d_ks%d_nt%d" % k)
def test_nt_form_equals_the_two_launches_and_the_runtime_form(gpu, key, flavour, monkeypatch):
    nsw, ks, nt = key
    shape = FORMS[key]
    tpw = -(-nt // (4 // ks))
    seed = 0
    #  N = 1 and 2, relu and no activation at Co = 32; a second slice (Co = 64) once
    for n, relu, co in [(1, 1, 32), (2, 1, 32), (1, 0, 32), (2, 0, 32), (1, 1, 64)]:
        seed += 1
        what = "form %s flavour %d: n %d relu %d co %d" % (key, flavour, n, relu, co)
        monkeypatch.setenv("SHL_MI355X_PWDW_TILE", shape["tile"])
        monkeypatch.setenv("SHL_MI355X_PWDW_GENERIC", "0")
        pair = NtPair(gpu, 10 * nt + 100 * ks + seed, shape["h"], shape["w"], shape["c"], co, shape["stride"], n, relu, FLAVOURS[flavour])
        assert pair.form() == 1, what + ": the pair does not run the fused latency form"
        geo = pair.geometry()
        bh, bw = (int(v) for v in shape["tile"].split("x"))
        assert geo[2:8] == [bh, bw, 0, 0, 0, 0] and geo[8:10] == [nt, ks], "%s: geometry %s, expected %s rectangles, %d tiles, K split %d" % (what, geo, shape["tile"], nt, ks)
        assert pair.launch_form() == [LAUNCH_NT, nsw, ks, tpw, nt], "%s: launches %s, not the NT form" % (what, pair.launch_form())
        got = pair.fused()
        bad, worst = cases.mismatch_report(got, pair.want)
        assert bad == 0, "%s (geometry %s): fused vs stand-alone: %d mismatches (max |d| %d)" % (what, geo, bad, worst)
        if flavour == 3:
            bad, worst = cases.mismatch_report(got, pair.oracle())
            assert bad == 0, "%s: fused vs the oracle chain: %d mismatches (max |d| %d)" % (what, bad, worst)
        monkeypatch.setenv("SHL_MI355X_PWDW_GENERIC", "1")
        assert pair.launch_form()[0] == LAUNCH_RUNTIME, what + ": SHL_MI355X_PWDW_GENERIC=1 must force the run-time form"
        assert np.array_equal(pair.fused(), got), what + ": the run-time form and the NT form differ"
        pair.release()

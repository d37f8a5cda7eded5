"""The fused stem + depthwise launch (csrc/stemdw_fused.hip) on the shapes where its input gather and its padding can go wrong.

A task of the kernel gathers the 27 input bytes of a stem output pixel; a tap outside the image -- and every tap of a patch
pixel outside the stem's map -- takes the stem's input zero point, and a patch pixel outside the map is stored as the depthwise
layer's padding value.  A wrong bound reads another pixel or keeps a byte that should have been replaced: both show only where
the padding is a large part of the image, so the inputs here are a few pixels wide and high, the zero points of both layers are
far from zero, and rectangles stick out of the map.  Every case compares the fused launch, between two guard bands, bit for
bit against the two stand-alone launches and, where both layers' scales are exact powers of two, against the oracle chain as
well.

Seeded operands in the manner of tests/pair_sweeps.py: make_case(seed) for the stem, make_case(seed + SECOND_SEED) for the
depthwise layer, coupled through the intermediate zero point.
"""
import ctypes as C

import numpy as np
import pytest

import cases
import pair_sweeps as ps
from cases import pkg

BAND = 4096
SEED0 = 935000


def E(h, w, st=1, sp=1, dil=1, ds=1, dp=1, n=1, act=(1, 1), exact=(True, True), zp_in=-5, zp_mid=7, tile=None):
    sp = (sp,) * 4 if isinstance(sp, int) else sp
    dp = (dp,) * 4 if isinstance(dp, int) else dp
    return dict(h=h, w=w, st=st, sp=sp, dil=dil, ds=ds, dp=dp, n=n, act=act, exact=exact, zp_in=zp_in, zp_mid=zp_mid, tile=tile)


# input h x w, stem stride / padding / dilation, depthwise stride / padding, images, activations, exact scales, zero points, tile
EDGES = [
    E(3, 3, st=1, sp=1, ds=1, dp=1, act=(0, 1), zp_in=9, zp_mid=-3),                       # every tap row and column leaves the image somewhere
    E(3, 3, st=2, sp=1, ds=2, dp=2, n=3, act=(2, 0), exact=(False, False), zp_in=-128, zp_mid=127),
    E(3, 3, st=1, sp=0, ds=1, dp=1, act=(1, 2), zp_in=127, zp_mid=-128),                   # a 1 x 1 stem map: eight of nine patch pixels are padding
    E(4, 5, st=1, sp=0, ds=2, dp=1, n=3, act=(0, 0), exact=(True, False), zp_in=33, zp_mid=-3),   # (mixed scales: the run-time flavour)
    E(4, 5, st=2, sp=1, ds=1, dp=2, act=(1, 1), zp_in=-77, zp_mid=7),                      # depthwise padding 2: patch origin at -2
    E(7, 9, st=1, sp=1, ds=2, dp=0, act=(2, 2), exact=(False, False), zp_in=9, zp_mid=127),
    E(7, 9, st=2, sp=0, ds=1, dp=0, n=3, act=(1, 0), zp_in=-128, zp_mid=-128),             # no padding anywhere: no tap may be replaced
    E(7, 9, st=1, sp=0, ds=1, dp=2, act=(0, 2), zp_in=127, zp_mid=7),
    E(9, 4, st=1, sp=1, ds=1, dp=1, act=(1, 1), exact=(False, False), zp_in=-5, zp_mid=-3),
    E(9, 4, st=2, sp=1, ds=2, dp=2, n=3, act=(2, 1), zp_in=64, zp_mid=127),
    E(5, 5, st=1, sp=1, dil=2, ds=1, dp=1, act=(1, 1), zp_in=-99, zp_mid=-128),            # dilation 2: taps two pixels apart
    E(5, 5, st=1, sp=0, dil=2, ds=2, dp=2, n=3, act=(0, 1), exact=(False, False), zp_in=9, zp_mid=7),
    E(7, 9, st=1, sp=(0, 1, 1, 0), ds=1, dp=(1, 0, 2, 1), act=(2, 0), zp_in=-128, zp_mid=127),   # unequal padding on the four sides
    E(7, 9, st=1, sp=1, ds=1, dp=1, n=3, act=(1, 1), zp_in=127, zp_mid=-3, tile="2x4"),    # 4 x 3 rectangles of 2 x 4 on a 7 x 9 map: the last stick out
    E(12, 30, st=1, sp=1, ds=2, dp=1, n=2, act=(1, 2), zp_in=-128, zp_mid=127),            # 310 tasks: a second round of 256, its surplus tasks idle
]
IDS = ["%dx%d_s%d_p%s_d%d_dw_s%d_p%s_n%d%s" % (e["h"], e["w"], e["st"], "".join(map(str, e["sp"])), e["dil"], e["ds"],
                                              "".join(map(str, e["dp"])), e["n"], "_tile" + e["tile"] if e["tile"] else "") for e in EDGES]


def make_pair(i):
    e = EDGES[i]
    first = cases.make_case(SEED0 + i, n=e["n"], h=e["h"], w=e["w"], c=3, co=32, stride=(e["st"],) * 2, pad=e["sp"],
                            dilation=(e["dil"],) * 2, act=e["act"][0], exact=e["exact"][0])
    assert first["ho"] >= 1 and first["wo"] >= 1, "case %d: the stem has no output" % i
    second = cases.make_case(SEED0 + i + ps.SECOND_SEED, n=e["n"], h=first["ho"], w=first["wo"], c=32, depthwise=True,
                             stride=(e["ds"],) * 2, pad=e["dp"], act=e["act"][1], exact=e["exact"][1])
    assert second["ho"] >= 1 and second["wo"] >= 1, "case %d: the depthwise layer has no output" % i
    first["in_zp"] = e["zp_in"]
    ps.couple(first, second, e["zp_mid"])
    return first, second


def test_the_cases_cover_what_they_are_meant_to():
    """CPU: the list holds every shape, stride, padding, image count and activation it is there for"""
    pairs = [make_pair(i) for i in range(len(EDGES))]
    assert {(3, 3), (4, 5), (7, 9), (9, 4)} <= {(e["h"], e["w"]) for e in EDGES}
    assert {(1, 0), (1, 1), (2, 0), (2, 1)} <= {(e["st"], e["sp"][0]) for e in EDGES}
    assert any(e["dil"] == 2 and (e["h"], e["w"]) == (5, 5) for e in EDGES)
    assert {(1, 0), (2, 0), (1, 1), (2, 1), (1, 2), (2, 2)} <= {(e["ds"], e["dp"][0]) for e in EDGES}
    assert {1, 3} <= {e["n"] for e in EDGES}
    assert {0, 1, 2} <= {e["act"][0] for e in EDGES} and {0, 1, 2} <= {e["act"][1] for e in EDGES}
    assert all(e["zp_in"] != 0 and e["zp_mid"] != 0 for e in EDGES)
    assert {ps.flavour(dict(first=dict(exact=e["exact"][0]), second=dict(exact=e["exact"][1]))) for e in EDGES} == {(3, 3), (0, 0), (-1, -1)}
    # the tile case: rectangles that stick out of the map on both axes
    (e, (_, second)), = [(e, p) for e, p in zip(EDGES, pairs) if e["tile"]]
    th, tw = (int(v) for v in e["tile"].split("x"))
    assert second["ho"] % th and second["wo"] % tw and th < second["ho"] and tw < second["wo"]
    # the rule's own geometry elsewhere; one case with more than one round of 256 tasks
    geo = [ps.stemdw_geometry(p[1]["ho"], p[1]["wo"], e["ds"], e["ds"], e["n"], e["tile"]) for e, p in zip(EDGES, pairs)]
    assert all(g is not None for g in geo)
    assert max(g["phase1_trips"] for g in geo) >= 2 and min(g["phase1_trips"] for g in geo) == 1


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
@pytest.mark.parametrize("i", range(len(EDGES)), ids=IDS)
def test_fused_stem_pair_equals_the_two_launches_at_the_image_edges(gpu, i, monkeypatch):
    fe, hip, opt = gpu
    e = EDGES[i]
    monkeypatch.delenv("SHL_MI355X_STEMDW_TILE", raising=False)
    if e["tile"]:
        monkeypatch.setenv("SHL_MI355X_STEMDW_TILE", e["tile"])   # (read per call)
    first, second = make_pair(i)
    dev = cases.HipDevice(hip)
    keep = []
    mid = cases.csinn_run(fe, pkg.API_MI355X, first, device=dev, keep_params=keep)
    assert opt.shl_mi355x_params_kernel_name(keep[0][0]).decode() == "conv_stem_i8_dot4"
    second["input"] = mid
    alone = cases.csinn_run(fe, pkg.API_MI355X, second, device=dev, keep_params=keep)
    plan_a, plan_b = (opt.shl_mi355x_registry_get(p) for p, _ in keep)
    assert plan_a and plan_b, "no plan behind a layer's params"
    assert hip.shl_mi355x_pwdw_form(plan_a, plan_b, e["n"]) == ps.FAMILIES["stemdw_i8"]["form"], "the pair is not the fused stem form"
    nb = alone.nbytes
    d_in = dev.alloc(first["input"].nbytes)
    dev.upload(d_in, first["input"])
    buf = dev.alloc(nb + 2 * BAND)
    pkg.check(hip.shl_mi355x_memset(buf, 0x5A, nb + 2 * BAND, None), hip, "memset")
    pkg.check(hip.shl_mi355x_pwdw_forward(plan_a, plan_b, d_in, buf + BAND, e["n"], None), hip, "pwdw_forward(stem)")
    raw = dev.download(buf, (nb + 2 * BAND,), np.uint8)
    dev.free(buf)
    dev.free(d_in)
    for p, _ in keep:
        opt.shl_mi355x_release_params(p)
    got = raw[BAND:BAND + nb].view(np.int8).reshape(alone.shape)
    nbad, worst = cases.mismatch_report(got, alone)
    print("case %d %s: %s -> %s -> %s, %d of %d outputs differ from the stand-alone launches (max |d| %d)" %
          (i, IDS[i], first["in_shape"], second["in_shape"], alone.shape, nbad, alone.size, worst))
    assert nbad == 0, "fused vs stand-alone: %d mismatches (max |d| %d)" % (nbad, worst)
    assert not (raw[:BAND] != 0x5A).any() and not (raw[BAND + nb:] != 0x5A).any(), "bytes outside the output were written"
    if all(e["exact"]):
        o_second = dict(second)
        o_second["input"] = cases.oracle_run(first, "exact")
        nbad, worst = cases.mismatch_report(got, cases.oracle_run(o_second, "exact"))
        print("case %d: %d outputs differ from the oracle chain (max |d| %d)" % (i, nbad, worst))
        assert nbad == 0, "fused vs the oracle chain: %d mismatches (max |d| %d)" % (nbad, worst)

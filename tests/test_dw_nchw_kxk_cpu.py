"""The host half of the depthwise NCHW k x k kernel (csrc/dw_nchw_kxk.h), no GPU: scope, rectangle / plane geometry, LDS budget, the
int8 filter-row packer and the default rule, compiled into a stand-alone program under AddressSanitizer and UBSan that replays the
kernel's thread -> output map."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases

DRIVER = r"""
#include <stdio.h>
#include <vector>
#include "dw_nchw_kxk.h"
using namespace shl;
int main(int, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    int i8, N, C, Co, G, H, W, Ho, Wo, Kh, Kw, sh, sw, dh, dw, zp;
    while (f && fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &i8, &N, &C, &Co, &G, &H, &W, &Ho, &Wo, &Kh, &Kw, &sh, &sw, &dh, &dw, &zp) == 16) {
        DnGeom g = {};
        const bool scope = dn_scope(i8, C, Co, G, Kh, Kw, sh, sw, dh, dw, zp), ok = scope && dn_geometry(i8, N, C, H, W, Ho, Wo, Kh, Kw, sh, sw, g);
        long long cover_bad = 0, read_bad = 0, pack_bad = 0;
        if (ok) {  // the kernels' thread decode: every output once, every window read inside the thread's plane patch
            std::vector<int> seen((size_t)N * C * Ho * Wo, 0);
            const int per = g.cg * g.rw, rd = dn_read_dw(i8, Kw, sw);
            for (long long bx = 0; bx < g.groups; ++bx)
                for (int by = 0; by < g.tiles_x * g.tiles_y; ++by)
                    for (int tid = 0; tid < DN_THREADS; ++tid) {
                        const int pi = tid / per, rr = (tid - pi * per) / g.cg, t = tid - pi * per - rr * g.cg;
                        const long long plane = bx * g.pl + pi;
                        const int oy = by / g.tiles_x * g.rw + rr, ox = (by % g.tiles_x * g.cg + t) * DN_TX;
                        if (pi >= g.pl || plane >= (long long)N * C || oy >= Ho || ox >= Wo) continue;
                        for (int j = 0; j < DN_TX && ox + j < Wo; ++j) ++seen[(size_t)(plane * Ho + oy) * Wo + ox + j];
                        read_bad += rr * sh + Kh > g.ph || t * sw * (i8 ? 1 : 2) + rd > g.pitch_dw || ((DN_TX * t + 3) * sw + Kw) > g.pw;
                    }
            for (int v : seen) cover_bad += v != 1;
            read_bad += g.row_dw > g.pitch_dw || g.row_dw * 4 < g.pw * g.es || !(g.pitch_dw & 1) || g.plane_dw != g.ph * g.pitch_dw ||
                        g.w_dw < g.pl * g.plane_dw || (g.w_dw & 3) || g.lds_bytes != 4 * (g.w_dw + (i8 ? 0 : g.pl * DN_W_SLOT)) || g.cg * g.rw * g.pl > DN_THREADS;
            std::vector<int8_t> w((size_t)C * Kh * Kw);
            unsigned s = 12345u + C;
            for (auto &v : w) v = (int8_t)((s = s * 1664525u + 1013904223u) >> 24);
            std::vector<uint32_t> packed((size_t)dn_weight_bytes(C, Kh) / 4);
            std::vector<int32_t> acc(C);
            dn_pack(w.data(), C, Kh, Kw, zp, packed.data(), acc.data());
            for (int c = 0; c < C; ++c) {
                long long sum = 0;
                for (int ky = 0; ky < Kh; ++ky)
                    for (int kx = 0; kx < 8; ++kx) {
                        const int8_t got = (int8_t)(packed[(size_t)(c * Kh + ky) * 2 + kx / 4] >> (8 * (kx % 4)));
                        const int8_t want = kx < Kw ? w[(size_t)(c * Kh + ky) * Kw + kx] : (int8_t)0;
                        pack_bad += got != want, sum += want;
                    }
                pack_bad += acc[c] != -zp * sum;
            }
        }
        printf("%d %d %lld %lld %lld %d %d %d\n", scope, ok, cover_bad, read_bad, pack_bad, g.lds_bytes, g.pl,
               dn_default(i8, (long long)N * C, Ho, Wo, Kh, Kw, sh, sw) && !dn_scope(i8, C, C, C, Kh, Kw, sh, sw, 1, 1, 0));  // (what the rule sees)
    }
    return f ? 0 : 2;
}
"""


def problem(i8, c, h, w, k, s=(1, 1), pad=None, n=1, d=(1, 1), co=None, group=None, zp=-5):
    pad = pad or (k[0] // 2, k[1] // 2, k[0] // 2, k[1] // 2)
    ho, wo = cases.out_size(h, k[0], s[0], pad[0], pad[2], d[0]), cases.out_size(w, k[1], s[1], pad[1], pad[3], d[1])
    return (i8, n, c, co or c, group or c, h, w, ho, wo, k[0], k[1], s[0], s[1], d[0], d[1], zp)


# the shapes of tests/test_dw_nchw_kxk.py, the measured layers at batch 1 and 32, seeded ones over the whole scope -- in both dtypes
_T = [(5, 7, 7, (5, 5)), (8, 9, 11, (7, 7), (1, 1), None, 2), (4, 12, 9, (5, 5), (2, 2)), (6, 8, 8, (5, 5), (2, 2), (1, 1, 2, 2)),
      (4, 9, 11, (5, 3), (2, 1)), (4, 6, 6, (1, 7)), (4, 6, 6, (7, 1)), (3, 6, 6, (7, 7)), (2, 40, 40, (5, 5), (1, 1), None, 2),
      (2, 5, 70, (5, 5)), (4, 9, 9, (4, 4), (1, 1), (0, 0, 0, 0))]
_T += [(c, hw, hw, (k, k), (s, s), None, n) for n in (1, 32) for (c, hw, k, s) in
       ((72, 56, 5, 2), (120, 28, 5, 1), (240, 28, 5, 2), (672, 14, 5, 1), (96, 56, 7, 1), (768, 7, 7, 1))]
_rng = np.random.default_rng(78)
for _ in range(150):
    _k = (int(_rng.integers(1, 8)), int(_rng.integers(1, 8)))
    _T.append((int(_rng.integers(2, 13)), int(_rng.integers(7, 41)), int(_rng.integers(7, 80)), _k if _k != (3, 3) else (3, 5),
               (int(_rng.integers(1, 3)), int(_rng.integers(1, 3))), tuple(int(v) for v in _rng.integers(0, 4, 4)), int(_rng.integers(1, 4))))
PROBLEMS = [problem(i8, *t) for t in _T for i8 in (1, 0)]
# the classes tests/test_dw_nchw_kxk.py keeps on their kernels, and the limits
REFUSED = [problem(1, 8, 8, 8, (3, 3)), problem(0, 8, 8, 8, (3, 3)), problem(1, 4, 12, 12, (5, 5), d=(2, 2)), problem(1, 4, 8, 8, (5, 5), co=8),
           problem(1, 8, 8, 8, (5, 5), group=4), problem(1, 8, 8, 8, (5, 5), group=1), problem(0, 4, 20, 20, (8, 5)), problem(0, 4, 20, 20, (5, 5), (3, 1)),
           problem(1, 4, 8, 8, (5, 5), zp=200), problem(0, 1024, 1 << 10, 1 << 10, (5, 5), n=4)]


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if shutil.which("g++") is None or os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer builds run on machines without a GPU, with a host compiler")
    tmp = tmp_path_factory.mktemp("dw_nchw")
    (tmp / "driver.cpp").write_text(DRIVER), (tmp / "problems.txt").write_text("".join(" ".join(map(str, p)) + "\n" for p in PROBLEMS + REFUSED))
    exe = str(tmp / "dw_nchw_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(cases.ROOT, "csi-nn2_amd", "csrc"), str(tmp / "driver.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe, str(tmp / "problems.txt")], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
    out = [[int(v) for v in ln.split()] for ln in res.stdout.splitlines()]
    assert len(out) == len(PROBLEMS + REFUSED)
    return out


@pytest.mark.parametrize("i", range(len(PROBLEMS)), ids=["x".join(map(str, p)) for p in PROBLEMS])
def test_every_output_once_reads_inside_the_patch_lds_in_budget_and_rows_unpack(rows, i):
    scope, ok, cover_bad, read_bad, pack_bad, lds, pl, default = rows[i]
    assert (scope, ok) == (1, 1) and (cover_bad, read_bad, pack_bad) == (0, 0, 0) and 0 < lds <= 32 * 1024 and pl >= 1, rows[i]


def test_shapes_outside_the_scope_or_the_limits_are_refused_and_the_default_rule_stays_inside_the_scope(rows):
    assert [r[1] for r in rows[len(PROBLEMS):]] == [0] * len(REFUSED)
    assert not any(r[7] for r in rows), "the default rule takes a kernel size or stride outside the scope"

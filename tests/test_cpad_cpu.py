"""The host half of the padded-channel implicit-GEMM kernel (csrc/cpad.h), no GPU: scope, rectangle / patch geometry, LDS budget and
weight packer compiled into a stand-alone program under AddressSanitizer and UBSan; what it prints and packs is checked against numpy."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases

DRIVER = r"""
#include <stdio.h>
#include <vector>
#include "cpad.h"
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    int C, Co, Kh, Kw, sh, sw, pt, pl, H, W, Ho, Wo, N, dh, dw, idx = 0;
    while (f && fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &C, &Co, &Kh, &Kw, &sh, &sw, &pt, &pl, &H, &W, &Ho, &Wo, &N, &dh, &dw) == 15) {
        shl::CpGeom g = {};
        const bool ok = shl::cp_scope(C, Kh, Kw, sh, sw, dh, dw, -5) && shl::cp_geometry(C, Co, Kh, Kw, sh, sw, pt, pl, H, W, Ho, Wo, N, g);
        long long staged_end = 0, magic_bad = 0;
        if (ok) {
            for (int j = 0; j < g.nitems; ++j) {  // the kernel's item decode: the magic divisions, the last byte an item writes
                const int pix = (int)(((unsigned long long)(unsigned)j * g.dq_magic) >> 32), r = (int)(((unsigned long long)(unsigned)pix * g.pw_magic) >> 32);
                magic_bad += pix != j / (g.cp / 4) || r != pix / g.pw;
                const long long end = g.tab_bytes + (long long)r * g.pitch + (long long)(pix - r * g.pw) * g.pp + 4 * (j - pix * (g.cp / 4)) + 4;
                staged_end = end > staged_end ? end : staged_end;
            }
            char name[512];  // OHWI weights in, fragments + acc_init (zp_in = -5) out
            snprintf(name, sizeof name, "%s/w%d.bin", argv[2], idx);
            FILE *wf = fopen(name, "rb");
            std::vector<int8_t> w((size_t)Co * Kh * Kw * C), packed((size_t)shl::cp_weight_bytes(g));
            std::vector<int32_t> acc(Co);
            if (!wf || fread(w.data(), 1, w.size(), wf) != w.size()) return 3;
            shl::cp_pack(w.data(), C, Co, Kh, Kw, -5, g, packed.data(), acc.data());
            snprintf(name, sizeof name, "%s/p%d.bin", argv[2], idx);
            FILE *pf = fopen(name, "wb");
            if (!pf || fwrite(packed.data(), 1, packed.size(), pf) != packed.size() || fwrite(acc.data(), 4, acc.size(), pf) != acc.size()) return 4;
            fclose(pf), fclose(wf);
        }
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %lld %lld %lld\n", ok ? 1 : 0, g.flat, g.cp, g.pp, g.cpc, g.nchunk, g.nsteps, g.nblk, g.ncb,
               g.btx, g.bty, g.tiles_x, g.tiles_y, g.pw, g.ph, g.pitch, g.tab_bytes, g.nitems, (long long)shl::cp_lds_bytes(g),
               ok ? (long long)shl::cp_furthest_read(g, Kw, sh, sw) : 0, staged_end, magic_bad, (long long)shl::cp_weight_bytes(g));
        ++idx;
    }
    return f ? 0 : 2;
}
"""


def problem(c, co, k=(3, 3), s=(1, 1), pad=(1, 1, 1, 1), h=8, w=8, n=1, d=(1, 1)):
    ho, wo = cases.out_size(h, k[0], s[0], pad[0], pad[2], d[0]), cases.out_size(w, k[1], s[1], pad[1], pad[3], d[1])
    return (c, co, k[0], k[1], s[0], s[1], pad[0], pad[1], h, w, ho, wo, n, d[0], d[1])


P0 = (0, 0, 0, 0)
# (C, Cout, Kh, Kw, sh, sw, pt, pl, H, W, Ho, Wo, N, dh, dw): the shapes of tests/test_cpad.py ...
PROBLEMS = [problem(24, 40, (1, 1), pad=P0, h=9, w=7), problem(58, 58, (1, 1), pad=P0, h=6, w=5, n=2), problem(72, 24, (1, 1), (2, 2), P0, 9, 9),
            problem(8, 16, s=(2, 2), pad=(0, 0, 1, 1), h=9, w=9), problem(40, 24), problem(20, 20), problem(12, 32, (5, 5), (2, 2), (2, 2, 2, 2), 13, 11),
            problem(232, 32, h=5, w=5), problem(24, 32, n=2), problem(24, 16, (1, 1), pad=P0, h=70, w=70), problem(24, 72, (1, 1), pad=P0, h=296, w=296),
            problem(24, 32, h=20, w=40, n=2), problem(232, 32, h=12, w=16), problem(8, 72, h=148, w=296)]
# ... the measured layers at batch 1 and 32, and seeded ones over the whole scope (a few of them exceed the LDS budget: refused)
PROBLEMS += [problem(c, co, k, pad=(k[0] // 2,) * 4, h=hw, w=hw, n=n) for n in (1, 32) for (c, co, hw, k) in
             ((24, 144, 56, (1, 1)), (120, 40, 28, (1, 1)), (200, 80, 14, (1, 1)), (232, 232, 7, (1, 1)), (24, 24, 56, (3, 3)), (40, 40, 28, (3, 3)))]
_rng = np.random.default_rng(77)
SEEDED = [problem(int(_rng.choice([8, 9, 17, 24, 31, 40, 58, 72, 100, 116, 184, 250])), int(_rng.integers(1, 200)), (int(_rng.integers(1, 8)), int(_rng.integers(1, 8))),
                  (int(_rng.integers(1, 5)), int(_rng.integers(1, 5))), tuple(int(v) for v in _rng.integers(0, 4, 4)), int(_rng.integers(7, 40)), int(_rng.integers(7, 40)),
                  int(_rng.integers(1, 4))) for _ in range(36)]
# the examples outside the scope of tests/test_cpad.py (binary16 and asymmetric weights are the plan's to refuse) and the limits
REFUSED = [problem(16, 16), problem(5, 16, (5, 5), pad=(2, 2, 2, 2)), problem(24, 16, pad=(2, 2, 2, 2), d=(2, 2)), problem(24, 16, d=(1, 2)), problem(7, 16), problem(32, 16, (1, 1), pad=P0), problem(24, 16, (8, 3)), problem(24, 16, s=(5, 1)),
           problem(250, 16, (7, 7), (4, 4), (3, 3, 3, 3), 40, 40), problem(24, 16, (1, 1), pad=P0, h=1 << 12, w=1 << 12, n=8)]


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if shutil.which("g++") is None or os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer builds run on machines without a GPU, with a host compiler")
    tmp = tmp_path_factory.mktemp("cpad")
    every = PROBLEMS + SEEDED + REFUSED
    (tmp / "driver.cpp").write_text(DRIVER), (tmp / "problems.txt").write_text("".join(" ".join(map(str, p)) + "\n" for p in every))
    exe = str(tmp / "cpad_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(cases.ROOT, "csi-nn2_amd", "csrc"), str(tmp / "driver.cpp"), "-o", exe], check=True)
    weights = {}
    for i, (C, Co, Kh, Kw) in enumerate(p[:4] for p in every):
        weights[i] = np.random.default_rng(191 + i).integers(-128, 128, (Co, Kh * Kw, C), dtype=np.int8)
        weights[i].tofile(str(tmp / ("w%d.bin" % i)))
    res = subprocess.run([exe, str(tmp / "problems.txt"), str(tmp)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
    out = [[int(v) for v in ln.split()] for ln in res.stdout.splitlines()]
    assert len(out) == len(every)
    return out, weights, tmp


@pytest.mark.parametrize("i", range(len(PROBLEMS + SEEDED)), ids=["x".join(map(str, p)) for p in PROBLEMS + SEEDED])
def test_patch_fits_lds_reads_stay_inside_it_and_packed_weights_unpack_to_ohwi(rows, i):
    C, Co, Kh, Kw, sh, sw, pt, pl, H, W, Ho, Wo, N = (PROBLEMS + SEEDED)[i][:13]
    ok, flat, cp, pp, cpc, nchunk, nsteps, nblk, ncb, btx, bty, tiles_x, tiles_y, pw, ph, pitch, tab, nitems, lds, furthest, staged_end, magic_bad, wbytes = rows[0][i]
    if not ok:  # only a seeded problem may be refused, and only by the LDS budget: one tile's patch does not fit
        slots = -(-C // 16) | 1  # 16-byte slots between pixels, then between rows: both odd
        table = 4 * (2 * ((Kh * Kw * -(-C // 16) + 1) // 2) + 2)
        one = ((7 * sw + Kw) * slots | 1) * 16 * (3 * sh + Kh) + -(-table // 16) * 16
        assert i >= len(PROBLEMS) and one > 48 * 1024, (PROBLEMS + SEEDED)[i]
        return
    assert flat == int(Kh == Kw == sh == sw == 1 and pt == pl == 0 and (Ho, Wo) == (H, W))
    assert cp == -(-C // 16) * 16 and cpc == cp // 16 and pp in (cp, cp + 16) and (pp // 16) % 2 == 1 and (pitch // 16) % 2 == 1 and pitch >= pw * pp
    assert nchunk == Kh * Kw * cpc and nsteps == -(-nchunk // 2) and nblk == -(-Co // 32) and ncb == min(2, nblk) and wbytes == nblk * nsteps * 1024
    assert 1 <= btx * bty <= 16 // ncb and magic_bad == 0 and nitems == ph * pw * cp // 4
    if flat:  # runs of 32 pixels over the whole batch, every pixel in exactly one workgroup by construction: ceil
        assert (pw, ph, tab) == (32 * btx, 1, 0) and tiles_y == 1 and (tiles_x - 1) * btx * 32 < N * H * W <= tiles_x * btx * 32
    else:
        assert -(-Wo // 8) <= tiles_x * btx < -(-Wo // 8) + btx and -(-Ho // 4) <= tiles_y * bty < -(-Ho // 4) + bty
        assert pw == (8 * btx - 1) * sw + Kw and ph == (4 * bty - 1) * sh + Kh and tab >= 4 * (2 * nsteps + 2) and tiles_x <= 65535 and tiles_y * N <= 65535
    assert staged_end <= lds == tab + ph * pitch <= 48 * 1024
    # every B fragment read: 16 bytes at the pixel's first tap + the chunk's offset (tap row, tap column, channel offset)
    q = np.arange(nchunk)
    off = (q // cpc // Kw) * pitch + (q // cpc % Kw) * pp + 16 * (q % cpc)
    y, x = (np.arange(32 * btx), np.zeros(1, int)) if flat else (np.arange(4 * bty) * sh * pitch, np.arange(8 * btx) * sw)
    base = tab + (y * pp if flat else y)[:, None] + x[None, :] * pp
    assert furthest == base.max() + off.max() + 16 <= lds
    # the packed weights: [block][step][half][row][16 B] -> [channel][chunk][16], chunk q = tap q // cpc, channels 16 (q % cpc) ..
    w, raw = rows[1][i], np.fromfile(str(rows[2] / ("p%d.bin" % i)), dtype=np.int8)
    got = raw[:wbytes].reshape(nblk, nsteps, 2, 32, 16).transpose(0, 3, 1, 2, 4).reshape(nblk * 32, nsteps * 2, 16)
    want = np.zeros((nblk * 32, nsteps * 2 * 16), np.int8)
    padded = np.zeros((Co, Kh * Kw, cp), np.int8)
    padded[:, :, :C] = w
    want[:Co, :nchunk * 16] = padded.reshape(Co, -1)
    assert np.array_equal(got.reshape(nblk * 32, -1), want)
    assert np.array_equal(raw[wbytes:].view(np.int32), 5 * w.astype(np.int64).sum(axis=(1, 2)))  # acc_init = -zp_in sum(w), zp_in = -5


def test_shapes_outside_the_scope_the_budget_or_the_grid_are_refused(rows):
    assert [r[0] for r in rows[0][len(PROBLEMS + SEEDED):]] == [0] * len(REFUSED)

"""The host half of the Kh x Kw stem kernel (csrc/stem_kxk.h), no GPU: scope, rectangle / patch geometry, weight packer and default
rule compiled into a stand-alone program under AddressSanitizer and UBSan; what it prints and packs is checked here against numpy."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases

DRIVER = r"""
#include <stdio.h>
#include <vector>
#include "stem_kxk.h"
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    int C, Co, Kh, Kw, sh, sw, Ho, Wo, N, idx = 0;
    while (f && fscanf(f, "%d %d %d %d %d %d %d %d %d", &C, &Co, &Kh, &Kw, &sh, &sw, &Ho, &Wo, &N) == 9) {
        shl::SkGeom g = {};
        const bool ok = shl::sk_geometry(C, Co, Kh, Kw, sh, sw, Ho, Wo, N, g);
        unsigned long long sum = 0;
        if (ok) {  // OHWI weights in, fragments + acc_init (zp_in = -5) out
            char name[512];
            snprintf(name, sizeof name, "%s/w%d.bin", argv[2], idx);
            FILE *wf = fopen(name, "rb");
            std::vector<int8_t> w((size_t)Co * Kh * Kw * C), packed((size_t)shl::sk_weight_bytes(g));
            std::vector<int32_t> acc(Co);
            if (!wf || fread(w.data(), 1, w.size(), wf) != w.size()) return 3;
            shl::sk_pack(w.data(), C, Co, Kh, Kw, -5, g, packed.data(), acc.data());
            for (size_t i = 0; i < packed.size(); ++i) sum += (uint8_t)packed[i];
            snprintf(name, sizeof name, "%s/p%d.bin", argv[2], idx);
            FILE *pf = fopen(name, "wb");
            if (!pf || fwrite(packed.data(), 1, packed.size(), pf) != packed.size() || fwrite(acc.data(), 4, acc.size(), pf) != acc.size()) return 4;
            fclose(pf);
        }
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %lld %llu %d\n", ok ? 1 : 0, g.nblk, g.ncb, g.spr, g.btx, g.bty, g.tiles_x, g.tiles_y,
               g.row_bytes, g.ph, g.pitch, g.ndw, (int)(g.rdw_magic >> 1), (long long)shl::sk_lds_bytes(g),
               (long long)shl::sk_furthest_read(g, C, sh, sw), (long long)shl::sk_weight_bytes(g), sum,
               (shl::sk_default((int64_t)N * Ho * Wo, C, Co, Kh, Kw, sh, sw, false) ? 1 : 0) + (shl::sk_default((int64_t)N * Ho * Wo, C, Co, Kh, Kw, sh, sw, true) ? 2 : 0));
        ++idx;
    }
    return f ? 0 : 2;
}
"""

# (C, Cout, Kh, Kw, sh, sw, Ho, Wo, N): the shapes of tests/test_stem_kxk.py ...
PROBLEMS = [(3, 64, 7, 7, 2, 2, 12, 10, 1), (3, 40, 7, 7, 2, 2, 4, 4, 2), (3, 96, 4, 4, 4, 4, 4, 5, 1), (3, 32, 16, 16, 16, 16, 2, 3, 1),
            (1, 32, 5, 5, 2, 2, 6, 6, 1), (4, 16, 3, 5, 1, 2, 9, 6, 1), (2, 24, 7, 7, 1, 1, 8, 8, 1), (3, 16, 1, 1, 1, 1, 8, 8, 1),
            (3, 64, 7, 7, 2, 2, 35, 35, 1)]
# ... the measured stems, and the scope's corners: one byte and 64 bytes of filter row, 16 taps, stride 16, one channel, a wide map
PROBLEMS += [(3, 64, 7, 7, 2, 2, 112, 112, 32), (3, 96, 4, 4, 4, 4, 56, 56, 8), (3, 768, 16, 16, 16, 16, 14, 14, 1), (1, 32, 5, 5, 2, 2, 64, 64, 1), (1, 32, 5, 5, 2, 2, 64, 64, 8),
             (1, 1, 1, 1, 1, 1, 1, 1, 1), (4, 33, 16, 16, 16, 16, 9, 9, 3), (4, 8, 16, 16, 1, 1, 40, 40, 1), (1, 300, 1, 16, 16, 1, 5, 70, 1),
             (2, 64, 2, 16, 1, 16, 33, 17, 1), (4, 64, 16, 1, 16, 1, 7, 500, 1)]
# the default rule (profiles/stem_kxk_notes.md): bit 0 NHWC, bit 1 NCHW; every problem not named here stays off
BY_DEFAULT = {(3, 64, 7, 7, 2, 2, 112, 112, 32): 3, (3, 96, 4, 4, 4, 4, 56, 56, 8): 3, (3, 768, 16, 16, 16, 16, 14, 14, 1): 3, (1, 32, 5, 5, 2, 2, 64, 64, 1): 1,
              (1, 32, 5, 5, 2, 2, 64, 64, 8): 3}
REFUSED = [(5, 16, 5, 5, 1, 1, 8, 8, 1), (3, 16, 3, 3, 1, 1, 8, 8, 1), (4, 16, 5, 17, 1, 1, 8, 8, 1), (3, 16, 17, 5, 1, 1, 8, 8, 1), (3, 16, 5, 5, 17, 1, 8, 8, 1),
           (0, 16, 5, 5, 1, 1, 8, 8, 1), (3, 16, 5, 5, 1, 1, 4, 16 * 8 * 65535 + 1, 1), (3, 16, 5, 5, 1, 1, 16 * 4 * 65535 + 1, 8, 1)]


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if shutil.which("g++") is None or os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer builds run on machines without a GPU, with a host compiler")
    tmp = tmp_path_factory.mktemp("stem_kxk")
    (tmp / "driver.cpp").write_text(DRIVER), (tmp / "problems.txt").write_text("".join(" ".join(map(str, p)) + "\n" for p in PROBLEMS + REFUSED))
    exe = str(tmp / "stem_kxk_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(cases.ROOT, "csi-nn2_amd", "csrc"), str(tmp / "driver.cpp"), "-o", exe], check=True)
    weights = {}
    for i, (C, Co, Kh, Kw) in enumerate(p[:4] for p in PROBLEMS):
        weights[i] = np.random.default_rng(91 + i).integers(-128, 128, (Co, Kh, Kw * C), dtype=np.int8)
        weights[i].tofile(str(tmp / ("w%d.bin" % i)))
    res = subprocess.run([exe, str(tmp / "problems.txt"), str(tmp)], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
    out = [[int(v) for v in ln.split()] for ln in res.stdout.splitlines()]
    assert len(out) == len(PROBLEMS) + len(REFUSED)
    return out, weights, tmp


@pytest.mark.parametrize("i", range(len(PROBLEMS)), ids=["x".join(map(str, p)) for p in PROBLEMS])
def test_geometry_covers_the_map_once_and_every_fragment_read_stays_inside_the_patch(rows, i):
    C, Co, Kh, Kw, sh, sw, Ho, Wo, N = PROBLEMS[i]
    ok, nblk, ncb, spr, btx, bty, tiles_x, tiles_y, row_bytes, ph, pitch, ndw, magic_half, lds, furthest, wbytes = rows[0][i][:16]
    assert rows[0][i][17] == BY_DEFAULT.get(PROBLEMS[i], 0)
    assert ok == 1 and nblk == -(-Co // 32) and ncb == min(2, nblk) and spr == (2 if Kw * C > 32 else 1) and wbytes == nblk * Kh * spr * 1024
    assert 1 <= btx * bty <= 16 // ncb  # four waves x four (tile, channel block) pairs
    # per axis with the kernel's own mapping (workgroup, tile, pixel of the 8 x 4 tile -> output): every output row / column exactly once
    for extent, b, tiles, span in ((Wo, btx, tiles_x, 8), (Ho, bty, tiles_y, 4)):
        wg, tile, px = np.meshgrid(np.arange(tiles), np.arange(b), np.arange(span), indexing="ij")
        out = (wg * b * span + tile * span + px).ravel()
        assert np.array_equal(np.bincount(out[out < extent], minlength=extent), np.ones(extent, np.int64))
    assert row_bytes == ((8 * btx - 1) * sw + Kw) * C and ph == (4 * bty - 1) * sh + Kh
    assert pitch % 8 == 4 and row_bytes <= pitch <= row_bytes + 8 and ndw * 4 == ph * pitch and lds == ph * pitch + 48 <= 48 * 1024
    # every B fragment read: five aligned dwords covering 16 bytes at row (y sh + ky) + x sw C + 32 step + 16 half
    y, x, ky, step, half = np.meshgrid(np.arange(4 * bty), np.arange(8 * btx), np.arange(Kh), np.arange(spr), np.arange(2), indexing="ij")
    addr = (y * sh + ky) * pitch + x * sw * C + 32 * step + 16 * half
    assert furthest == (addr // 4 * 4 + 20).max() < lds
    assert (x * sw * C + Kw * C).max() <= row_bytes  # ... and a filter row's own Kw C bytes are staged pixels of its patch row
    j = np.arange(ndw, dtype=np.uint64)
    assert np.array_equal((j * np.uint64(2 * magic_half + 1)) >> np.uint64(32), j // np.uint64(pitch // 4))  # the kernel's division by pitch / 4
    assert tiles_x <= 65535 and tiles_y * N <= 65535


def test_shapes_outside_the_scope_or_the_grid_are_refused(rows):
    assert [r[0] for r in rows[0][len(PROBLEMS):]] == [0] * len(REFUSED)


@pytest.mark.parametrize("i", range(len(PROBLEMS)), ids=["x".join(map(str, p[:4])) for p in PROBLEMS])
def test_unpacked_fragments_are_the_ohwi_weights_and_zeros_elsewhere(rows, i):
    C, Co, Kh, Kw = PROBLEMS[i][:4]
    nblk, spr, w, raw = rows[0][i][1], rows[0][i][3], rows[1][i], np.fromfile(str(rows[2] / ("p%d.bin" % i)), dtype=np.int8)
    n = nblk * Kh * spr * 1024
    assert raw.size == n + 4 * Co
    # [block][ky][step][half][row][16 B] -> [channel][ky][K byte of the padded filter row]
    got = raw[:n].reshape(nblk, Kh, spr, 2, 32, 16).transpose(0, 4, 1, 2, 3, 5).reshape(nblk * 32, Kh, spr * 32)
    want = np.zeros_like(got)
    want[:Co, :, :Kw * C] = w
    assert np.array_equal(got, want)
    assert np.array_equal(raw[n:].view(np.int32), 5 * w.astype(np.int64).sum(axis=(1, 2)))
    assert int(raw[:n].view(np.uint8).sum(dtype=np.uint64)) == rows[0][i][16]  # the program's own checksum of what it wrote

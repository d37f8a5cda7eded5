"""The host geometry of the Kh x Kw depthwise kernel (csrc/dw_kxk.h:dwk_geometry), no GPU: compiled into a stand-alone program
under AddressSanitizer and UBSan, one problem per line in, the geometry out; the properties are checked here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases

DRIVER = r"""
#include <stdio.h>
#include "dw_kxk.h"
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int C, Kh, Kw, sh, sw, Ho, Wo, N;
    while (fscanf(f, "%d %d %d %d %d %d %d %d", &C, &Kh, &Kw, &sh, &sw, &Ho, &Wo, &N) == 8) {
        shl::DwkGeom g = {};
        const bool ok = shl::dwk_geometry(C, Kh, Kw, sh, sw, Ho, Wo, N, g);
        printf("%d %d %d %d %d %d %d %d %d %lld %lld %d\n", ok ? 1 : 0, g.btx, g.bty, g.tiles_x, g.tiles_y, g.pw, g.ph, g.cb, g.npieces,
               (long long)shl::dwk_lds_bytes(g, true), (long long)g.pw_magic, shl::dwk_default((int64_t)N * Ho * Wo, C, Kh * Kw, sh > 1 || sw > 1) ? 1 : 0);
    }
    fclose(f);
    return 0;
}
"""

# (C, Kh, Kw, sh, sw, Ho, Wo, N): the shapes of tests/test_dw_kxk.py ...
PROBLEMS = [(32, 5, 5, 1, 1, 9, 9, 1), (64, 5, 5, 2, 2, 6, 5, 1), (96, 7, 7, 1, 1, 7, 7, 3), (128, 5, 3, 2, 1, 5, 11, 1),
            (64, 5, 5, 2, 2, 4, 4, 1), (160, 5, 5, 1, 1, 10, 10, 1), (64, 7, 7, 1, 1, 6, 6, 1), (256, 5, 5, 1, 1, 7, 7, 1),
            (32, 5, 5, 1, 1, 40, 40, 2), (32, 1, 7, 1, 1, 6, 6, 1)]
# ... each stride pair at each channel block for 5x5 and 7x7 on a map of several rectangles, an even kernel, a map at the grid limit
PROBLEMS += [(c, k, k, sh, sw, 57, 43, 2) for k in (5, 7) for c in (32, 64, 128) for sh in (1, 2) for sw in (1, 2)]
PROBLEMS += [(128, 4, 6, 1, 1, 20, 20, 1), (32, 5, 5, 1, 1, 4, 16 * 65535, 1)]
# ... and the default rule's measured classes (profiles/dw_kxk_notes.md): ConvNeXt-T's 7x7 in; under 96 channels, stride 2 and 5x5 out
BY_DEFAULT = {(96, 7, 7, 1, 1, 56, 56, 1): 1, (768, 7, 7, 1, 1, 7, 7, 1): 1, (96, 7, 7, 1, 1, 56, 56, 8): 1, (64, 7, 7, 1, 1, 56, 56, 8): 0,
              (96, 7, 7, 1, 1, 56, 56, 9): 0, (96, 7, 7, 2, 2, 56, 56, 1): 0, (96, 7, 7, 1, 2, 56, 56, 1): 0, (672, 5, 5, 1, 1, 14, 14, 32): 0}
PROBLEMS += list(BY_DEFAULT)
REFUSED = [(48, 5, 5, 1, 1, 8, 8, 1), (32, 3, 3, 1, 1, 8, 8, 1), (32, 8, 5, 1, 1, 8, 8, 1), (32, 5, 5, 3, 1, 8, 8, 1),
           (32, 5, 5, 1, 1, 4, 16 * 65535 + 1, 1), (128, 5, 5, 1, 1, 8, 8, 65536)]


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if shutil.which("g++") is None or os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer builds run on machines without a GPU, with a host compiler")
    tmp = tmp_path_factory.mktemp("dw_kxk")
    (tmp / "driver.cpp").write_text(DRIVER)
    exe = str(tmp / "dw_kxk_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(cases.ROOT, "csi-nn2_amd", "csrc"), str(tmp / "driver.cpp"), "-o", exe], check=True)
    (tmp / "problems.txt").write_text("".join(" ".join(map(str, p)) + "\n" for p in PROBLEMS + REFUSED))
    res = subprocess.run([exe, str(tmp / "problems.txt")], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
    out = [[int(v) for v in ln.split()] for ln in res.stdout.splitlines()]
    assert len(out) == len(PROBLEMS) + len(REFUSED)
    return out


@pytest.mark.parametrize("i", range(len(PROBLEMS)), ids=["x".join(map(str, p)) for p in PROBLEMS])
def test_geometry_covers_the_map_once_with_its_taps_inside_lds_and_grid_limits(rows, i):
    C, Kh, Kw, sh, sw, Ho, Wo, N = PROBLEMS[i]
    ok, btx, bty, tiles_x, tiles_y, pw, ph, cb, npieces, lds, magic, by_default = rows[i]
    assert ok == 1 and by_default == BY_DEFAULT.get(PROBLEMS[i], by_default)
    assert cb in (32, 64, 128) and C % cb == 0 and 1 <= btx <= 2 and 1 <= btx * bty <= 4 * (128 // cb)  # four tiles per wave at most
    # enumerated per axis with the kernel's own mapping (workgroup, tile of the rectangle, pixel of the 8 x 4 tile -> output):
    # every output row / column is produced exactly once, and each of its taps lies inside the workgroup's patch
    for extent, b, tiles, span, s, K, p in ((Wo, btx, tiles_x, 8, sw, Kw, pw), (Ho, bty, tiles_y, 4, sh, Kh, ph)):
        wg, tile, px = np.meshgrid(np.arange(tiles), np.arange(b), np.arange(span), indexing="ij")
        out = (wg * b * span + tile * span + px).ravel()
        assert np.array_equal(np.bincount(out[out < extent], minlength=extent), np.ones(extent, np.int64))
        assert ((tile * span + px) * s + K - 1).max() < p  # patch coordinate of the last tap, patch origin = the rectangle's first tap
    assert npieces * 1024 >= pw * ph * cb > (npieces - 1) * 1024
    assert sw == 2 or pw % 2 == 0
    j = np.arange(pw * ph, dtype=np.uint64)
    assert np.array_equal((j * np.uint64(magic)) >> np.uint64(32), j // np.uint64(pw))  # the kernel's division by pw
    assert lds == npieces * 1024 + 12 * cb + -(-Kh * Kw * cb // 16) * 16 + 256 and lds <= 80 * 1024
    assert tiles_x <= 65535 and tiles_y * N <= 65535


def test_shapes_outside_the_scope_or_the_grid_are_refused(rows):
    assert [r[0] for r in rows[len(PROBLEMS):]] == [0] * len(REFUSED)

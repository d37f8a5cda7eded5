"""The host half of the grouped matrix-core kernel (csrc/group_mfma.h), no GPU: scope, geometry and the weight packer compiled
into a stand-alone program under AddressSanitizer and UBSan; the geometry's properties and the packed fragments are checked here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases

DRIVER = r"""
#include <stdio.h>
#include <vector>
#include "group_mfma.h"
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int C, Co, G, Kh, Kw, sh, sw, Ho, Wo, N, idx = 0;
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d", &C, &Co, &G, &Kh, &Kw, &sh, &sw, &Ho, &Wo, &N) == 10) {
        shl::GmGeom g = {};
        const bool ok = shl::gm_geometry(C, Co, G, Kh, Kw, sh, sw, Ho, Wo, N, g);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %d\n", ok ? 1 : 0, g.nunits, g.nblk, g.upg, g.kc, g.nslab, g.btx, g.bty, g.tiles_x,
               g.tiles_y, g.pw, g.ph, g.row_pitch, g.nslots, (long long)shl::gm_lds_bytes(g), (long long)g.pw_magic,
               shl::gm_default((int64_t)N * Ho * Wo, C, Co, G, Kh * Kw, sh > 1 || sw > 1) ? 1 : 0);
        char name[512];
        snprintf(name, sizeof name, "%s/w%d.bin", argv[2], idx);
        FILE *wf = ok ? fopen(name, "rb") : NULL;
        if (wf) {  // OIHW weights in, fragments + acc_init (zp_in = -5) out
            std::vector<int8_t> w((size_t)Co * (C / G) * Kh * Kw), packed((size_t)shl::gm_weight_bytes(g));
            std::vector<int32_t> acc(Co);
            if (fread(w.data(), 1, w.size(), wf) != w.size()) return 3;
            fclose(wf);
            shl::gm_pack(w.data(), C, Co, G, Kh, Kw, -5, g, packed.data(), acc.data());
            snprintf(name, sizeof name, "%s/p%d.bin", argv[2], idx);
            FILE *pf = fopen(name, "wb");
            if (!pf || fwrite(packed.data(), 1, packed.size(), pf) != packed.size() || fwrite(acc.data(), 4, acc.size(), pf) != acc.size()) return 4;
            fclose(pf);
        }
        ++idx;
    }
    fclose(f);
    return 0;
}
"""

# (C, Cout, G, Kh, Kw, sh, sw, Ho, Wo, N): the shapes of tests/test_group_mfma.py ...
PROBLEMS = [(64, 64, 16, 3, 3, 1, 1, 9, 7, 1), (64, 64, 8, 3, 3, 2, 2, 6, 5, 3), (96, 96, 6, 3, 3, 1, 1, 7, 7, 1), (64, 64, 2, 3, 3, 1, 1, 8, 8, 1),
            (128, 64, 2, 3, 3, 1, 1, 8, 8, 1), (64, 128, 2, 3, 3, 1, 1, 8, 8, 1), (64, 64, 4, 1, 1, 1, 1, 8, 8, 1), (64, 64, 8, 5, 5, 2, 2, 4, 4, 1),
            (32, 32, 8, 3, 3, 1, 1, 40, 40, 2)]
# ... each stride pair for 3x3 and 7x7 on a map of several rectangles, narrow and two wide forms, and the floor of the default rule
PROBLEMS += [(c, co, g, k, k, sh, sw, 57, 43, 2) for k in (3, 7) for (c, co, g) in ((64, 64, 16), (256, 256, 2), (128, 384, 2)) for sh in (1, 2) for sw in (1, 2)]
# ... and the default rule's measured classes (profiles/group_mfma_notes.md); first the layer tests/test_group_conv.py pins
BY_DEFAULT = {(128, 128, 32, 3, 3, 1, 1, 9, 7, 3): 0, (128, 128, 32, 3, 3, 1, 1, 56, 56, 1): 1, (128, 128, 32, 3, 3, 2, 2, 28, 28, 1): 0,
              (128, 128, 32, 3, 3, 2, 2, 28, 28, 32): 1, (256, 256, 32, 3, 3, 2, 2, 14, 14, 1): 0, (512, 512, 32, 3, 3, 2, 2, 7, 7, 1): 1,
              (1024, 1024, 32, 3, 3, 1, 1, 7, 7, 1): 1, (2048, 2048, 32, 3, 3, 1, 1, 7, 7, 32): 1, (128, 128, 8, 3, 3, 1, 1, 28, 28, 1): 1,
              (1024, 1024, 32, 5, 5, 1, 1, 7, 7, 32): 0, (768, 768, 8, 3, 3, 1, 1, 14, 14, 32): 0}
PROBLEMS += list(BY_DEFAULT)
REFUSED = [(192, 192, 96, 3, 3, 1, 1, 8, 8, 1), (32, 64, 8, 3, 3, 1, 1, 8, 8, 1), (48, 48, 4, 3, 3, 1, 1, 8, 8, 1), (64, 64, 1, 3, 3, 1, 1, 8, 8, 1),
           (64, 64, 8, 8, 3, 1, 1, 8, 8, 1), (64, 64, 8, 3, 3, 3, 1, 8, 8, 1), (64, 64, 8, 3, 3, 1, 1, 4, 16 * 65535 + 1, 1), (96, 96, 2, 3, 3, 1, 1, 8, 8, 1)]
PACKED = range(9)  # the problems whose weights go through the packer


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if shutil.which("g++") is None or os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer builds run on machines without a GPU, with a host compiler")
    tmp = tmp_path_factory.mktemp("group_mfma")
    (tmp / "driver.cpp").write_text(DRIVER), (tmp / "problems.txt").write_text("".join(" ".join(map(str, p)) + "\n" for p in PROBLEMS + REFUSED))
    exe = str(tmp / "group_mfma_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(cases.ROOT, "csi-nn2_amd", "csrc"), str(tmp / "driver.cpp"), "-o", exe], check=True)
    weights = {}
    for i in PACKED:
        C, Co, G, Kh, Kw = PROBLEMS[i][:5]
        weights[i] = np.random.default_rng(77 + i).integers(-128, 128, (Co, C // G, Kh * Kw), dtype=np.int8)
        weights[i].tofile(str(tmp / ("w%d.bin" % i)))
    res = subprocess.run([exe, str(tmp / "problems.txt"), str(tmp)], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
    out = [[int(v) for v in ln.split()] for ln in res.stdout.splitlines()]
    assert len(out) == len(PROBLEMS) + len(REFUSED)
    return out, weights, tmp


@pytest.mark.parametrize("i", range(len(PROBLEMS)), ids=["x".join(map(str, p)) for p in PROBLEMS])
def test_geometry_covers_channels_and_map_once_with_its_taps_inside_the_patch(rows, i):
    C, Co, G, Kh, Kw, sh, sw, Ho, Wo, N = PROBLEMS[i]
    ok, nunits, nblk, upg, kc, nslab, btx, bty, tiles_x, tiles_y, pw, ph, row_pitch, nslots, lds, magic, by_default = rows[0][i]
    assert ok == 1 and by_default == BY_DEFAULT.get(PROBLEMS[i], by_default)
    assert nblk in (1, 2, 4) and nunits * nblk * 32 == Co and kc == nslab * 32 and 1 <= btx <= 2 and 1 <= btx * bty <= 16 // nblk
    # every unit's output channels read only their own group, which lies inside the unit's window
    oc, c0 = np.arange(Co), np.arange(Co) // (32 * nblk) // upg * kc
    assert np.all(oc // (Co // G) * (C // G) >= c0) and np.all((oc // (Co // G) + 1) * (C // G) <= c0 + kc) and c0.max() + kc <= C
    # per axis with the kernel's own mapping (workgroup, tile of the rectangle, pixel of the 8 x 4 tile -> output): every output
    # row / column is produced exactly once, and each of its taps lies inside the workgroup's patch
    for extent, b, tiles, span, s, K, p in ((Wo, btx, tiles_x, 8, sw, Kw, pw), (Ho, bty, tiles_y, 4, sh, Kh, ph)):
        wg, tile, px = np.meshgrid(np.arange(tiles), np.arange(b), np.arange(span), indexing="ij")
        out = (wg * b * span + tile * span + px).ravel()
        assert np.array_equal(np.bincount(out[out < extent], minlength=extent), np.ones(extent, np.int64))
        assert ((tile * span + px) * s + K - 1).max() < p
    assert nslots == 2 * pw * ph <= (3 if nslab > 1 else 5) * 256  # the pieces a thread holds in registers
    assert row_pitch % 16 == 0 and row_pitch >= pw * 48 and lds == ph * row_pitch <= 40 * 1024
    j = np.arange(pw * ph, dtype=np.uint64)
    assert np.array_equal((j * np.uint64(magic)) >> np.uint64(32), j // np.uint64(pw))  # the kernel's division by pw
    assert tiles_x <= 65535 and tiles_y * N <= 65535


def test_shapes_outside_the_scope_or_the_grid_are_refused(rows):
    assert [r[0] for r in rows[0][len(PROBLEMS):]] == [0] * len(REFUSED)


@pytest.mark.parametrize("i", PACKED, ids=["x".join(map(str, PROBLEMS[i][:5])) for i in PACKED])
def test_packed_fragments_are_the_zero_filled_window_matrix(rows, i):
    C, Co, G, Kh, Kw = PROBLEMS[i][:5]
    nunits, nblk, upg, kc, nslab = rows[0][i][1:6]
    w, taps, cpg = rows[1][i], Kh * Kw, C // G
    raw = np.fromfile(str(rows[2] / ("p%d.bin" % i)), dtype=np.int8)
    assert raw.size == Co * kc * taps + 4 * Co
    # [unit][block][slab][tap][half][row][16 B] -> [Cout][tap][window channel]
    got = raw[:Co * kc * taps].reshape(nunits, nblk, nslab, taps, 2, 32, 16).transpose(0, 1, 5, 3, 2, 4, 6).reshape(Co, taps, kc)
    full = np.zeros((Co, taps, C), np.int8)  # the dense zero-filled matrix, straight from the OIHW weights
    for oc in range(Co):
        g = oc // (Co // G)
        full[oc, :, g * cpg:(g + 1) * cpg] = w[oc].T
    c0 = np.arange(Co) // (32 * nblk) // upg * kc
    want = np.stack([full[oc, :, c0[oc]:c0[oc] + kc] for oc in range(Co)])
    assert np.array_equal(got, want)
    assert np.array_equal(raw[Co * kc * taps:].view(np.int32), 5 * w.astype(np.int64).sum(axis=(1, 2)))

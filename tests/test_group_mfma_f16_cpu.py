"""The host half of the grouped binary16 matrix-core kernel (csrc/group_mfma_f16.h), no GPU: geometry and the weight packer
compiled into a stand-alone program under AddressSanitizer and UBSan; the packed fragments are unpacked back to OIHW here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases

DRIVER = r"""
#include <stdio.h>
#include <vector>
#include "group_mfma_f16.h"
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    int C, Co, G, Kh, Kw, sh, sw, Ho, Wo, N, idx = 0;
    for (; fscanf(f, "%d %d %d %d %d %d %d %d %d %d", &C, &Co, &G, &Kh, &Kw, &sh, &sw, &Ho, &Wo, &N) == 10; ++idx) {
        shl::GhGeom g = {};
        if (!shl::gh_geometry(C, Co, G, Kh, Kw, sh, sw, Ho, Wo, N, g)) return 3;
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld\n", g.nunits, g.nblk, g.upg, g.kc, g.nslab, g.cpg, g.mvalid, g.tpm,
               g.spslab, g.bpw, g.btx, g.bty, g.tiles_x, g.tiles_y, g.pw, g.ph, g.row_pitch, g.nslots, (long long)shl::gh_lds_bytes(g));
        std::vector<uint16_t> w((size_t)Co * (C / G) * Kh * Kw), packed((size_t)shl::gh_weight_bytes(g) / 2, 0xffff);
        for (size_t i = 0; i < w.size(); ++i) w[i] = (uint16_t)(1 + i % 65535);
        shl::gh_pack(w.data(), C, Co, G, Kh, Kw, g, packed.data());
        char name[512];
        snprintf(name, sizeof name, "%s/p%d.bin", argv[2], idx);
        FILE *pf = fopen(name, "wb");
        if (!pf || fwrite(packed.data(), 2, packed.size(), pf) != packed.size()) return 4;
        fclose(pf);
    }
    return 0;
}
"""

# (C, Cout, G, Kh, Kw, sh, sw, Ho, Wo, N): narrow 4 / 8 / 16, wide with one and two slabs and with two and four blocks, 1x1, 5x5,
# and 7x7 at stride 2 on a map of several rectangles (the LDS and staging bounds)
PROBLEMS = [(32, 32, 8, 3, 3, 1, 1, 9, 7, 1), (64, 64, 8, 3, 3, 2, 2, 6, 5, 3), (96, 96, 6, 3, 3, 1, 1, 7, 7, 1), (64, 64, 2, 3, 3, 1, 1, 8, 8, 1),
            (128, 64, 2, 3, 3, 1, 1, 8, 8, 1), (64, 128, 2, 3, 3, 1, 1, 8, 8, 1), (64, 64, 4, 1, 1, 1, 1, 8, 8, 1), (64, 64, 8, 5, 5, 2, 2, 4, 4, 1)]
PROBLEMS += [(c, co, g, 7, 7, 2, 2, 57, 43, 2) for (c, co, g) in ((64, 64, 16), (64, 64, 4), (256, 256, 2), (128, 384, 2))]


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if shutil.which("g++") is None or os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer builds run on machines without a GPU, with a host compiler")
    tmp = tmp_path_factory.mktemp("group_mfma_f16")
    (tmp / "driver.cpp").write_text(DRIVER), (tmp / "problems.txt").write_text("".join(" ".join(map(str, p)) + "\n" for p in PROBLEMS))
    exe = str(tmp / "group_mfma_f16_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(cases.ROOT, "csi-nn2_amd", "csrc"), str(tmp / "driver.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe, str(tmp / "problems.txt"), str(tmp)], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
    out = [[int(v) for v in ln.split()] for ln in res.stdout.splitlines()]
    assert len(out) == len(PROBLEMS)
    return out, tmp


@pytest.mark.parametrize("i", range(len(PROBLEMS)), ids=["x".join(map(str, p)) for p in PROBLEMS])
def test_geometry_bounds_and_every_weight_once_with_zero_padding(rows, i):
    C, Co, G, Kh, Kw, sh, sw, Ho, Wo, N = PROBLEMS[i]
    nunits, nblk, upg, kc, nslab, cpg_n, mvalid, tpm, spslab, bpw, btx, bty, tiles_x, tiles_y, pw, ph, row_pitch, nslots, lds = rows[0][i]
    cpg, opg, taps, nblocks = C // G, Co // G, Kh * Kw, nunits * nblk
    assert nblk in (2, 4, 8) and bpw == max(1, nblk // 4) and nblocks * mvalid == Co
    # the map is covered, every tap of every tile pixel lies inside the patch, and the patch fits LDS and the staging registers
    assert tiles_x * btx * 8 >= Wo and tiles_y * bty * 2 >= Ho and 1 <= btx * bty <= 8 * max(1, 4 // nblk)
    assert (btx * 8 - 1) * sw + Kw - 1 < pw and (bty * 2 - 1) * sh + Kh - 1 < ph
    assert row_pitch % 16 == 0 and row_pitch >= pw * 80 and lds == ph * row_pitch + 256 <= 48 * 1024
    assert nslots == 4 * pw * ph <= (6 if nslab > 1 else 10) * 256
    assert taps <= spslab * tpm <= 64 and kc == nslab * 32
    # unpack [block][slab][step][lane = (K quarter, row)][8 halves] -> per block a [16 rows][slab][step][K] matrix, and from it OIHW
    raw = np.fromfile(str(rows[1] / ("p%d.bin" % i)), dtype=np.uint16)
    assert raw.size == nblocks * nslab * spslab * 512
    mat = raw.reshape(nblocks, nslab, spslab, 4, 16, 8).transpose(0, 4, 1, 2, 3, 5).reshape(nblocks, 16, nslab, spslab, 32)
    want = (1 + np.arange(Co * cpg * taps) % 65535).astype(np.uint16).reshape(Co, cpg, taps)
    got, seen = np.zeros_like(want), np.zeros(mat.shape, bool)
    for b, m in np.ndindex(nblocks, mvalid):
        oc = (b * opg if cpg_n else b * 16) + m
        if cpg_n:  # K = (tap of the step, channel of the group)
            got[oc] = mat[b, m, 0].reshape(spslab * tpm, cpg)[:taps].T
            seen[b, m, 0].reshape(spslab * tpm, cpg)[:taps] = True
        else:  # K = channel of the slab, the step is the tap
            got[oc] = mat[b, m].transpose(0, 2, 1).reshape(cpg, taps)
            seen[b, m] = True
        grp, c0 = oc // opg, (b // nblk) // upg * kc  # a unit's blocks read only the unit's window
        assert c0 <= grp * cpg and (grp + 1) * cpg <= c0 + kc <= C
    assert np.array_equal(got, want)  # every weight exactly once (blocks x valid rows are the output channels, once each) ...
    assert not mat[~seen].any()       # ... and every padding position is +0

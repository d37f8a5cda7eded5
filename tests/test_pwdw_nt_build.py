"""Build-level guard for the NT forms of the batch-1 pair kernel (pwdw_fused.hip: pwdw_fused_nt_kernel<NSW, KS, NT, EPQ, EPD>).

A window whose tile count NT is no multiple of the wave groups used to run the form that reads the count at run time: a finishing
loop with two row / column divisions, two window tests and a branch per round between the two barriers, where a launch is one
wave's instruction stream (profiles/pwdw_nt_notes.md).  With NT compiled in, that stretch is straight-line code.  This test
disassembles the gfx950 code objects of the built libshl_mi355x.so, in the manner of tests/test_latency_shadow.py (whose helpers it
uses), and checks for every NT instantiation:

  * no s_load and no global_load behind the first MFMA;
  * no backward branch between the two s_barriers (the run-time finishing loop is one);
  * at most 128 VGPRs and no scratch;
  * the first global_load is not later (instruction index) than in the padded form the pair ran before.

CPU only: needs llvm-objdump / llvm-readelf (ROCm's LLVM) and the built library, no GPU.
"""
import os

import pytest

import test_latency_shadow as shadow
from cases import pkg

#  (NSW, KS, NT) of launch_pwdw_fused's SHL_PWDW_NT list x the epilogue flavours (3, 3), (0, 0) and the run-time one
NT_FORMS = [(1, 1, 5), (2, 1, 3), (2, 2, 3)]
FLAVOURS = (3, 0, -1)

# Index (from 0) of the first global_load of the form each NT form replaces -- pwdw_fused_kernel<TPW, NSW, 512, true, KS, TPW, false,
# EPI, EPI> with TPW = ceil(NT / (4 / KS)) -- in the build of the parent commit, same compiler flags (build.py), HIP 7.2: obtained by
# running shadow.first_global_load() on that commit's libshl_mi355x.so.  A bound, not an expectation.
#   (NSW, KS, NT, EPI): index
PARENT_FIRST_LOAD = {
    (1, 1, 5, 3): 38, (1, 1, 5, 0): 38, (1, 1, 5, -1): 38,
    (2, 1, 3, 3): 38, (2, 1, 3, 0): 38, (2, 1, 3, -1): 38,
    (2, 2, 3, 3): 44, (2, 2, 3, 0): 44, (2, 2, 3, -1): 44,
}


def _int(v):
    return "Li%dE" % v if v >= 0 else "Lin%dE" % -v


def nt_name(nsw, ks, nt, epi):
    return "_ZN3shl20pwdw_fused_nt_kernelI%s%s%s%s%sEEvNS_8PwDwArgsE" % (_int(nsw), _int(ks), _int(nt), _int(epi), _int(epi))


CASES = [((nsw, ks, nt, epi), nt_name(nsw, ks, nt, epi)) for nsw, ks, nt in NT_FORMS for epi in FLAVOURS]
assert sorted(k for k, _ in CASES) == sorted(PARENT_FIRST_LOAD)


@pytest.fixture(scope="module")
def nt_build(built, tmp_path_factory):
    if not shadow._tool("llvm-objdump") or not shadow._tool("llvm-readelf"):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    lib = pkg.lib_path("libshl_mi355x.so")
    assert os.path.exists(lib), "libshl_mi355x.so is not built (python csi-nn2_amd/build.py)"
    work = str(tmp_path_factory.mktemp("pwdw_nt"))
    return shadow.disassemble(lib, work), shadow.usage_from_notes(work)


def backward_branches_between_the_barriers(body):
    """(the two barriers' indices, the backward branches between them)"""
    bars = [i for i, ins in enumerate(body) if ins[1] == "s_barrier"]
    assert len(bars) == 2, "the kernel has two barriers (partial sums met; patch written), found %d" % len(bars)
    index_of = {ins[0]: i for i, ins in enumerate(body)}
    back = []
    for i in range(bars[0], bars[1]):
        addr, op, operands, enc = body[i]
        if not shadow._BRANCH.match(op):
            continue
        simm = enc & 0xffff
        simm -= 0x10000 if simm & 0x8000 else 0
        target = index_of.get(addr + 4 + 4 * simm)
        if target is None or target <= i:
            back.append("%d: %s %s" % (i, op, operands))
    return bars, back


@pytest.mark.parametrize("key,name", CASES, ids=["nt" + "_".join(str(v) for v in k) for k, _ in CASES])
def test_nt_form_finishes_straight_line_and_requests_everything_in_the_shadow(nt_build, key, name):
    kernels, usage = nt_build
    assert name in kernels, "NT instantiation missing from the library: " + name
    body = kernels[name]
    bad = shadow.late_loads(body)
    assert not bad, "load after the first MFMA (index %d) in %s:\n  %s" % (shadow.first_compute(body), name, "\n  ".join(bad))
    bars, back = backward_branches_between_the_barriers(body)
    first = shadow.first_global_load(body)
    print("%s: %d instructions, first global_load at %s (parent %d), first MFMA at %d, barriers at %s" %
          (name, len(body), first, PARENT_FIRST_LOAD[key], shadow.first_compute(body), bars))
    assert not back, "backward branch between the barriers %s of %s:\n  %s" % (bars, name, "\n  ".join(back))
    assert first is not None and first <= PARENT_FIRST_LOAD[key], "first global_load of %s at instruction %s, the parent's stood at %d" % (name, first, PARENT_FIRST_LOAD[key])
    assert name in usage, "no register report for " + name
    vgprs, scratch = usage[name]
    assert vgprs <= 128 and scratch == 0, "%s: %d VGPRs, %d bytes of scratch" % (name, vgprs, scratch)

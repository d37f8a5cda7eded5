"""Build-level guard for what stands in front of the fragment loads of the batch-1 pair kernel (pwdw_fused.hip).

At batch 1 a launch lasts as long as one wave's instruction stream plus every memory round trip that nothing overlaps
(profiles/operand_first_notes.md).  The kernel therefore reads everything its prologue needs from ONE block at the front of the
kernel arguments -- two wide scalar loads, one wait -- and requests its weight and pixel fragments right behind it.  The compiler
undoes that silently: a late s_load whose destination lies inside an earlier, still outstanding one forces a second wait, a second
~200-cycle round trip in front of the first fragment load (every compile-time form of the parent commit had it).  This test
disassembles the gfx950 code objects of the built libshl_mi355x.so, in the manner of tests/test_latency_shadow.py (whose helpers
it uses), and checks, for every SHL_PWDW_FIXED production instantiation with the epilogue flavours (3, 3) and (0, 0):

  * no s_load between the first `s_waitcnt lgkmcnt(0)` and the first global_load: one scalar round trip in front of the fragments;
  * the first global_load is not later (instruction index) than in the build of the commit before this work;
  * at most 128 VGPRs and no scratch.

(The stem pair, stemdw_fused.hip, is not covered: its branch-free, wait-once form measured no gain and was not kept --
profiles/operand_first_notes.md.)

CPU only: needs llvm-objdump / llvm-readelf (ROCm's LLVM) and the built library, no GPU.
"""
import os
import re

import pytest

import test_latency_shadow as shadow
from cases import pkg

FLAVOURS = (3, 0)


# Index (from 0) of the first global_load in the build of the parent commit, same compiler flags (build.py), HIP 7.2: obtained by
# running shadow.first_global_load() on that commit's libshl_mi355x.so.  A bound, not an expectation.
#   (NSW, KS, TPW, EMT, EPI): index
PARENT_FIRST_LOAD = {
    (1, 1, 1, 0, 0): 97, (1, 1, 1, 0, 3): 97, (1, 1, 1, 1, 0): 97, (1, 1, 1, 1, 3): 97,
    (1, 1, 2, 0, 0): 97, (1, 1, 2, 0, 3): 97, (1, 1, 2, 1, 0): 97, (1, 1, 2, 1, 3): 97,
    (2, 1, 1, 0, 0): 95, (2, 1, 1, 0, 3): 95, (2, 1, 1, 1, 0): 95, (2, 1, 1, 1, 3): 95,
    (2, 1, 2, 0, 0): 95, (2, 1, 2, 0, 3): 95, (2, 1, 2, 1, 0): 95, (2, 1, 2, 1, 3): 95,
    (2, 2, 1, 0, 0): 99, (2, 2, 1, 0, 3): 100, (2, 2, 1, 1, 0): 100, (2, 2, 1, 1, 3): 100,
    (2, 2, 2, 0, 0): 99, (2, 2, 2, 0, 3): 100, (2, 2, 2, 1, 0): 100, (2, 2, 2, 1, 3): 100,
    (2, 4, 1, 0, 0): 98, (2, 4, 1, 0, 3): 99, (2, 4, 1, 1, 0): 99, (2, 4, 1, 1, 3): 99,
    (2, 4, 2, 0, 0): 98, (2, 4, 2, 0, 3): 99, (2, 4, 2, 1, 0): 99, (2, 4, 2, 1, 3): 99,
    (4, 4, 1, 0, 0): 98, (4, 4, 1, 0, 3): 99, (4, 4, 1, 1, 0): 99, (4, 4, 1, 1, 3): 99,
    (4, 4, 2, 0, 0): 98, (4, 4, 2, 0, 3): 99, (4, 4, 2, 1, 0): 99, (4, 4, 2, 1, 3): 99,
}

PAIR_CASES = [((nsw, ks, tpw, emt, epi), shadow.pwdw_name(nsw, ks, tpw, emt, epi))
              for nsw, ks, tpw in shadow.PWDW_FIXED for emt in (0, 1) for epi in FLAVOURS]
assert sorted(k for k, _ in PAIR_CASES) == sorted(PARENT_FIRST_LOAD)

_LGKM0 = re.compile(r"lgkmcnt\(0\)")
_SLOAD = re.compile(r"^(s_load|s_buffer_load)")


@pytest.fixture(scope="module")
def operand_build(built, tmp_path_factory):
    if not shadow._tool("llvm-objdump") or not shadow._tool("llvm-readelf"):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    lib = pkg.lib_path("libshl_mi355x.so")
    assert os.path.exists(lib), "libshl_mi355x.so is not built (python csi-nn2_amd/build.py)"
    work = str(tmp_path_factory.mktemp("operand_first"))
    return shadow.disassemble(lib, work), shadow.usage_from_notes(work)


def scalar_loads_behind_the_first_wait(body):
    """(index of the first `s_waitcnt lgkmcnt(0)`, index of the first global_load, the s_load instructions between them)"""
    first_load = shadow.first_global_load(body)
    assert first_load is not None, "no global_load in the kernel"
    waits = [i for i, ins in enumerate(body) if ins[1] == "s_waitcnt" and _LGKM0.search(ins[2])]
    assert waits and waits[0] < first_load, "no s_waitcnt lgkmcnt(0) in front of the first global_load (index %d)" % first_load
    late = ["%d: %s %s" % (i, body[i][1], body[i][2]) for i in range(waits[0], first_load) if _SLOAD.match(body[i][1])]
    return waits[0], first_load, late


def check_registers(usage, name):
    assert name in usage, "no register report for " + name
    vgprs, scratch = usage[name]
    assert vgprs <= 128 and scratch == 0, "%s: %d VGPRs, %d bytes of scratch" % (name, vgprs, scratch)


@pytest.mark.parametrize("key,name", PAIR_CASES, ids=["pwdw" + "_".join(str(v) for v in k) for k, _ in PAIR_CASES])
def test_pair_has_one_scalar_round_trip_in_front_of_its_fragments(operand_build, key, name):
    kernels, usage = operand_build
    assert name in kernels, "production instantiation missing from the library: " + name
    body = kernels[name]
    wait, first, late = scalar_loads_behind_the_first_wait(body)
    print("%s: first s_waitcnt lgkmcnt(0) at %d, first global_load at %d (parent %d), %d instructions" %
          (name, wait, first, PARENT_FIRST_LOAD[key], len(body)))
    assert not late, "a second scalar round trip in front of the first global_load (index %d) of %s:\n  %s" % (first, name, "\n  ".join(late))
    assert first <= PARENT_FIRST_LOAD[key], "first global_load of %s at instruction %d, the parent's stood at %d" % (name, first, PARENT_FIRST_LOAD[key])
    check_registers(usage, name)

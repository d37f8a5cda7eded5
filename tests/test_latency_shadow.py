"""Build-level guard for the batch-1 latency kernels (pwdw_fused.hip, conv1x1_latency.hip, conv_gemv.hip).

At batch 1 a launch lasts as long as one wave's instruction stream plus every memory round trip that nothing overlaps
(profiles/r06_notes.md, profiles/latency_shadow_notes.md).  These kernels therefore request every constant -- kernel arguments
(s_load) and epilogue / depthwise tables (global_load) -- BEFORE the first MFMA or dot product, in the shadow of the fragment
loads' latency.  The compiler undoes that silently whenever a conditional exit or a late first use lets it sink a load into the
block behind the barriers, so this test disassembles the gfx950 code objects of the built libshl_mi355x.so and checks, for every
production instantiation:

  * no s_load and no global_load / buffer_load between the first MFMA / dot-product instruction and the end of the kernel
    (except inside the loop that contains that first compute instruction itself: the GEMV's weight stream);
  * the first global_load is not later (instruction index) than in the build of the commit before the shadow work;
  * at most 128 VGPRs and no scratch (the forms are __launch_bounds__(512)).

CPU only: needs llvm-objdump (ROCm's LLVM) and the built library, no GPU.
"""
import os
import re
import shutil
import subprocess

import pytest

from cases import pkg

LLVM_BIN = "/opt/rocm/llvm/bin"


def _tool(name):
    p = os.path.join(LLVM_BIN, name)
    return p if os.path.exists(p) else shutil.which(name)


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


# ---- the production instantiations, by mangled name ------------------------------------------------------------------------
# pwdw_fused.hip: SHL_PWDW_FIXED(NSW, KS, TPW) x (exact tile count or not) x the two epilogue flavours whole models come in
PWDW_FIXED = [(4, 4, 2), (4, 4, 1), (2, 4, 2), (2, 4, 1), (2, 2, 2), (2, 2, 1), (2, 1, 1), (2, 1, 2), (1, 1, 1), (1, 1, 2)]


def pwdw_name(nsw, ks, tpw, emt, epi):
    return "_ZN3shl17pwdw_fused_kernelILi%dELi%dELi512ELb1ELi%dELi%dELb%dELi%dELi%dEEEvNS_8PwDwArgsE" % (tpw, nsw, ks, tpw, emt, epi, epi)


def lat_name(nsw, mt, epi, pool):
    return "_ZN3shl22conv1x1_latency_kernelILi%dELi%dELi%dELb%dEEEvNS_8ConvArgsENS_11LatPoolArgsE" % (nsw, mt, epi, pool)


def gemv_name(i8, opw):
    return "_ZN3shl16conv_gemv_kernelILb%dELi%dEEEvNS_8ConvArgsE" % (i8, opw)


# Index of the first global_load in the build of the parent commit (the last one before the constants moved into the shadow),
# same compiler flags (build.py), HIP 7.2: obtained by running first_global_load() below on that commit's libshl_mi355x.so.
# A bound, not an expectation: the loads the MFMAs wait for must never start later than they did then.
PWDW_BOUND = {
    # (NSW, KS, TPW, EMT, EPI): index
    (4, 4, 2, 0, 3): 128,
    (4, 4, 2, 0, 0): 128,
    (4, 4, 2, 1, 3): 128,
    (4, 4, 2, 1, 0): 128,
    (4, 4, 1, 0, 3): 117,
    (4, 4, 1, 0, 0): 117,
    (4, 4, 1, 1, 3): 117,
    (4, 4, 1, 1, 0): 117,
    (2, 4, 2, 0, 3): 124,
    (2, 4, 2, 0, 0): 124,
    (2, 4, 2, 1, 3): 124,
    (2, 4, 2, 1, 0): 124,
    (2, 4, 1, 0, 3): 119,
    (2, 4, 1, 0, 0): 119,
    (2, 4, 1, 1, 3): 119,
    (2, 4, 1, 1, 0): 119,
    (2, 2, 2, 0, 3): 126,
    (2, 2, 2, 0, 0): 126,
    (2, 2, 2, 1, 3): 126,
    (2, 2, 2, 1, 0): 126,
    (2, 2, 1, 0, 3): 119,
    (2, 2, 1, 0, 0): 119,
    (2, 2, 1, 1, 3): 119,
    (2, 2, 1, 1, 0): 119,
    (2, 1, 1, 0, 3): 112,
    (2, 1, 1, 0, 0): 112,
    (2, 1, 1, 1, 3): 112,
    (2, 1, 1, 1, 0): 112,
    (2, 1, 2, 0, 3): 118,
    (2, 1, 2, 0, 0): 118,
    (2, 1, 2, 1, 3): 118,
    (2, 1, 2, 1, 0): 118,
    (1, 1, 1, 0, 3): 114,
    (1, 1, 1, 0, 0): 99,
    (1, 1, 1, 1, 3): 99,
    (1, 1, 1, 1, 0): 99,
    (1, 1, 2, 0, 3): 130,
    (1, 1, 2, 0, 0): 130,
    (1, 1, 2, 1, 3): 130,
    (1, 1, 2, 1, 0): 130,
}
LAT_BOUND = {
    # (NSW, MT, EPI, POOL): index
    (1, 1, 3, 0): 21,
    (1, 1, 3, 1): 19,
    (1, 1, 0, 0): 21,
    (1, 1, 0, 1): 19,
    (1, 2, 3, 0): 19,
    (1, 2, 3, 1): 19,
    (1, 2, 0, 0): 19,
    (1, 2, 0, 1): 19,
    (2, 1, 3, 0): 30,
    (2, 1, 3, 1): 30,
    (2, 1, 0, 0): 30,
    (2, 1, 0, 1): 30,
    (2, 2, 3, 0): 37,
    (2, 2, 3, 1): 42,
    (2, 2, 0, 0): 37,
    (2, 2, 0, 1): 42,
    (4, 1, 3, 0): 23,
    (4, 1, 3, 1): 25,
    (4, 1, 0, 0): 23,
    (4, 1, 0, 1): 25,
    (4, 2, 3, 0): 33,
    (4, 2, 3, 1): 38,
    (4, 2, 0, 0): 33,
    (4, 2, 0, 1): 38,
}
GEMV_BOUND = {
    # (int8, OPW): index
    (1, 2): 48,
    (1, 4): 86,
    (0, 2): 50,
    (0, 4): 80,
}

CASES = [("pwdw", k, pwdw_name(*k)) for k in sorted(PWDW_BOUND)] + [("lat", k, lat_name(*k)) for k in sorted(LAT_BOUND)] + \
    [("gemv", k, gemv_name(*k)) for k in sorted(GEMV_BOUND)]
BOUNDS = {"pwdw": PWDW_BOUND, "lat": LAT_BOUND, "gemv": GEMV_BOUND}


# ---- disassembly -----------------------------------------------------------------------------------------------------------
_INS = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):\s*([0-9A-Fa-f]{8})")
_SYM = re.compile(r"^[0-9a-f]+ <(\S+)>:")


def disassemble(lib, workdir):
    """{kernel symbol: [(address, mnemonic, operands, first encoding dword)]} of every gfx950 code object in `lib`"""
    objdump = _tool("llvm-objdump")
    local = os.path.join(workdir, "lib.so")
    shutil.copy(lib, local)
    subprocess.run([objdump, "--offloading", "lib.so"], cwd=workdir, check=True, stdout=subprocess.DEVNULL)
    kernels = {}
    for f in sorted(os.listdir(workdir)):
        if "gfx950" not in f:
            continue
        out = subprocess.run([objdump, "-d", os.path.join(workdir, f)], check=True, capture_output=True, text=True).stdout
        name = None
        for ln in out.splitlines():
            m = _SYM.match(ln)
            if m:
                name = m.group(1)
                kernels[name] = []
                continue
            m = _INS.match(ln)
            if m and name is not None:
                if m.group(1) == "s_code_end":
                    continue
                kernels[name].append((int(m.group(3), 16), m.group(1), m.group(2), int(m.group(4), 16)))
    return kernels


_COMPUTE = re.compile(r"^(v_mfma|v_smfmac|v_dot\d|v_cvt_f32_f16)")  # MFMA; int8 dot product; the binary16 GEMV's widening
_LOAD = re.compile(r"^(s_load|s_buffer_load|global_load|buffer_load|flat_load|scratch_load)")
_VLOAD = re.compile(r"^(global_load|buffer_load|flat_load)")
_BRANCH = re.compile(r"^(s_branch|s_cbranch)")


def first_compute(body):
    for i, ins in enumerate(body):
        if _COMPUTE.match(ins[1]):
            return i
    return None


def first_global_load(body):
    for i, ins in enumerate(body):
        if _VLOAD.match(ins[1]):
            return i
    return None


def compute_loops(body):
    """[(first, last)] instruction index ranges of backward branches whose body contains a compute instruction"""
    index_of = {ins[0]: i for i, ins in enumerate(body)}
    loops = []
    for i, (addr, op, _, enc) in enumerate(body):
        if not _BRANCH.match(op):
            continue
        simm = enc & 0xffff
        simm -= 0x10000 if simm & 0x8000 else 0
        target = index_of.get(addr + 4 + 4 * simm)
        if target is not None and target <= i and any(_COMPUTE.match(b[1]) for b in body[target:i + 1]):
            loops.append((target, i))
    return loops


def late_loads(body):
    """loads behind the first compute instruction that are not part of a loop around compute instructions"""
    start = first_compute(body)
    assert start is not None, "no MFMA / dot product in the kernel"
    loops = [(a, b) for a, b in compute_loops(body) if a <= start <= b]  # only the loop the first compute instruction itself is in
    bad = []
    for i in range(start + 1, len(body)):
        if _LOAD.match(body[i][1]) and not any(a <= i <= b for a, b in loops):
            bad.append("%d: %s %s" % (i, body[i][1], body[i][2]))
    return bad


# ---- registers and scratch -------------------------------------------------------------------------------------------------
def usage_from_reports(objdir):
    """{kernel symbol: (vgprs, scratch bytes)} from the <source>.usage.txt files build.py writes next to the objects"""
    res = {}
    if not os.path.isdir(objdir):
        return res
    for f in ("pwdw_fused", "conv1x1_latency", "conv_gemv"):
        path = os.path.join(objdir, f + ".usage.txt")
        if not os.path.exists(path):
            continue
        name, vg = None, None
        for ln in open(path):
            if "Function Name:" in ln:
                name = ln.split("Function Name:")[1].split("[")[0].strip()
            elif " VGPRs:" in ln:
                vg = int(ln.split("VGPRs:")[1].split("[")[0])
            elif "ScratchSize [bytes/lane]:" in ln:
                res[name] = (vg, int(ln.split("ScratchSize [bytes/lane]:")[1].split("[")[0]))
    return res


def usage_from_notes(workdir):
    """the same from the code objects' metadata (a tree whose objects were not kept: only the library travels)"""
    readelf = _tool("llvm-readelf")
    res = {}
    if not readelf:
        return res
    for f in sorted(os.listdir(workdir)):
        if "gfx950" not in f:
            continue
        out = subprocess.run([readelf, "--notes", os.path.join(workdir, f)], check=True, capture_output=True, text=True).stdout
        for block in out.split("- .agpr_count:")[1:]:
            sym = re.search(r"\.symbol:\s+(\S+)\.kd", block)
            vg = re.search(r"\.vgpr_count:\s+(\d+)", block)
            sc = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
            if sym and vg and sc:
                res[sym.group(1)] = (int(vg.group(1)), int(sc.group(1)))
    return res


@pytest.fixture(scope="module")
def shadow_build(built, tmp_path_factory):
    if not _hipcc() or not _tool("llvm-objdump"):
        pytest.skip("hipcc / llvm-objdump not available")
    lib = pkg.lib_path("libshl_mi355x.so")
    assert os.path.exists(lib), "libshl_mi355x.so is not built (python csi-nn2_amd/build.py)"
    work = str(tmp_path_factory.mktemp("shadow"))
    kernels = disassemble(lib, work)
    usage = usage_from_reports(os.path.join(pkg.LIB_DIR, "obj"))
    if not all(name in usage for _, _, name in CASES):
        usage = usage_from_notes(work)
    return kernels, usage


@pytest.mark.parametrize("family,key,name", CASES, ids=["%s%s" % (f, "_".join(str(int(v)) for v in k)) for f, k, _ in CASES])
def test_constants_are_requested_in_the_shadow(shadow_build, family, key, name):
    kernels, usage = shadow_build
    assert name in kernels, "production instantiation missing from the library: " + name
    body = kernels[name]
    bad = late_loads(body)
    assert not bad, "load after the first MFMA / dot product (index %d) in %s:\n  %s" % (first_compute(body), name, "\n  ".join(bad))
    first = first_global_load(body)
    bound = BOUNDS[family][key]
    assert first is not None and first <= bound, "first global_load of %s at instruction %s, the bound is %d" % (name, first, bound)
    assert name in usage, "no register report for " + name
    vgprs, scratch = usage[name]
    assert vgprs <= 128 and scratch == 0, "%s: %d VGPRs, %d bytes of scratch" % (name, vgprs, scratch)

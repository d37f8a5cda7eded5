"""Golden vectors for matmul -- csinn_matmul, batched, both transposes, the "dense" broadcast -- from the GENUINE reference
(oracle/_ref).

    python tests/golden/make_matmul_golden.py   ->  tests/golden/matmul_cases.npz, matmul_op_ids.json
Layer mode on CSINN_REF through csinn_matmul_init + csinn_matmul (source/reference/matmul.c:134-138).  Inputs are regenerated
by matmul_cases.all_cases(); only the outputs are stored (binary16 outputs as their bit patterns: some hold NaNs).  Every case
runs twice and must give the same bits.  matmul_op_ids.json holds the op id and the layout of struct csinn_matmul_params as the
genuine headers give them.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cases  # noqa: E402
import matmul_cases as mc  # noqa: E402
from cases import pkg  # noqa: E402

FIELDS = ("trans_a", "trans_b")


def probe_source():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "csi_nn.h"', 'int main(void)', '{', '    printf("{");',
             '    printf("\\"CSINN_OP_MATMUL\\": %d, ", (int)CSINN_OP_MATMUL);']
    for f in FIELDS:
        lines.append('    printf("\\"offsetof csinn_matmul_params.%s\\": %%zu, ", offsetof(struct csinn_matmul_params, %s));' % (f, f))
    lines.append('    printf("\\"sizeof csinn_matmul_params\\": %zu", sizeof(struct csinn_matmul_params));')
    lines += ['    printf("}\\n");', '    return 0;', '}', '']
    return "\n".join(lines)


def measure(include_dirs):
    """the op id and the params block's layout as the headers under `include_dirs` give them"""
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        open(src, "w").write(probe_source())
        subprocess.run(["gcc", "-std=gnu99", "-w", src, "-o", exe] + ["-I" + d for d in include_dirs], check=True)
        return json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)


def reference_checkout():
    """where csi-nn2_amd/build.py looks for the reference's sources"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("build", os.path.join(cases.ROOT, "csi-nn2_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.REFERENCE


def main():
    ref = os.path.join(reference_checkout(), "include")
    ids = measure([ref, ref + "/csinn"])
    json.dump(ids, open(os.path.join(HERE, "matmul_op_ids.json"), "w"), sort_keys=True)
    print(ids)
    fe = cases.load_reference_frontend()
    fe.shl_debug_set_level(1)  # errors only: the library warns about every binary16 saturation
    blob = {}
    for case in mc.all_cases():
        out = mc.layer_run(fe, pkg.API_REF, case)
        again = mc.layer_run(fe, pkg.API_REF, case)
        assert np.array_equal(mc.bits(out), mc.bits(again)), "not reproducible: " + mc.case_id(case)
        blob[mc.golden_key(case)] = mc.bits(out)
    path = os.path.join(HERE, "matmul_cases.npz")
    np.savez_compressed(path, **blob)
    print("wrote %d cases to %s (%d bytes)" % (len(blob), path, os.path.getsize(path)))


if __name__ == "__main__":
    main()

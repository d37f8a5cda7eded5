"""Golden results for the binary16 special-value cases of tests/tail_sweeps.py (families gap, softmax and add: inf, NaN,
signed zeros, +-65504, ties and subnormal sums), produced by the GENUINE reference (oracle/_ref/libshl_ref_x86.so, built
from the reference's sources by oracle/Makefile.ref) in layer mode on CSINN_REF.

    python tests/golden/make_tail_sweep_golden.py      ->  tests/golden/tail_sweep_specials.npz

Per case: a CRC of the operands (the draw must not drift), a CRC of the whole result and the result's words at the planted
elements (tail_sweeps.specials) -- NaN as 0x7E00 throughout, the sign of a NaN is the host's.  "seed" is the seed of the
draws: the test that reads this file draws with it whatever SHL_TEST_FUZZ_SEED says.
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cases  # noqa: E402
import tail  # noqa: E402
import tail_sweeps as ts  # noqa: E402
from cases import pkg  # noqa: E402


def operands_crc(case):
    crc = zlib.crc32(np.ascontiguousarray(case["x"]).tobytes())
    return zlib.crc32(np.ascontiguousarray(case["y"]).tobytes(), crc) if "y" in case else crc


def record(case, out):
    words = ts.canonical_f16(out)
    return {case["name"] + "/x_crc": np.uint32(operands_crc(case)),
            case["name"] + "/out_crc": np.uint32(zlib.crc32(words.tobytes())),
            case["name"] + "/out": words[ts.specials(case)]}


def main():
    fe = cases.load_reference_frontend()
    blob = {"seed": np.int64(ts.BASE_SEED)}
    for fam, i in ts.special_cases():
        case = ts.build(fam, i)
        out = tail.siso_run(fe, pkg.API_REF, case)
        blob.update(record(case, out))
        print("%-12s %-28s %d planted words" % (case["name"], str(out.shape), ts.specials(case).size))
    path = os.path.join(HERE, "tail_sweep_specials.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""attention_sweeps.all_cases() on the GPU (-m gpu), no form variable set.  Per case:
  (a) the fused launch equals the device's own matmul (mfma form) -> mul -> softmax -> matmul (mfma form) on the same -- for
      the unaligned stratum: the same off-grid -- pointers bit for bit, and leaves the poisoned bytes around its output alone;
  (b) int8: the unfused scores equal matmul_cases.exact_ref of Q K^T bit for bit;
  (c) int8: the fused output equals attention_cases.device_formula bit for bit WHETHER OR NOT the plan-time proof holds: the
      formula is the exact CPU statement of what the mfma form computes, so outside the proof (every default-class case under
      p's usual record: 255 x 128 x 768 > 2^24) nothing is left to a gate.  Where that fails, the device's own intermediates
      say which layer differs;
  (d) int8 against the oracle chain: bit for bit inside the proof, inside DESIGN's gate outside it;
  (e) binary16 against the oracle chain inside the project's 1e-3 gate."""
import numpy as np
import pytest

import attention_cases as ac
import attention_sweeps as sw
import cases
import eltwise_cases
import matmul_cases as mc
import tail
from cases import pkg

CASES = sw.all_cases()
IDS = [sw.case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return hip, cases.HipDevice(hip)


def _differing(got, want):
    return int(np.count_nonzero(mc.bits(got) != mc.bits(want)))


def layers_that_differ(c, scores, x_in, p, chain):
    """int8: every unfused layer of the device against the CPU statement of that layer ON THE DEVICE'S OWN INPUT, so that a
    difference is the layer's and not an earlier one's: {layer: outputs that differ}"""
    out = {"q k^T": _differing(scores, mc.exact_ref(ac._qk_case(c)))}
    x_q = c["s_q"]
    if c["has_scale"]:
        want = eltwise_cases.eltwise_numpy(dict(op="mul", dtype="int8", x=scores, y=c["c"], in_q=c["s_q"], in1_q=c["c_q"], out_q=c["sc_q"],
                                                small_first=c["scale_first"]))
        out["mul"], x_q = _differing(x_in, want), c["sc_q"]
    want = tail.siso_oracle(dict(kind="softmax", x=x_in, dtype="int8", layout="NCHW", axis=2, in_q=x_q, out_q=c["p_q"]))
    out["softmax"] = _differing(p, want)
    out["p v"] = _differing(chain, mc.exact_ref(ac._pv_case(c, p)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_equals_the_unfused_calls_the_exact_formula_and_the_oracle_chain(gpu, case, monkeypatch):
    hip, dev = gpu
    for var in ("SHL_MI355X_MATMUL_FORM", "SHL_MI355X_MUL_FORM", "SHL_MI355X_SOFTMAX_SEQ"):
        monkeypatch.delenv(var, raising=False)
    name = sw.case_id(case)
    fused, chain, p, scores, x_in = ac.run_both(hip, dev, case)
    mc.assert_same(fused, chain, name + ": fused vs matmul, mul, softmax, matmul")  # (a)
    want = ac.oracle_chain(case)
    if case["dtype"] != "int8":
        mc.assert_f16_gate(fused, want["out"], name + ": fused vs the oracle chain")  # (e)
        return
    formula = ac.device_formula(case)
    mc.assert_same(scores, formula["s"], name + ": the unfused scores vs the exact Q K^T")  # (b)
    differing = _differing(fused, formula["out"])
    assert differing == 0, "%s: %d outputs of the fused launch differ from the mfma form's exact formula; per unfused layer on the " \
        "device's own input: %r" % (name, differing, layers_that_differ(case, scores, x_in, p, chain))  # (c)
    if ac.both_exact(case):  # (d)
        mc.assert_same(p, want["p"], name + ": the unfused probabilities vs the oracle chain")
        mc.assert_same(fused, want["out"], name + ": fused vs the oracle chain")
    else:
        mc.assert_within_gate(fused, want["out"], name + ": fused vs the oracle chain")

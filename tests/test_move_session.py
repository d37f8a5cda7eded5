"""Transpose, pad, reshape and flatten inside a session (-m gpu): a classifier tail (global_avgpool2d -> flatten or reshape ->
fullyconnected), a TensorFlow stride-2 block (pad 0 / 1 -> depthwise 3x3 stride 2 without padding) and a detection head
(reshape -> transpose -> sigmoid) from move_cases.py stay device-resident, are captured as one hipGraph and match the oracle
chain (convolutions and fullyconnected through the C oracle, everything else through the numpy restatements): int8 bit for
bit, binary16 within 1e-3.  The fusion planner takes the same decisions as on the same graph without the four layer kinds.
The transposed tensor of the head is a graph output that may be bound to a buffer the caller keeps in HBM.  Also behind the
genuine front-end and graph executor."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import move_cases as mc
from cases import pkg
from test_concat_session import matches, planner_counts


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", [("int8", "NHWC"), ("f16", "NCHW")])
@pytest.mark.parametrize("which", sorted(mc.NETS))
def test_network_runs_device_resident_and_matches_the_oracle_chain(gpu, which, dtype, layout):
    fe, hip, opt = gpu
    net = mc.NETS[which](dtype, layout)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    for k in (0, 1, 0):  # the graph replay reads fresh data
        x = net.input(k)
        got, want = net.run(fe, x), net.oracle(x)
        for name in net.outputs:
            assert got[name].shape == want[name].shape
            assert matches(got[name], want[name], dtype), "%s %s %s input %d: output %s differs from the oracle chain" % (
                which, dtype, layout, k, name)
    o0, o1 = net.oracle(net.input(0)), net.oracle(net.input(1))
    for name in net.outputs:
        assert not np.array_equal(o0[name], o1[name]), "the two inputs must tell runs apart"
    # what the planner folds and fuses is what it folds and fuses in the same graph without the four layer kinds (each one's
    # input a graph output, its output a graph input): they neither hide a consumer nor add one
    bare = mc.NETS[which](dtype, layout, cut=True)
    bare_sess = bare.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(bare_sess) >= 1
    assert bare.layer_count == net.layer_count - mc.CUT_LAYERS[which]
    want_counts = planner_counts(opt, bare_sess)
    assert want_counts[0] >= 1, "the graph holds a conv -> relu pair that folds"
    assert planner_counts(opt, sess) == want_counts
    bare.close(fe)
    net.close(fe)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", [("int8", "NHWC"), ("f16", "NCHW")])
def test_the_transposed_tensor_bound_to_the_callers_hbm_buffer_is_written_in_place(gpu, dtype, layout):
    """the transposed tensor of the detection head is a graph output (and feeds the sigmoid): first fetched through host
    buffers, then bound to a buffer in HBM -- the graph is captured again around it -- with the other output still coming
    back through the host, then unbound again"""
    fe, hip, opt = gpu
    net = mc.detection_head(dtype, layout)
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2
    dev = cases.HipDevice(hip)
    x0, x1 = net.input(0), net.input(1)
    want0, want1 = net.oracle(x0), net.oracle(x1)
    got = net.run(fe, x0)
    assert matches(got["prob"], want0["prob"], dtype) and matches(got["moved"], want0["moved"], dtype), "host run"
    dt = pkg.DTYPE_INT8 if dtype == "int8" else pkg.DTYPE_FLOAT16
    act_l = pkg.LAYOUT_NHWC if layout == "NHWC" else pkg.LAYOUT_NCHW
    m = want1["moved"]
    d_m = dev.alloc(m.nbytes)
    dev.upload(d_m, np.full(m.nbytes, 0x5A, np.uint8))
    keep = pkg.Keep()
    fe.csinn_update_output(1, pkg.make_tensor(fe, keep, m.shape, dt, act_l, sess=sess, device_ptr=d_m), sess)
    host_out = np.zeros_like(want1["prob"])
    fe.csinn_update_output(0, pkg.make_tensor(fe, keep, host_out.shape, dt, act_l, data=host_out, sess=sess), sess)
    q = net.rec("data")
    for x, want in ((x1, want1), (x0, want0), (x1, want1)):
        fe.csinn_update_input(0, pkg.make_tensor(fe, keep, x.shape, dt, act_l, data=x, sess=sess, scales=(q[0],), zps=(q[1],)), sess)
        assert fe.csinn_session_run(sess) == pkg.CSINN_TRUE
        assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "captured again around the caller's buffer"
        pkg.check(hip.shl_mi355x_stream_sync(opt.shl_mi355x_session_stream(sess)), hip, "sync")
        assert matches(dev.download(d_m, m.shape, m.dtype), want["moved"], dtype), "the transposed tensor, in place in HBM"
        assert matches(host_out, want["prob"], dtype), "the other output, through the host"
    # unbound again: both outputs come back through the host
    host_m = np.zeros_like(m)
    fe.csinn_update_output(1, pkg.make_tensor(fe, keep, m.shape, dt, act_l, data=host_m, sess=sess), sess)
    fe.csinn_update_input(0, pkg.make_tensor(fe, keep, x0.shape, dt, act_l, data=x0, sess=sess, scales=(q[0],), zps=(q[1],)), sess)
    assert fe.csinn_session_run(sess) == pkg.CSINN_TRUE
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2
    assert matches(host_m, want0["moved"], dtype) and matches(host_out, want0["prob"], dtype), "after unbinding"
    dev.free(d_m)
    net.close(fe)


DROPIN = r"""
import sys
sys.path.insert(0, %(tests)r)
import numpy as np
import cases, move_cases as mc
from cases import pkg
fe = cases.load_reference_frontend()          # genuine libshl_ref_x86.so: its own gref builds the graph
hip, opt = pkg.load_backend(fe)
bad = 0
for which in sorted(mc.NETS):
    for dtype, layout in (("int8", "NHWC"), ("f16", "NCHW")):
        net = mc.NETS[which](dtype, layout)
        sess = net.build(fe, pkg.API_MI355X)
        mode = opt.shl_mi355x_session_is_device_resident(sess)
        for k in range(2):
            x = net.input(k)
            want, got = net.oracle(x), net.run(fe, x)
            for name in net.outputs:
                g, w = got[name], want[name]
                if dtype == "int8":
                    ok = bool(np.array_equal(g, w))
                else:
                    ok = bool(np.all(np.abs(g.astype(np.float32) - w.astype(np.float32)) <= 1e-3 * np.maximum(np.abs(w.astype(np.float32)), 1e-3)))
                print(which, dtype, layout, "input", k, "output", name, "device mode", mode, "ok", ok)
                bad += int(not ok) + int(mode != 2)
print("MOVENETS_OK" if bad == 0 else "MOVENETS_FAIL")
"""


@pytest.mark.gpu
@pytest.mark.skipif(not cases.have_reference(), reason="oracle/_ref/libshl_ref_x86.so not present")
def test_networks_drop_in_behind_the_genuine_graph_executor(gpu):
    """The reference's csinn_transpose / _reshape / _flatten / _pad and its gref record the layers; the backend's callbacks
    run them device-resident (one that fell through to the C reference would drop the whole session to the host path:
    mode 0)."""
    code = DROPIN % dict(tests=os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "MOVENETS_OK" in res.stdout, res.stdout + res.stderr

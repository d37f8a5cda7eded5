"""What a device-resident session plans (source/mi355x_opt/session.c:plan_fusion) and what it then enqueues, on three
small int8 NHWC graphs at batch 1 where folding an activation and merging two layers meet, or where a second consumer
forbids both.  Each graph is set up twice in one process -- device-resident, and host-staged layer by layer under
SHL_MI355X_HOST_SESSION=1 (read per setup) -- and the two runs must agree bit for bit, with each other and with the oracle
chain (exact scales throughout: the oracle's fp32 arithmetic has no rounding to disagree about).  The three planner
counters and residency mode 2 are pinned, so a plan that skipped or ran a layer twice shows up either in the counters
or in the bytes."""
import numpy as np
import pytest

import cases
import tail
from cases import pkg
from test_fusion import PWDW_PAIRS, make_pwdw
from test_tail import CONV_POOL


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt


def rec(case):
    return (float(np.float32(case["out_scale"])), int(case["out_zp"]))


def follow(case, prev):
    """`case` reads what `prev` writes: its input record is prev's output record"""
    case["in_scale"], case["in_zp"] = prev["out_scale"], prev["out_zp"]
    case["b_scale"] = (np.float32(case["in_scale"]) * case["k_scale"]).astype(np.float32)
    return case


class Graph:
    """layers: (kind, name, names of the tensors it reads, info) in execution order; a layer's output tensor carries the
    layer's name, the graph input is "data", the graph output is the last layer's.
      conv     info = a cases.make_case dict with act 0 (csinn_conv2d)
      relu     info = its output record (the record of the tensor it reads is that tensor's own)
      add / pool (global_avgpool2d) / softmax    likewise"""

    dtype, layout = "int8", "NHWC"

    def __init__(self, in_shape, q_in, layers, seed):
        self.in_shape, self.q_in, self.layers, self.seed = tuple(in_shape), q_in, layers, seed

    def input(self, k):
        return np.random.default_rng(self.seed + k).integers(-100, 100, self.in_shape, dtype=np.int8)

    def _shapes_and_records(self):
        shape, q = {"data": self.in_shape}, {"data": self.q_in}
        for kind, name, src, info in self.layers:
            s = shape[src[0]]
            shape[name] = info["out_shape"] if kind == "conv" else (s[0], 1, 1, s[3]) if kind == "pool" else s
            q[name] = rec(info) if kind == "conv" else info
        return shape, q

    def oracle(self, x):
        _, q = self._shapes_and_records()
        val = {"data": x}
        for kind, name, src, info in self.layers:
            if kind == "conv":
                case = dict(info)
                case["input"] = np.ascontiguousarray(val[src[0]])
                val[name] = cases.oracle_run(case, "ref")
                continue
            c = dict(kind=kind, x=val[src[0]], dtype="int8", layout="NHWC", axis=3, in_q=q[src[0]], out_q=q[name])
            if kind == "add":
                c.update(y=val[src[1]], in1_q=q[src[1]])
            val[name] = tail.siso_oracle(c)
        return val[self.layers[-1][1]]

    def build(self, fe, api):
        keep = pkg.Keep()
        sess = fe.csinn_alloc_session()
        sc = sess.contents
        sc.base_api, sc.base_run_mode, sc.base_dtype = api, pkg.RM_CPU_GRAPH, pkg.DTYPE_INT8
        sc.base_quant_type = pkg.QUANT_INT8_ASYM_W_SYM
        sc.debug_level = 0
        fe.csinn_session_init(sess)
        fe.csinn_set_input_number(1, sess)
        fe.csinn_set_output_number(1, sess)
        shape, q = self._shapes_and_records()
        act_l = pkg.LAYOUT_NHWC

        def T(dims, scales, zps, name, data=None, const=0, layout=act_l, dtype=pkg.DTYPE_INT8):
            return pkg.make_tensor(fe, keep, dims, dtype, layout, data=data, is_const=const, name=name, sess=sess,
                                   scales=scales, zps=zps)
        t = {"data": T(self.in_shape, (self.q_in[0],), (self.q_in[1],), b"data")}
        ops = []
        for kind, name, src, info in self.layers:
            nm = name.encode()
            t[name] = T(shape[name], (q[name][0],), (q[name][1],), nm + b"_out")
            if kind == "conv":
                case = info
                assert case["act"] == 0 and tuple(case["in_shape"]) == tuple(shape[src[0]]), name
                assert (float(np.float32(case["in_scale"])), int(case["in_zp"])) == q[src[0]], name
                t_w = T(case["w_shape"], tuple(case["k_scale"]), tuple(case["k_zp"]), nm + b"_w", case["kernel"], 1,
                        pkg.LAYOUT_1HWO if case["depthwise"] else pkg.LAYOUT_OHWI)
                t_b = T((case["co"],), tuple(case["b_scale"]), (0,), nm + b"_b", case["bias"], 1, pkg.LAYOUT_O, pkg.DTYPE_INT32)
                p = pkg.conv_params(fe, keep, api, act_l, case["stride"], case["pad"], case["dilation"], case["group"], 0,
                                    sess, nm)
                ops.append(("csinn_conv2d", (t[src[0]], t[name], t_w, t_b, p)))
            elif kind == "add":
                p = pkg.siso_params(fe, keep, api, "add", act_l, 1, sess, nm)
                ops.append(("csinn_add", (t[src[0]], t[src[1]], t[name], p)))
            else:
                p = pkg.siso_params(fe, keep, api, kind, act_l, 3, sess, nm)
                stem = {"relu": "csinn_relu", "pool": "csinn_global_avgpool2d", "softmax": "csinn_softmax"}[kind]
                ops.append((stem, (t[src[0]], t[name], p)))
        for stem, args in ops:
            assert getattr(fe, stem + "_init")(*args) == pkg.CSINN_TRUE, stem
        fe.csinn_set_tensor_entry(t["data"], sess)
        fe.csinn_set_input(0, t["data"], sess)
        for stem, args in ops:
            assert getattr(fe, stem)(*args) == pkg.CSINN_TRUE, stem
        last = self.layers[-1][1]
        fe.csinn_set_output(0, t[last], sess)
        assert fe.csinn_session_setup(sess) == pkg.CSINN_TRUE
        self._keep, self._sess, self._out_shape, self._in_q = keep, sess, tuple(shape[last]), self.q_in
        return sess

    run = tail.MiniNet.run
    close = tail.MiniNet.close


def check(gpu, monkeypatch, make, folded, pairs, pools):
    """the device-resident session plans what is expected and computes what the host-staged session and the oracle do"""
    fe, hip, opt = gpu
    net = make()
    sess = net.build(fe, pkg.API_MI355X)
    assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
    counts = (opt.shl_mi355x_session_folded_activations(sess), opt.shl_mi355x_session_fused_pairs(sess),
              opt.shl_mi355x_session_fused_pools(sess))
    print("folded, pairs, pools =", counts)
    assert counts == (folded, pairs, pools)
    monkeypatch.setenv("SHL_MI355X_HOST_SESSION", "1")
    host = make()
    host_sess = host.build(fe, pkg.API_MI355X)
    monkeypatch.delenv("SHL_MI355X_HOST_SESSION")
    assert opt.shl_mi355x_session_is_device_resident(host_sess) == 0
    assert opt.shl_mi355x_session_folded_activations(host_sess) == 0
    outs = []
    for k in (0, 1, 0):  # the graph replay reads fresh data
        x = net.input(k)
        got, staged, want = net.run(fe, x), host.run(fe, x), net.oracle(x)
        assert got.shape == want.shape
        n, worst = cases.mismatch_report(got, staged)
        assert n == 0, "input %d: device-resident vs host-staged: %d mismatches (max |d| %d)" % (k, n, worst)
        n, worst = cases.mismatch_report(got, want)
        assert n == 0, "input %d: device-resident vs the oracle chain: %d mismatches (max |d| %d)" % (k, n, worst)
        outs.append(want)
    assert not np.array_equal(outs[0], outs[1]), "the two inputs must tell runs apart"
    host.close(fe)
    net.close(fe)


def pair_with_both_halves_folded():
    """pw 32 -> 64 @16x16 -> relu -> dw 3x3 stride 2 -> relu -> pw 64 -> 32 -> relu: the pair is test_fusion.py's first,
    which qualifies on its own; every relu a layer of its own with its convolution's output record"""
    pw, dw = make_pwdw(0, **dict(PWDW_PAIRS[0], relu=(0, 0)))
    pw2 = follow(cases.make_case(790, n=1, h=dw["ho"], w=dw["wo"], c=dw["co"], co=32, k=(1, 1), pad=(0, 0, 0, 0)), dw)
    layers = [("conv", "pw", ["data"], pw), ("relu", "pw_relu", ["pw"], rec(pw)),
              ("conv", "dw", ["pw_relu"], dw), ("relu", "dw_relu", ["dw"], rec(dw)),
              ("conv", "pw2", ["dw_relu"], pw2), ("relu", "pw2_relu", ["pw2"], rec(pw2))]
    return Graph(pw["in_shape"], (float(pw["in_scale"]), int(pw["in_zp"])), layers, seed=4100)


def two_consumers():
    """conv1x1 16 -> 16 @8x8 -> relu, then add(conv_out, relu_out): the convolution's output has two consumers, so the relu
    (which carries the convolution's record and would fold) stays a layer of its own"""
    conv = cases.make_case(791, n=1, h=8, w=8, c=16, co=16, k=(1, 1), pad=(0, 0, 0, 0))
    layers = [("conv", "conv", ["data"], conv), ("relu", "relu", ["conv"], rec(conv)),
              ("add", "sum", ["conv", "relu"], (float(np.float32(2.0 * conv["out_scale"])), -30))]
    return Graph(conv["in_shape"], (float(conv["in_scale"]), int(conv["in_zp"])), layers, seed=4200)


def fold_in_front_of_conv_pool():
    """pw -> relu -> global_avgpool2d -> softmax at the smallest batch-1 shape among test_tail.py's conv + pool cases"""
    kw = min((c for c in CONV_POOL if c["n"] == 1), key=lambda c: c["hw"] * c["hw"] * c["c"] * c["co"])
    assert (kw["hw"], kw["c"], kw["co"]) == (8, 256, 64)
    conv = cases.make_case(792, n=1, h=kw["hw"], w=kw["hw"], c=kw["c"], co=kw["co"], k=(1, 1), pad=(0, 0, 0, 0))
    layers = [("conv", "pw", ["data"], conv), ("relu", "pw_relu", ["pw"], rec(conv)),
              ("pool", "gap", ["pw_relu"], (float(np.float32(conv["out_scale"] / 4)), -20)),
              ("softmax", "prob", ["gap"], (1.0 / 256, -128))]
    return Graph(conv["in_shape"], (float(conv["in_scale"]), int(conv["in_zp"])), layers, seed=4300)


@pytest.mark.gpu
def test_a_pair_whose_halves_both_carry_a_folded_activation(gpu, monkeypatch):
    """six layers, two launches: [pw + relu + dw + relu] and [pw + relu].  The merge has a folded activation on both
    sides of it, and the layer behind the pair is found behind the second fold."""
    check(gpu, monkeypatch, pair_with_both_halves_folded, folded=3, pairs=1, pools=0)


@pytest.mark.gpu
def test_a_second_consumer_blocks_the_fold_and_every_merge(gpu, monkeypatch):
    """three layers, three launches: nothing folds, nothing pairs, and add reads both tensors"""
    check(gpu, monkeypatch, two_consumers, folded=0, pairs=0, pools=0)


@pytest.mark.gpu
def test_a_fold_in_front_of_convolution_plus_pool(gpu, monkeypatch):
    """four layers, two launches: [pw + relu + global_avgpool2d] and softmax.  The pool reads the ACTIVATION's output
    record, and the layer behind the merge is the softmax, not the pool a second time."""
    check(gpu, monkeypatch, fold_in_front_of_conv_pool, folded=1, pairs=0, pools=1)

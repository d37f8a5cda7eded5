"""Cases of an int8 table activation folded into the convolution's launch -- conv2d [+ folded relu / relu6] -> sigmoid |
hard_sigmoid | silu | leaky_relu, or the gate of a swish / hard-swish, sigmoid | hard_sigmoid -> mul(x, gate)
(shl_mi355x_conv_lut_forward) -- with the oracle chain, the two ways to run them on the device, the gate tables' golden
cases and two small networks for the session tests.

  gate_cases()      every (activation, record triple, operand order) whose 256 products the genuine library gave
                    (tests/golden/act_fuse_cases.npz, written by tests/golden/make_act_fuse_golden.py)
  all_cases()       (shape, table) pairs.  Shapes are residual_cases.py's strata, the smallest at which each store path of the
                    two carrying kernel families can go wrong; tables are TABLES below
  child_cases()     256 x 128, 256 x 256 and the flavours without producer waves: `python act_fuse_cases.py` runs them under the
                    caller's environment (the switches are read once per process)
  yolo_stack(), hswish_block() and the nets that must NOT fuse
"""
import ctypes as C
import os
import sys

import numpy as np

import cases
import eltwise_cases as ec
import residual_cases as rc
from cases import pkg
from pool_cases import _q
from residual_nets import SkipNet

POISON, GUARD = rc.POISON, rc.GUARD
EVERY = np.arange(-128, 128, dtype=np.int16).astype(np.int8)  # byte q at index q + 128
SLOPE = 0.1

# ------------------------------------------------------------------------------------------ the gate tables
GATE_KINDS = ("sigmoid", "hard_sigmoid")
# (x: the convolution's output, gate: the activation's output, out: the mul's output)
GATE_TRIPLES = {
    "pow2": (_q(2.0 ** -4, -5), _q(2.0 ** -8, -128), _q(2.0 ** -4, -5)),
    "conv": (_q(0.0473, -9), _q(0.00392157, -128), _q(0.0311, 3)),       # converter scales
    "zps": (_q(0.0391, -128), _q(0.0079, 0), _q(0.0207, 127)),            # zero points at both ends and in the middle: x >= 0 under
                                                                          # an output zero point of 127 saturates every product
    "zps_neg": (_q(0.0391, 127), _q(0.0079, 0), _q(0.0011, 127)),         # ... x <= 0 under it spreads them
}


def gate_cases():
    return [dict(name="gate_%s_%s_%s" % (kind, key, "x_first" if x_first else "gate_first"), kind=kind, q=GATE_TRIPLES[key], x_first=x_first)
            for kind in GATE_KINDS for key in GATE_TRIPLES for x_first in (1, 0)]


def gate_layers(case, x=EVERY):
    """the two layers of a gate as eltwise_cases describes single-op problems: (activation case, a function giving the mul case
    from the activation's output)"""
    qx, qg, qo = case["q"]
    act = dict(name=case["name"] + "_act", op=case["kind"], dtype="int8", x=np.ascontiguousarray(x), in_q=qx, out_q=qg, n=0.0, layout="NHWC")

    def mul_of(gate):
        # eltwise_run gives `y` as the FIRST input under small_first: the gate first
        return dict(name=case["name"] + "_mul", op="mul", dtype="int8", x=np.ascontiguousarray(x), y=np.ascontiguousarray(gate),
                    in_q=qx, in1_q=qg, out_q=qo, layout="N", small_first=not case["x_first"], b_const=False)
    return act, mul_of


def gate_numpy(case, x=EVERY):
    """the numpy restatement of the reference for the two layers"""
    act, mul_of = gate_layers(case, x)
    return ec.eltwise_numpy(mul_of(ec.eltwise_numpy(act)))


def gate_through(fe, api, case):
    """the two layers in layer mode through a front-end (the genuine library: api = pkg.API_REF)"""
    act, mul_of = gate_layers(case)
    return ec.eltwise_run(fe, api, mul_of(ec.eltwise_run(fe, api, act)))


def golden():
    blob = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "act_fuse_cases.npz"))
    return {k: blob[k] for k in blob.files}


def gate_table(opt, case):
    """shl_mi355x_gate_mul_table_i8's 256 bytes, indexed by (uint8_t)q"""
    (sx, zx), (sg, zg), (so, zo) = case["q"]
    tab = np.zeros(256, np.uint8)
    opt.shl_mi355x_gate_mul_table_i8(ec.KIND[case["kind"]], sx, zx, sg, zg, case["x_first"], so, zo, tab.ctypes.data_as(C.POINTER(C.c_uint8)))
    return tab


def by_q(table):
    """a table indexed by (uint8_t)q as int8 results in the order of EVERY (q = -128 .. 127)"""
    return table[EVERY.view(np.uint8)].view(np.int8)


# ------------------------------------------------------------------------------------------ convolution + table
# name -> (kind, output record or None, extra).  The table's input record is the convolution's output record
TABLES = {
    "sigmoid": ("sigmoid", _q(0.00392157, -128), {}),
    "hard_sigmoid": ("hard_sigmoid", _q(0.0041, -120), {}),
    "silu": ("silu", _q(0.0219, 4), {}),
    "leaky_relu": ("leaky_relu", _q(0.0311, -20), {}),
    "silu_zp_min": ("silu", _q(0.0173, -128), {}),
    "leaky_zp_max": ("leaky_relu", _q(0.0257, 127), {}),
    "identity": ("identity", None, {}),
    "permutation": ("permutation", None, {}),
    "gate": ("gate", None, dict(kind="hard_sigmoid", gate_q=_q(0.00392157, -128), out_q=_q(0.0311, 3), x_first=0)),
}
PW = rc.PW
SHAPES = {
    # ---- wave
    "wave_1x1_m33_co36": ("wave", dict(PW, h=3, w=11, c=16, co=36), 1),
    "wave_1x1_m33_co30_elements": ("wave", dict(PW, h=3, w=11, c=16, co=30, exact=False), 2),
    "wave_1x1_c256_splitk_relu6": ("wave", dict(PW, h=8, w=8, c=256, co=32, act=2), 3),  # the convolution folds its own relu6
    "wave_3x3_5x7": ("wave", dict(h=5, w=7, c=16, co=32, exact=False), 4),
    "wave_3x3_s2_9x9": ("wave", dict(h=9, w=9, c=16, co=32, stride=(2, 2)), 5),
    # ---- tile
    "tile_m129_co144_staged": ("tile", dict(PW, h=3, w=43, c=64, co=144, exact=False), 8),
    "tile_m129_co130_elements": ("tile", dict(PW, h=3, w=43, c=16, co=130), 9),
    "tile_m257_co64_256x64_relu6": ("tile", dict(PW, h=1, w=257, c=64, co=64, act=2), 10),
}
_CONVS = {}


def conv_of(shape):
    """the shape's convolution problem, made once"""
    if shape not in _CONVS:
        form, kw, seed = (SHAPES.get(shape) or CHILD_SHAPES[shape])
        _CONVS[shape] = cases.make_case(9300 + seed, **kw)
    return _CONVS[shape]


def _case(shape, table):
    return dict(name=shape + "-" + table, shape=shape, form=(SHAPES.get(shape) or CHILD_SHAPES[shape])[0], table=table)


def all_cases():
    out = []
    # every table on one shape of each family (the dword stores of the wave kernel, the staged stores of the tile kernel) ...
    for shape in ("wave_1x1_m33_co36", "tile_m129_co144_staged"):
        out += [_case(shape, t) for t in TABLES]
    # ... and on every other store path the table that tells every byte and every byte lane apart, and one activation
    others = [s for s in SHAPES if s not in ("wave_1x1_m33_co36", "tile_m129_co144_staged")]
    acts = ("silu", "leaky_relu", "sigmoid", "hard_sigmoid", "gate", "silu_zp_min")
    for i, shape in enumerate(others):
        out += [_case(shape, "permutation"), _case(shape, acts[i % len(acts)])]
    return out


# the large tile flavours need uniform-tap addressing (C % 64 == 0); one ragged tile in each direction
CHILD_SHAPES = {
    "tile_m257_co144_c64": ("tile", dict(PW, h=1, w=257, c=64, co=144, exact=False), 20),
    "tile_m257_co272_c64": ("tile", dict(PW, h=1, w=257, c=64, co=272), 21),
    "tile_3x3_m260_co130_c64": ("tile", dict(h=10, w=26, c=64, co=130), 22),
}
CHILD_ENVS = rc.CHILD_ENVS


def child_cases():
    return [_case("tile_m257_co144_c64", "permutation"), _case("tile_m257_co272_c64", "silu"), _case("tile_3x3_m260_co130_c64", "permutation"),
            _case("tile_3x3_m260_co130_c64", "gate")]


def conv_q(c):
    return _q(float(np.float32(c["out_scale"])), c["out_zp"])


def oracle_table(case):
    """the case's table from the numpy restatement of the reference, as int8 results in the order of EVERY"""
    kind, out_q, extra = TABLES[case["table"]]
    in_q = conv_q(conv_of(case["shape"]))
    if kind == "identity":
        return EVERY.copy()
    if kind == "permutation":
        return np.random.default_rng(77).permutation(256).astype(np.uint8).view(np.int8)
    if kind == "gate":
        return gate_numpy(dict(name="g", kind=extra["kind"], q=(in_q, extra["gate_q"], extra["out_q"]), x_first=extra["x_first"]))
    return ec.eltwise_numpy(dict(op=kind, dtype="int8", x=EVERY, in_q=in_q, out_q=out_q, n=float(np.float32(SLOPE))))


def device_table(opt, case):
    """the 256 bytes handed to the device, indexed by (uint8_t)q: the backend's own builders for the layers' tables"""
    kind, out_q, extra = TABLES[case["table"]]
    (si, zi) = conv_q(conv_of(case["shape"]))
    tab = np.zeros(256, np.uint8)
    ptr = tab.ctypes.data_as(C.POINTER(C.c_uint8))
    if kind in ("identity", "permutation"):
        tab[EVERY.view(np.uint8)] = oracle_table(case).view(np.uint8)
    elif kind == "gate":
        tab = gate_table(opt, dict(kind=extra["kind"], q=((si, zi), extra["gate_q"], extra["out_q"]), x_first=extra["x_first"]))
    elif kind == "leaky_relu":
        opt.shl_mi355x_leaky_relu_table_i8(si, zi, out_q[0], out_q[1], SLOPE, ptr)
    else:
        getattr(opt, "shl_mi355x_%s_table_i8" % kind)(si, zi, out_q[0], out_q[1], ptr)
    return tab


_ORACLE_CONV = {}


def oracle_chain(case):
    """conv (oracle formulation X: what the device computes bit for bit in both scale regimes, computed once per shape), then
    the reference's layers on the stored bytes"""
    if case["shape"] not in _ORACLE_CONV:
        _ORACLE_CONV[case["shape"]] = cases.oracle_run(conv_of(case["shape"]), "exact")
    conv = _ORACLE_CONV[case["shape"]]
    return dict(conv=conv, out=oracle_table(case)[conv.astype(np.int16) + 128])


def run_both(hip, opt, dev, case):
    """(fused output, unfused output, the guard bytes around the fused output, the fused launch's kernel name), on one set of
    buffers"""
    c = conv_of(case["shape"])
    n = int(np.prod(c["out_shape"]))
    plan = rc.make_plan(hip, c)
    table = device_table(opt, case)
    d_in, d_conv, d_un, d_guarded = dev.alloc(c["input"].nbytes), dev.alloc(n), dev.alloc(n), dev.alloc(n + 2 * GUARD)
    try:
        dev.upload(d_in, c["input"])
        dev.upload(d_guarded, np.full(n + 2 * GUARD, POISON, np.uint8))
        name = hip.shl_mi355x_conv_lut_kernel_name(plan, 0).decode()
        pkg.check(hip.shl_mi355x_conv_lut_forward(plan, d_in, d_guarded + GUARD, 0, table.ctypes.data, None), hip, "conv_lut_forward")
        pkg.check(hip.shl_mi355x_conv_forward(plan, d_in, d_conv, 0, None), hip, "conv_forward")
        pkg.check(hip.shl_mi355x_unary_lut_i8(d_conv, d_un, n, table.ctypes.data, None), hip, "unary_lut_i8")
        unfused = dev.download(d_un, c["out_shape"], np.int8)
        whole = dev.download(d_guarded, (n + 2 * GUARD,), np.uint8)
        fused = whole[GUARD:GUARD + n].view(np.int8).reshape(c["out_shape"])
        return fused, unfused, np.concatenate([whole[:GUARD], whole[GUARD + n:]]), name
    finally:
        for p in (d_in, d_conv, d_un, d_guarded):
            dev.free(p)
        hip.shl_mi355x_conv_plan_destroy(plan)


def check_case(hip, opt, dev, case, expect_family):
    want = oracle_chain(case)["out"]
    fused, unfused, guards, name = run_both(hip, opt, dev, case)
    assert name == expect_family + "+lut", (case["name"], name)
    assert (guards == POISON).all(), case["name"] + ": the fused launch wrote outside its output"
    for what, got in (("unfused", unfused), ("fused", fused)):
        bad, worst = cases.mismatch_report(got, want)
        assert bad == 0, "%s: %s differs from the oracle chain on %d of %d outputs (max %d)" % (case["name"], what, bad, got.size, worst)
    assert np.array_equal(fused, unfused)


# ------------------------------------------------------------------------------------------ networks
class ActNet(SkipNet):
    """SkipNet with the table activations, a mul of two activations (the second one may be [1, 1, 1, C]) and a global average
    pool; the oracle chain runs them through eltwise_cases.eltwise_numpy"""

    def oracle(self, x, extra=None):
        import tail
        env = {self.in_name: x}
        for kind, name, ins, outs, info in self.layers:
            a = env[ins[0]]
            if kind == "conv":
                case = dict(self.cv[name])
                case["input"] = np.ascontiguousarray(a)
                env[outs[0]] = cases.oracle_run(case, "ref")
            elif kind in ec.UNARY:
                env[outs[0]] = ec.eltwise_numpy(dict(op=kind, dtype="int8", x=a, in_q=self.rec(ins[0]), out_q=self.rec(outs[0]),
                                                     n=float(np.float32(SLOPE))))
            elif kind == "mul":
                first, second = env[ins[0]], env[ins[1]]
                small_first = first.size < second.size
                full, small = (second, first) if small_first else (first, second)
                qf, qs = (self.rec(ins[1]), self.rec(ins[0])) if small_first else (self.rec(ins[0]), self.rec(ins[1]))
                env[outs[0]] = ec.eltwise_numpy(dict(op="mul", dtype="int8", x=full, y=small, in_q=qf, in1_q=qs, out_q=self.rec(outs[0]),
                                                     small_first=small_first))
            elif kind == "add":
                env[outs[0]] = tail.siso_oracle(dict(kind="add", x=a, y=env[ins[1]], dtype="int8", layout="NHWC", axis=1,
                                                     in_q=self.rec(ins[0]), in1_q=self.rec(ins[1]), out_q=self.rec(outs[0])))
            else:
                what = {"relu": "relu", "gap": "pool"}[kind]
                env[outs[0]] = tail.siso_oracle(dict(kind=what, x=a, dtype="int8", layout="NHWC", axis=1, in_q=self.rec(ins[0]),
                                                     out_q=self.rec(outs[0])))
        return env

    def build(self, fe, api):
        keep = pkg.Keep()
        sess = fe.csinn_alloc_session()
        sc = sess.contents
        sc.base_api, sc.base_run_mode, sc.base_dtype = api, pkg.RM_CPU_GRAPH, pkg.DTYPE_INT8
        sc.base_quant_type = pkg.QUANT_INT8_ASYM_W_SYM
        sc.debug_level = 0
        fe.csinn_session_init(sess)
        act_l = pkg.LAYOUT_NHWC

        def T(dims, rec, name, data=None, const=0, layout=act_l, dtype=pkg.DTYPE_INT8, scales=None):
            return pkg.make_tensor(fe, keep, dims, dtype, layout, data=data, is_const=const, name=name, sess=sess,
                                   scales=scales if scales is not None else (rec[0],), zps=(rec[1] if rec else 0,))
        env = {self.in_name: T(self.shape(self.in_name), self.rec(self.in_name), self.in_name.encode())}
        ops = []
        for kind, name, ins, outs, info in self.layers:
            env[outs[0]] = T(self.shape(outs[0]), self.rec(outs[0]), outs[0].encode())
            nm = name.encode()
            if kind == "conv":
                case = self.cv[name]
                w_l = pkg.LAYOUT_1HWO if case["depthwise"] else pkg.LAYOUT_OHWI
                t_w = T(case["w_shape"], None, nm + b"_w", case["kernel"], 1, w_l, scales=tuple(case["k_scale"]))
                t_b = T((case["co"],), None, nm + b"_b", case["bias"], 1, pkg.LAYOUT_O, pkg.DTYPE_INT32, scales=tuple(case["b_scale"]))
                p = pkg.conv_params(fe, keep, api, act_l, case["stride"], case["pad"], case["dilation"], case["group"], 0, sess, nm)
                stem = {0: "csinn_conv2d", 1: "csinn_conv2d_relu", 2: "csinn_conv2d_relu6"}[case["act"]]
                if case["depthwise"]:
                    stem = stem.replace("csinn_conv2d", "csinn_depthwise_conv2d")
                ops.append((stem, (env[ins[0]], env[outs[0]], t_w, t_b, p)))
            elif kind in ("add", "mul"):
                ops.append(("csinn_" + kind, (env[ins[0]], env[ins[1]], env[outs[0]], pkg.siso_params(fe, keep, api, kind, act_l, 1, sess, nm))))
            elif kind == "gap":
                ops.append(("csinn_global_avgpool2d", (env[ins[0]], env[outs[0]], pkg.siso_params(fe, keep, api, "pool", act_l, 1, sess, nm))))
            else:
                ops.append(("csinn_" + kind, (env[ins[0]], env[outs[0]], pkg.siso_params(fe, keep, api, kind, act_l, 1, sess, nm, n=SLOPE))))
        fe.csinn_set_input_number(1, sess)
        fe.csinn_set_output_number(len(self.outputs), sess)
        for stem, args in ops:
            assert getattr(fe, stem + "_init")(*args) == pkg.CSINN_TRUE, stem
        fe.csinn_set_tensor_entry(env[self.in_name], sess)
        fe.csinn_set_input(0, env[self.in_name], sess)
        for stem, args in ops:
            assert getattr(fe, stem)(*args) == pkg.CSINN_TRUE, stem
        for i, o in enumerate(self.outputs):
            fe.csinn_set_output(i, env[o], sess)
        rc_ = fe.csinn_session_setup(sess)
        assert rc_ == pkg.CSINN_TRUE or getattr(fe, "kind", "") == "reference"
        self._keep, self._sess, self.layer_count = keep, sess, len(ops)
        return sess


q = lambda s, z: _q(2.0 ** s, z)


def yolo_stack():
    """3x3 s2 conv -> silu -> 1x1 conv -> leaky_relu -> 3x3 conv -> silu -> add(skip): three table activations"""
    t = {"x": (16, 12, q(-4, -5)), "c1": (32, 6, q(-3, 3)), "a1": (32, 6, q(-4, -90)), "c2": (32, 6, q(-3, -9)), "a2": (32, 6, q(-4, -60)),
         "c3": (32, 6, q(-3, 11)), "a3": (32, 6, q(-4, -100)), "out": (32, 6, q(-3, -110))}
    L = [("conv", "down", ["x"], ["c1"], dict(k=3, stride=2)), ("silu", "silu1", ["c1"], ["a1"], {}),
         ("conv", "pw", ["a1"], ["c2"], {}), ("leaky_relu", "leaky", ["c2"], ["a2"], {}),
         ("conv", "body", ["a2"], ["c3"], dict(k=3)), ("silu", "silu2", ["c3"], ["a3"], {}), ("add", "add", ["a3", "a1"], ["out"], {})]
    return ActNet("int8", "NHWC", 71, "x", t, L, ["out"])


def hswish_block():
    """1x1 expand -> hard_sigmoid -> mul(conv, gate) -> depthwise 3x3 -> 1x1 project -> sigmoid -> mul(gate, conv): two gates,
    the convolution's output on either side of the mul"""
    t = {"x": (16, 8, q(-4, -5)), "e": (48, 8, q(-4, 7)), "g1": (48, 8, q(-8, -128)), "h1": (48, 8, q(-4, -100)), "d": (48, 8, q(-3, -20)),
         "p": (16, 8, q(-4, 9)), "g2": (16, 8, q(-8, -128)), "out": (16, 8, q(-4, -30))}
    L = [("conv", "expand", ["x"], ["e"], {}), ("hard_sigmoid", "hsig", ["e"], ["g1"], {}), ("mul", "hswish", ["e", "g1"], ["h1"], {}),
         ("conv", "dw", ["h1"], ["d"], dict(k=3, depthwise=True, k_log2=-5)), ("conv", "project", ["d"], ["p"], {}),
         ("sigmoid", "sig", ["p"], ["g2"], {}), ("mul", "swish", ["g2", "p"], ["out"], {})]
    return ActNet("int8", "NHWC", 72, "x", t, L, ["out"])


def exported_intermediate():
    """conv -> silu, the convolution's output a graph output too"""
    t = {"x": (16, 8, q(-4, -5)), "c": (32, 8, q(-3, 3)), "out": (32, 8, q(-4, -90))}
    L = [("conv", "conv", ["x"], ["c"], dict(k=3)), ("silu", "silu", ["c"], ["out"], {})]
    return ActNet("int8", "NHWC", 73, "x", t, L, ["out", "c"])


def exported_gate():
    """conv -> hard_sigmoid -> mul(conv, gate), the gate a graph output too"""
    t = {"x": (16, 8, q(-4, -5)), "c": (32, 8, q(-4, 7)), "g": (32, 8, q(-8, -128)), "out": (32, 8, q(-4, -100))}
    L = [("conv", "conv", ["x"], ["c"], {}), ("hard_sigmoid", "hsig", ["c"], ["g"], {}), ("mul", "hswish", ["c", "g"], ["out"], {})]
    return ActNet("int8", "NHWC", 74, "x", t, L, ["out", "g"])


def third_reader():
    """conv -> hard_sigmoid -> mul(conv, gate), and a relu that reads the convolution's output as well"""
    t = {"x": (16, 8, q(-4, -5)), "c": (32, 8, q(-4, 7)), "g": (32, 8, q(-8, -128)), "out": (32, 8, q(-4, -100)), "r": (32, 8, q(-4, -128))}
    L = [("conv", "conv", ["x"], ["c"], {}), ("hard_sigmoid", "hsig", ["c"], ["g"], {}), ("mul", "hswish", ["c", "g"], ["out"], {}),
         ("relu", "relu", ["c"], ["r"], {})]
    return ActNet("int8", "NHWC", 75, "x", t, L, ["out", "r"])


def broadcast_gate():
    """a squeeze-and-excite gate: conv -> global_avgpool -> hard_sigmoid -> mul(conv, gate [1, 1, 1, C]): the mul broadcasts"""
    t = {"x": (16, 8, q(-4, -5)), "c": (32, 8, q(-4, 7)), "s": (32, 1, q(-5, 0)), "g": (32, 1, q(-8, -128)), "out": (32, 8, q(-4, -100))}
    L = [("conv", "conv", ["x"], ["c"], dict(k=3)), ("gap", "squeeze", ["c"], ["s"], {}), ("hard_sigmoid", "hsig", ["s"], ["g"], {}),
         ("mul", "excite", ["c", "g"], ["out"], {})]
    return ActNet("int8", "NHWC", 76, "x", t, L, ["out"])


FUSING = {"yolo_stack": (yolo_stack, 3), "hswish_block": (hswish_block, 2)}
APART = {"exported_intermediate": exported_intermediate, "exported_gate": exported_gate, "third_reader": third_reader,
         "broadcast_gate": broadcast_gate}


if __name__ == "__main__":  # the child of tests/test_act_fuse.py: the tile flavours chosen through the environment
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    device = cases.HipDevice(hip)
    os.environ["SHL_MI355X_ACT_FORM"] = "tile"
    for cs in child_cases():
        check_case(hip, opt, device, cs, "tile")
        print("ok", cs["name"])
    print("child ok", len(child_cases()))
    sys.exit(0)

"""Small networks with a skip connection, given as split_shuffle_cases.GraphNet gives them -- a list of layers over named
tensors, run through the csinn session API in graph mode and as an oracle chain -- with the two layer kinds the residual tail
needs on top: add (two activations; same shape, or the second one [1, 1, 1, C] for a broadcast) and relu6.

  basic_block       conv3x3 -> add(conv, x) -> relu                                   (tests/tail.py:ResidualNet's structure)
  inverted_block    pw expand + relu6 -> dw3x3 + relu6 -> pw project -> add(x, proj)  (MobileNetV2; no activation behind the sum)
  projection_block  main: conv1x1 + relu -> conv3x3; shortcut conv1x1 on x; add(main, shortcut) -> relu: the add directly
                    follows the SHORTCUT convolution, which is the one that fuses
  two_consumers     basic_block whose convolution output is a graph output too
  broadcast_block   conv3x3 -> add(conv, per-channel tensor [1, 1, 1, C]) -> relu
"""
import numpy as np

import cases
import tail
from cases import pkg
from pool_cases import _q
from split_shuffle_cases import GraphNet


class SkipNet(GraphNet):
    """tensors: name -> (channels, height, record); a height of 0 marks a per-channel tensor [1, 1, 1, C]"""

    def shape(self, name):
        c, h, _ = self.tensors[name]
        if h == 0:
            return (1, 1, 1, c) if self.layout == "NHWC" else (1, c, 1, 1)
        return GraphNet.shape(self, name)

    def oracle(self, x, extra=None):
        env = {self.in_name: x}
        env.update(extra or {})
        form = "ref" if self.dtype == "int8" else "f16"
        for kind, name, ins, outs, info in self.layers:
            a = env[ins[0]]
            if kind == "conv":
                case = dict(self.cv[name])
                case["input"] = np.ascontiguousarray(a)
                env[outs[0]] = cases.oracle_run(case, form)
            elif kind == "add":
                b = np.ascontiguousarray(np.broadcast_to(env[ins[1]], a.shape))
                env[outs[0]] = tail.siso_oracle(dict(kind="add", x=a, y=b, dtype=self.dtype, layout=self.layout, axis=1,
                                                     in_q=self.rec(ins[0]), in1_q=self.rec(ins[1]), out_q=self.rec(outs[0])))
            else:
                env[outs[0]] = tail.siso_oracle(dict(kind=kind, x=a, dtype=self.dtype, layout=self.layout, axis=1,
                                                     in_q=self.rec(ins[0]), out_q=self.rec(outs[0])))
        return env

    def build(self, fe, api):
        keep = pkg.Keep()
        sess = fe.csinn_alloc_session()
        sc = sess.contents
        int8 = self.dtype == "int8"
        dt = pkg.DTYPE_INT8 if int8 else pkg.DTYPE_FLOAT16
        sc.base_api, sc.base_run_mode, sc.base_dtype = api, pkg.RM_CPU_GRAPH, dt
        sc.base_quant_type = pkg.QUANT_INT8_ASYM_W_SYM if int8 else pkg.QUANT_FLOAT16
        sc.debug_level = 0
        fe.csinn_session_init(sess)
        nhwc = self.layout == "NHWC"
        act_l = pkg.LAYOUT_NHWC if nhwc else pkg.LAYOUT_NCHW

        def T(dims, rec, name, data=None, const=0, layout=act_l, dtype=dt, scales=None):
            return pkg.make_tensor(fe, keep, dims, dtype, layout, data=data, is_const=const, name=name, sess=sess,
                                   scales=scales if scales is not None else (rec[0],), zps=(rec[1] if rec else 0,))
        env = {self.in_name: T(self.shape(self.in_name), self.rec(self.in_name), self.in_name.encode())}
        for cname, data in getattr(self, "consts", {}).items():
            env[cname] = T(self.shape(cname), self.rec(cname), cname.encode(), data, 1)
        ops = []
        for kind, name, ins, outs, info in self.layers:
            env[outs[0]] = T(self.shape(outs[0]), self.rec(outs[0]), outs[0].encode())
            nm = name.encode()
            if kind == "conv":
                case = self.cv[name]
                if case["depthwise"]:
                    w_l = pkg.LAYOUT_1HWO if nhwc else pkg.LAYOUT_O1HW
                else:
                    w_l = pkg.LAYOUT_OHWI if nhwc else pkg.LAYOUT_OIHW
                t_w = T(case["w_shape"], None, nm + b"_w", case["kernel"], 1, w_l, scales=tuple(case["k_scale"]))
                t_b = T((case["co"],), None, nm + b"_b", case["bias"], 1, pkg.LAYOUT_O, pkg.DTYPE_INT32 if int8 else dt,
                        scales=tuple(case["b_scale"]))
                p = pkg.conv_params(fe, keep, api, act_l, case["stride"], case["pad"], case["dilation"], case["group"], 0, sess, nm)
                stem = {0: "csinn_conv2d", 1: "csinn_conv2d_relu", 2: "csinn_conv2d_relu6"}[case["act"]]
                if case["depthwise"]:
                    stem = stem.replace("csinn_conv2d", "csinn_depthwise_conv2d")
                ops.append((stem, (env[ins[0]], env[outs[0]], t_w, t_b, p)))
            elif kind == "add":
                ops.append(("csinn_add", (env[ins[0]], env[ins[1]], env[outs[0]], pkg.siso_params(fe, keep, api, "add", act_l, 1, sess, nm))))
            else:
                ops.append(("csinn_" + kind, (env[ins[0]], env[outs[0]], pkg.siso_params(fe, keep, api, kind, act_l, 1, sess, nm))))
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
        rc = fe.csinn_session_setup(sess)
        assert rc == pkg.CSINN_TRUE or getattr(fe, "kind", "") == "reference"
        self._keep, self._sess, self.layer_count = keep, sess, len(ops)
        return sess


q = lambda s, z: _q(2.0 ** s, z)


def basic_block(dtype="int8", layout="NHWC", export_conv=False):
    t = {"x": (32, 12, q(-4, -5)), "conv": (32, 12, q(-3, 3)), "sum": (32, 12, q(-2, -30)), "out": (32, 12, q(-3, -128))}
    L = [("conv", "conv", ["x"], ["conv"], dict(k=3)), ("add", "add", ["conv", "x"], ["sum"], {}), ("relu", "relu", ["sum"], ["out"], {})]
    return SkipNet(dtype, layout, 61, "x", t, L, ["out"] + (["conv"] if export_conv else []))


def inverted_block(dtype="int8", layout="NHWC"):
    """the relu6 layers are layers of their own (same record as the convolution in front: a session folds them)"""
    t = {"x": (16, 14, q(-4, -5)), "ec": (96, 14, q(-5, -128)), "e": (96, 14, q(-5, -128)), "dc": (96, 14, q(-5, -128)),
         "d": (96, 14, q(-5, -128)), "proj": (16, 14, q(-3, 9)), "out": (16, 14, q(-2, -7))}
    L = [("conv", "expand", ["x"], ["ec"], {}), ("relu6", "expand_relu6", ["ec"], ["e"], {}),
         ("conv", "dw", ["e"], ["dc"], dict(k=3, depthwise=True, k_log2=-5)), ("relu6", "dw_relu6", ["dc"], ["d"], {}),
         ("conv", "project", ["d"], ["proj"], {}), ("add", "add", ["x", "proj"], ["out"], {})]
    return SkipNet(dtype, layout, 62, "x", t, L, ["out"])


def projection_block(dtype="int8", layout="NHWC"):
    t = {"x": (32, 8, q(-4, -5)), "m1": (16, 8, q(-3, -100)), "m2": (64, 8, q(-2, 11)), "short": (64, 8, q(-3, -9)),
         "sum": (64, 8, q(-1, -20)), "out": (64, 8, q(-2, -128))}
    L = [("conv", "reduce", ["x"], ["m1"], dict(act=1)), ("conv", "body", ["m1"], ["m2"], dict(k=3)),
         ("conv", "shortcut", ["x"], ["short"], {}), ("add", "add", ["m2", "short"], ["sum"], {}), ("relu", "relu", ["sum"], ["out"], {})]
    return SkipNet(dtype, layout, 63, "x", t, L, ["out"])


def broadcast_block(dtype="int8", layout="NHWC"):
    t = {"x": (32, 12, q(-4, -5)), "conv": (32, 12, q(-3, 3)), "pc": (32, 0, q(-4, 7)), "sum": (32, 12, q(-2, -30)), "out": (32, 12, q(-3, -128))}
    L = [("conv", "conv", ["x"], ["conv"], dict(k=3)), ("add", "add", ["conv", "pc"], ["sum"], {}), ("relu", "relu", ["sum"], ["out"], {})]
    net = SkipNet(dtype, layout, 64, "x", t, L, ["out"])
    net.consts = {"pc": np.random.default_rng(65).integers(-100, 100, net.shape("pc"), dtype=np.int8)}
    return net


FUSING = {"basic_block": basic_block, "inverted_block": inverted_block, "projection_block": projection_block}

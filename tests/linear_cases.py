"""Networks with linear layers as converters export them -- MatMul(x, W_const) followed by Add(., bias_const[N]) -- for the
session tests of the broadcasting add and of the matmul + bias fusion.

  LinearNet            matmul_cases.MatmulNet plus the layer kinds these networks need: addc (add of a constant, given second or
                       first: a bias, an attention bias), mul (two activations), hard_sigmoid; run through the csinn session API
                       in graph mode and as an oracle chain (matmul through matmul_cases.chain_ref, addc through
                       add_bcast_cases.add_numpy, mul / mulc / hard_sigmoid through eltwise_cases.eltwise_numpy, the rest
                       through the C oracle's restatements)
  mlp()                [2,17,64] -> matmul W1[64,128] + b1[128] -> relu -> matmul W2[128,64] + b2[64] (the bias given FIRST) ->
                       add the residual
  attention_bias()     the attention block of matmul_cases with a bias on q, k, v and on the output projection, batch 2, a
                       constant attention bias [1,2,17,17] added to the scaled scores (its producer is a mul: that add runs on
                       its own) and hard-swish (hard_sigmoid -> mul) in front of the output projection
int8: every record is a power of two inside matmul's plan-time proof, so either matmul form equals chain_ref bit for bit.
binary16: the data keep every float32 partial sum exact where a one-ulp difference would grow (see each network).
"""
import numpy as np

import add_bcast_cases
import eltwise_cases
import matmul_cases as mc
import move_cases
import tail
from cases import pkg
from pool_cases import _q


class LinearNet(mc.MatmulNet):
    """layers: (kind, name, input or tuple of inputs, output, info) with kind matmul (info: trans_a, trans_b; a second input
    named in `consts` is a constant), addc (info: const, first), mulc (info: const), mul, add (two activations), softmax
    (info: axis), relu, hard_sigmoid, reshape, transpose (info: perm)"""

    def oracle(self, x):
        env = {self.in_name: x}
        en = lambda **kw: eltwise_cases.eltwise_numpy(dict(dtype=self.dtype, n=0.0, **kw))
        for kind, name, src, dst, info in self.layers:
            srcs = src if isinstance(src, tuple) else (src,)
            a = env[srcs[0]]
            if kind in self.MOVES:
                env[dst] = move_cases.move_numpy(self._move_case(kind, src, dst, info, a))
            elif kind == "matmul":
                env[dst] = mc.chain_ref(self._matmul_case(srcs, dst, info, a, env.get(srcs[1])))
            elif kind == "addc":
                env[dst] = add_bcast_cases.add_numpy(dict(dtype=self.dtype, x=a, y=self.consts[info["const"]][0], in_q=self.rec(src),
                                                          in1_q=self.crec(info["const"]), out_q=self.rec(dst),
                                                          small_first=bool(info.get("first"))))
            elif kind == "mulc":
                env[dst] = en(op="mul", x=a, y=self.consts[info["const"]][0], in_q=self.rec(src), in1_q=self.crec(info["const"]),
                              out_q=self.rec(dst))
            elif kind == "mul":
                env[dst] = en(op="mul", x=a, y=env[srcs[1]], in_q=self.rec(srcs[0]), in1_q=self.rec(srcs[1]), out_q=self.rec(dst))
            elif kind == "hard_sigmoid":
                env[dst] = en(op="hard_sigmoid", x=a, in_q=self.rec(src), out_q=self.rec(dst))
            elif kind == "add":
                env[dst] = tail.siso_oracle(dict(kind="add", x=a, y=env[srcs[1]], dtype=self.dtype, layout=self.layout, axis=1,
                                                 in_q=self.rec(srcs[0]), in1_q=self.rec(srcs[1]), out_q=self.rec(dst)))
            else:
                env[dst] = tail.siso_oracle(dict(kind=kind, x=a, dtype=self.dtype, layout=self.layout, axis=info.get("axis", 1),
                                                 in_q=self.rec(src), out_q=self.rec(dst)))
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
        act_l = pkg.LAYOUT_NHWC if self.layout == "NHWC" else pkg.LAYOUT_NCHW
        by_rank = lambda n: {1: pkg.LAYOUT_N, 2: pkg.LAYOUT_NC}.get(n, act_l)

        def T(dims, rec, name, data=None, const=0):
            return pkg.make_tensor(fe, keep, dims, dt, by_rank(len(dims)), data=data, is_const=const, name=name, sess=sess,
                                   scales=(rec[0],), zps=(rec[1],))
        A = lambda name: T(self.shape(name), self.rec(name), name.encode())
        K = lambda name: T(self.consts[name][0].shape, self.crec(name), name.encode(), self.consts[name][0], 1)
        P = lambda kind, nm, axis=1: pkg.siso_params(fe, keep, api, kind, act_l, axis, sess, nm)
        env = {self.in_name: A(self.in_name)}
        ops = []
        for kind, name, src, dst, info in self.layers:
            srcs = src if isinstance(src, tuple) else (src,)
            env[dst] = A(dst)
            nm = name.encode()
            if kind in self.MOVES:
                p = move_cases.op_params(fe, keep, api, self._move_case(kind, src, dst, info), sess, layout=act_l)
                ops.append(("csinn_" + kind, (env[src], env[dst], p)))
            elif kind == "matmul":
                second = K(srcs[1]) if srcs[1] in self.consts else env[srcs[1]]
                p = pkg.matmul_params(fe, keep, api, act_l, info.get("trans_a"), info.get("trans_b"), sess, nm)
                ops.append(("csinn_matmul", (env[srcs[0]], second, env[dst], p)))
            elif kind == "addc":
                pair = (K(info["const"]), env[src]) if info.get("first") else (env[src], K(info["const"]))
                ops.append(("csinn_add", pair + (env[dst], P("add", nm))))
            elif kind == "mulc":
                ops.append(("csinn_mul", (env[src], K(info["const"]), env[dst], P("mul", nm))))
            elif kind in ("add", "mul"):
                ops.append(("csinn_" + kind, (env[srcs[0]], env[srcs[1]], env[dst], P(kind, nm))))
            else:
                ops.append(("csinn_" + kind, (env[src], env[dst], P(kind, nm, info.get("axis", 1)))))
        outputs = [env[o] for o in self.outputs]
        fe.csinn_set_input_number(1, sess)
        fe.csinn_set_output_number(len(outputs), sess)
        for stem, args in ops:
            assert getattr(fe, stem + "_init")(*args) == pkg.CSINN_TRUE, stem
        fe.csinn_set_tensor_entry(env[self.in_name], sess)
        fe.csinn_set_input(0, env[self.in_name], sess)
        for stem, args in ops:
            assert getattr(fe, stem)(*args) == pkg.CSINN_TRUE, stem
        for i, t in enumerate(outputs):
            fe.csinn_set_output(i, t, sess)
        rc = fe.csinn_session_setup(sess)
        assert rc == pkg.CSINN_TRUE or getattr(fe, "kind", "") == "reference"
        self._keep, self._sess, self.layer_count = keep, sess, len(ops)
        return sess


def _bias(rng, n, dtype, grid):
    if dtype == "int8":
        return rng.integers(-128, 128, (n,), dtype=np.int8)
    lo, hi, step = grid
    return (rng.integers(lo, hi + 1, (n,)) * step).astype(np.float16)


def mlp(dtype="int8", layout="NHWC"):
    """binary16: x is a multiple of 1/16 in [-2, 2], W1 and W2 multiples of 1/64 in [-1/16, 1/16], the biases multiples of 1/16
    in [-1, 1].  x W1 then sums multiples of 2^-10 below 8: exact, so the hidden layer is the same bits in either matmul form;
    it stays below 16 on the 2^-10 grid, and x W2's partial sums (multiples of 2^-16 below 128) are exact as well"""
    q = lambda s, z: _q(2.0 ** s, z)
    rng = np.random.default_rng(91)
    x, h = (2, 17, 64), (2, 17, 128)
    t = {"x": (x, q(-4, -5)), "h1m": (h, q(-4, 3)), "h1": (h, q(-4, 6)), "r": (h, q(-5, -128)), "h2m": (x, q(-4, -3)), "h2": (x, q(-4, 2)),
         "out": (x, q(-3, 7))}
    small = (-4, 4, 1.0 / 64)
    consts = {"W1": (mc._weights(rng, (64, 128), dtype, small), q(-10, 0)), "b1": (_bias(rng, 128, dtype, (-16, 16, 1.0 / 16)), q(-5, 4)),
              "W2": (mc._weights(rng, (128, 64), dtype, small), q(-10, 5)), "b2": (_bias(rng, 64, dtype, (-16, 16, 1.0 / 16)), q(-5, -9))}
    L = [("matmul", "fc1", ("x", "W1"), "h1m", {}),
         ("addc", "fc1_bias", "h1m", "h1", dict(const="b1")),
         ("relu", "relu", "h1", "r", {}),
         ("matmul", "fc2", ("r", "W2"), "h2m", {}),
         ("addc", "fc2_bias", "h2m", "h2", dict(const="b2", first=True)),
         ("add", "residual", ("h2", "x"), "out", {})]
    return LinearNet(dtype, layout, 93, "x", t, L, ["out"], consts, x_grid=(-32, 32, 1.0 / 16))


def attention_bias(dtype="int8", layout="NCHW"):
    """matmul_cases.attention_block (its data rules hold here too) at batch 2, with biases.  binary16: bq, bk are multiples of
    2^-5 in [-1, 1], so q and k stay exact multiples of 2^-5 below 64 and every partial sum of q k^T exact: the scores, the
    attention bias added to them and p are the same bits in either matmul form; bv, bo and the attention bias are non-negative,
    and hard-swish of a non-negative value is monotone, so everything behind the softmax stays a sum of non-negative terms"""
    q = lambda s, z: _q(2.0 ** s, z)
    rng = np.random.default_rng(97)
    s, c, h, hd, n = 17, 64, 2, 32, 2
    flat, split, heads, scores = (n, s, c), (n, s, h, hd), (n, h, s, hd), (n, h, s, s)
    t = {"x": (flat, q(-4, -5)), "out": (flat, q(-3, 7)), "projm": (flat, q(-3, -100)), "proj": (flat, q(-3, -90)),
         "s": (scores, q(-1, 5)), "sc": (scores, q(-3, 5)), "sb": (scores, q(-3, -9)), "p": (scores, _q(1.0 / 256, -128)),
         "oh": (heads, q(-4, 3)), "os": (split, q(-4, 3)), "o": (flat, q(-4, 3)), "hs": (flat, q(-7, -128)), "ox": (flat, q(-4, -40))}
    for nm, zp in (("q", -3), ("k", 0), ("v", 3)):
        t[nm + "m"] = (flat, q(-4, zp))
        t[nm] = (flat, q(-4, zp + 4))
        t[nm + "s"] = (split, q(-4, zp + 4))
        t[nm + "h"] = (heads, q(-4, zp + 4))
    signed, positive = (-1, 1, 1.0 / 8), (0, 2, 1.0 / 16)
    W = lambda grid: mc._weights(rng, (c, c), dtype, grid)
    consts = {"Wq": (W(signed), q(-10, 0)), "Wk": (W(signed), q(-10, 5)), "Wv": (W(positive), q(-10, 0)), "Wo": (W(positive), q(-10, -128)),
              "bq": (_bias(rng, c, dtype, (-32, 32, 1.0 / 32)), q(-6, 3)), "bk": (_bias(rng, c, dtype, (-32, 32, 1.0 / 32)), q(-6, -7)),
              "bv": (_bias(rng, c, dtype, (0, 16, 1.0 / 16)), q(-6, 0)), "bo": (_bias(rng, c, dtype, (0, 16, 1.0 / 16)), q(-6, 11)),
              "scale": (np.array([90], np.int8) if dtype == "int8" else np.array([0.17578125], np.float16), q(-9, 0)),
              "ab": (rng.integers(-128, 128, (1, h, s, s), dtype=np.int8) if dtype == "int8" else
                     (rng.integers(0, 33, (1, h, s, s)) / 16.0).astype(np.float16), q(-5, 0))}
    L = []
    for nm in "qkv":
        L += [("matmul", nm, ("x", "W" + nm), nm + "m", {}),
              ("addc", nm + "_bias", nm + "m", nm, dict(const="b" + nm, first=nm == "k")),
              ("reshape", nm + "_split", nm, nm + "s", {}),
              ("transpose", nm + "_heads", nm + "s", nm + "h", dict(perm=(0, 2, 1, 3)))]
    L += [("matmul", "qk", ("qh", "kh"), "s", dict(trans_b=True)),
          ("mulc", "scaled", "s", "sc", dict(const="scale")),
          ("addc", "attn_bias", "sc", "sb", dict(const="ab")),
          ("softmax", "softmax", "sb", "p", dict(axis=3)),
          ("matmul", "pv", ("p", "vh"), "oh", {}),
          ("transpose", "o_tokens", "oh", "os", dict(perm=(0, 2, 1, 3))),
          ("reshape", "o_merge", "os", "o", {}),
          ("hard_sigmoid", "hswish_gate", "o", "hs", {}),
          ("mul", "hswish", ("o", "hs"), "ox", {}),
          ("matmul", "proj", ("ox", "Wo"), "projm", {}),
          ("addc", "proj_bias", "projm", "proj", dict(const="bo")),
          ("add", "residual", ("proj", "x"), "out", {})]
    return LinearNet(dtype, layout, 99, "x", t, L, ["out", "p"], consts, x_grid=(0, 8, 1.0 / 4))


NETS = {"mlp": mlp, "attention_bias": attention_bias}
FUSED_LINEARS = {"mlp": 2, "attention_bias": 4}

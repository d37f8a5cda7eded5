"""The skip-connection networks of tests/residual_nets.py as binary16 NHWC sessions, plus a bottleneck tail:

  basic_block       conv3x3 -> add(conv, x) -> relu
  bottleneck_tail   conv1x1 reduce + relu -> conv1x1 expand -> add(expand, x) -> relu   (ResNet-50: the expansion fuses)
  inverted_block    pw expand + relu6 -> dw3x3 + relu6 -> pw project -> add(x, proj)    (no activation behind the sum)
  projection_block  the add directly follows the SHORTCUT convolution, which is the one that fuses
  two_consumers / broadcast_block / the NCHW copy: outside the scope

Sizes keep every convolution on the wave kernel in both sessions (at most a few wave tiles, no row-patch or block-tile grid), so
that the fused launch and the layers apart add K up in one order and the outputs can be compared on bits.
"""
import numpy as np

import residual_nets as rn
from residual_nets import SkipNet, q


def basic_block(layout="NHWC", export_conv=False):
    return rn.basic_block("f16", layout, export_conv)


def bottleneck_tail(layout="NHWC"):
    t = {"x": (64, 10, q(0, 0)), "m": (16, 10, q(0, 0)), "e": (64, 10, q(0, 0)), "sum": (64, 10, q(0, 0)), "out": (64, 10, q(0, 0))}
    L = [("conv", "reduce", ["x"], ["m"], dict(act=1)), ("conv", "expand", ["m"], ["e"], {}), ("add", "add", ["e", "x"], ["sum"], {}),
         ("relu", "relu", ["sum"], ["out"], {})]
    return SkipNet("f16", layout, 71, "x", t, L, ["out"])


def inverted_block(layout="NHWC"):
    return rn.inverted_block("f16", layout)


def projection_block(layout="NHWC"):
    return rn.projection_block("f16", layout)


def broadcast_block(layout="NHWC"):
    net = rn.broadcast_block("f16", layout)
    net.consts = {"pc": np.random.default_rng(72).standard_normal(net.shape("pc")).astype(np.float16)}
    return net


# name -> (constructor, the convolution whose launch carries the tail)
FUSING = {"basic_block": (basic_block, "conv"), "bottleneck_tail": (bottleneck_tail, "expand"), "inverted_block": (inverted_block, "project"),
          "projection_block": (projection_block, "shortcut")}

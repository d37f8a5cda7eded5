"""What the backend registers, pinned: for every op id and both dtypes, whether shl_cb_map_mi355x returns a callback, whether
it has an init, and which exported function its exec is.  The literal below was dumped from the library built at the commit
before the operator table of setup.c replaced the registration list and the session's own table; it is not derived from the
table.  Needs no GPU."""
import ctypes as C
import subprocess

import pytest

from cases import pkg

OP_SIZE = 194  # CSINN_OP_SIZE (include/csinn/csinn_data_structure.h)
DTYPE_SIZE = 13  # CSINN_DTYPE_SIZE
DTYPES = {"i8": (pkg.DTYPE_INT8,), "i8+f16": (pkg.DTYPE_INT8, pkg.DTYPE_FLOAT16)}

# (op id, dtypes, init present, <name> of the exported shl_mi355x_<name>_exec that exec equals)
REGISTERED = [
    (3, "i8+f16", False, "add"),  # CSINN_OP_ADD
    (14, "i8+f16", False, "avgpool2d"),  # CSINN_OP_AVGPOOL2D
    (26, "i8+f16", False, "concat"),  # CSINN_OP_CONCAT
    (28, "i8+f16", True, "conv2d"),  # CSINN_OP_CONV2D
    (29, "i8+f16", True, "conv2d"),  # CSINN_OP_CONV2D_RELU
    (30, "i8+f16", True, "conv2d"),  # CSINN_OP_CONV2D_RELU6
    (31, "i8", True, "conv2d_channel"),  # CSINN_OP_CONV2D_CHANNEL
    (32, "i8", True, "conv2d_channel_relu"),  # CSINN_OP_CONV2D_CHANNEL_RELU
    (33, "i8", True, "conv2d_channel_relu6"),  # CSINN_OP_CONV2D_CHANNEL_RELU6
    (35, "i8+f16", True, "conv2d"),  # CSINN_OP_DEPTHWISE_CONV2D
    (36, "i8+f16", True, "conv2d"),  # CSINN_OP_DEPTHWISE_CONV2D_RELU
    (37, "i8+f16", True, "conv2d"),  # CSINN_OP_DEPTHWISE_CONV2D_RELU6
    (38, "i8", True, "depthwise_conv2d_channel"),  # CSINN_OP_DEPTHWISE_CONV2D_CHANNEL
    (39, "i8", True, "depthwise_conv2d_channel_relu"),  # CSINN_OP_DEPTHWISE_CONV2D_CHANNEL_RELU
    (40, "i8", True, "depthwise_conv2d_channel_relu6"),  # CSINN_OP_DEPTHWISE_CONV2D_CHANNEL_RELU6
    (42, "i8+f16", True, "group_conv2d"),  # CSINN_OP_GROUP_CONV2D
    (43, "i8+f16", True, "group_conv2d"),  # CSINN_OP_GROUP_CONV2D_RELU
    (44, "i8+f16", True, "group_conv2d"),  # CSINN_OP_GROUP_CONV2D_RELU6 (the stand-alone front-end has an est for it)
    (45, "i8", True, "group_conv2d_channel"),  # CSINN_OP_GROUP_CONV2D_CHANNEL
    (46, "i8", True, "group_conv2d_channel_relu"),  # CSINN_OP_GROUP_CONV2D_CHANNEL_RELU
    (54, "i8+f16", True, "deconv2d"),  # CSINN_OP_DECONV2D
    (55, "i8+f16", True, "deconv2d"),  # CSINN_OP_DEPTHWISE_DECONV2D
    (56, "i8+f16", True, "deconv2d"),  # CSINN_OP_GROUP_DECONV2D
    (66, "i8+f16", True, "flatten"),  # CSINN_OP_FLATTEN
    (71, "i8+f16", True, "fullyconnected"),  # CSINN_OP_FULLYCONNECTED
    (74, "i8+f16", False, "global_avgpool2d"),  # CSINN_OP_GLOBAL_AVGPOOL2D
    (75, "i8+f16", True, "global_maxpool2d"),  # CSINN_OP_GLOBAL_MAXPOOL2D
    (78, "i8+f16", False, "hard_sigmoid"),  # CSINN_OP_HARD_SIGMOID
    (84, "i8+f16", False, "leaky_relu"),  # CSINN_OP_LEAKY_RELU
    (95, "i8+f16", True, "matmul"),  # CSINN_OP_MATMUL
    (96, "i8+f16", True, "max"),  # CSINN_OP_MAX
    (98, "i8+f16", False, "maxpool2d"),  # CSINN_OP_MAXPOOL2D
    (101, "i8+f16", True, "mean"),  # CSINN_OP_MEAN
    (103, "i8+f16", True, "min"),  # CSINN_OP_MIN
    (107, "i8+f16", False, "mul"),  # CSINN_OP_MUL
    (115, "i8+f16", True, "pad"),  # CSINN_OP_PAD
    (122, "i8+f16", True, "reduce_max"),  # CSINN_OP_REDUCE_MAX
    (123, "i8+f16", True, "reduce_mean"),  # CSINN_OP_REDUCE_MEAN
    (124, "i8+f16", True, "reduce_min"),  # CSINN_OP_REDUCE_MIN
    (126, "i8+f16", True, "reduce_sum"),  # CSINN_OP_REDUCE_SUM
    (127, "i8+f16", False, "relu"),  # CSINN_OP_RELU
    (129, "i8+f16", False, "relu6"),  # CSINN_OP_RELU6
    (132, "i8+f16", True, "reshape"),  # CSINN_OP_RESHAPE
    (133, "i8+f16", False, "resize"),  # CSINN_OP_RESIZE
    (153, "i8+f16", True, "shuffle_channel"),  # CSINN_OP_SHUFFLE_CHANNEL
    (154, "i8+f16", False, "sigmoid"),  # CSINN_OP_SIGMOID
    (159, "i8+f16", False, "softmax"),  # CSINN_OP_SOFTMAX
    (166, "i8+f16", True, "split"),  # CSINN_OP_SPLIT
    (173, "i8+f16", True, "sum"),  # CSINN_OP_SUM
    (179, "i8+f16", True, "transpose"),  # CSINN_OP_TRANSPOSE
    (190, "i8+f16", False, "silu"),  # CSINN_OP_SILU
]


@pytest.fixture(scope="module")
def cb_map(standalone):
    _, _, opt = standalone
    opt.shl_cb_map_mi355x.restype = C.POINTER(pkg.Callback)
    opt.shl_cb_map_mi355x.argtypes = [C.c_int, C.c_int]
    return opt


def _address(opt, symbol):
    return C.cast(getattr(opt, symbol), C.c_void_p).value


@pytest.mark.parametrize("op,dtypes,has_init,name", REGISTERED, ids=["op%d_%s" % (r[0], r[3]) for r in REGISTERED])
def test_registered_pairs_have_the_recorded_callbacks(cb_map, op, dtypes, has_init, name):
    want = _address(cb_map, "shl_mi355x_%s_exec" % name)
    for dt in DTYPES[dtypes]:
        cb = cb_map.shl_cb_map_mi355x(op, dt)
        assert cb, (op, dt)
        assert cb.contents.exec == want, (op, dt)
        assert bool(cb.contents.init) == has_init, (op, dt)
        assert cb.contents.est and cb.contents.caps and cb.contents.perf, (op, dt)


def test_no_other_pair_reaches_a_callback_of_the_backend(cb_map):
    """every other (op, dtype) has no callback at all, or -- next to a library with shl_cb_map_ref -- the reference's"""
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.lib_path("libshl_mi355x_opt.so")], capture_output=True, text=True,
                         check=True).stdout
    own = {_address(cb_map, ln.split()[-1]) for ln in out.splitlines() if ln.split() and ln.split()[-1].endswith("_exec")}
    assert len(own) >= len({r[3] for r in REGISTERED})
    registered = {(op, dt) for op, dtypes, _, _ in REGISTERED for dt in DTYPES[dtypes]}
    assert len(registered) == 94
    for op in range(OP_SIZE + 4):  # (and the utility ids behind the operators)
        for dt in range(DTYPE_SIZE):
            if (op, dt) in registered:
                continue
            cb = cb_map.shl_cb_map_mi355x(op, dt)
            assert not cb or cb.contents.exec not in own, (op, dt)

"""csi-nn2_amd -- MI355X (gfx950) backend for the CSI-NN2 / SHL operator API.

Python is only the loader and test/bench harness: the product is three native libraries
(see build.py).  This module mirrors the C structs with ctypes and exposes thin helpers that
call the *C* entry points (csinn_conv2d_init / csinn_conv2d / ...), exactly as a C user of the
reference would.  The directory name contains a hyphen (it is the reference's name plus
``_amd``), so import it with ``importlib.import_module("csi-nn2_amd")`` (tests/conftest.py does).

Nothing in here computes: without the HIP library and a gfx950 device every compute call
fails loudly (MI355XError).
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_DIR = os.path.join(HERE, "lib")

# ---- enum values (include/csinn/csinn_data_structure.h) -------------------------------------
DTYPE_INT8, DTYPE_INT32, DTYPE_FLOAT16, DTYPE_FLOAT32 = 3, 7, 8, 10
MEM_CPU, MEM_DMABUF, MEM_CPU_ACC = 0, 2, 5
QUANT_INT8_ASYM_W_SYM, QUANT_FLOAT16 = 11, 7
API_REF, API_GREF, API_MI355X = 0, 1, 14
RM_LAYER, RM_CPU_GRAPH = 0, 1
LAYOUT_N, LAYOUT_NC, LAYOUT_NCHW, LAYOUT_O, LAYOUT_OI, LAYOUT_OIHW, LAYOUT_O1HW = 1, 2, 4, 6, 7, 11, 13
LAYOUT_NHWC, LAYOUT_OHWI, LAYOUT_1HWO = 15, 18, 22
CSINN_TRUE = 1
OP_CONV2D, OP_CONV2D_RELU, OP_CONV2D_RELU6 = 28, 29, 30
OP_DEPTHWISE_CONV2D, OP_FULLYCONNECTED = 35, 71
OP_AVGPOOL2D, OP_MAXPOOL2D = 14, 98
OP_CONCAT = 26
OP_SPLIT, OP_SHUFFLE_CHANNEL = 166, 153
OP_TRANSPOSE, OP_RESHAPE, OP_FLATTEN, OP_PAD = 179, 132, 66, 115
PAD_CONSTANT, PAD_EDGE, PAD_REFLECT = 0, 1, 2
OP_MEAN, OP_SUM, OP_MAX, OP_MIN = 101, 173, 96, 103
OP_REDUCE_MEAN, OP_REDUCE_SUM, OP_REDUCE_MAX, OP_REDUCE_MIN = 123, 126, 122, 124
OP_GLOBAL_MAXPOOL2D = 75
REDUCE_SUM, REDUCE_MEAN, REDUCE_MAX, REDUCE_MIN = 0, 1, 2, 3   # shl_mi355x_reduce_desc.kind
REDUCE_INIT_FLT_MAX, REDUCE_INIT_FIRST = 0, 1                   # .init
REDUCE_GROUPS, REDUCE_CHUNK_BYTES = 4, 256
OP_MATMUL = 95
MATMUL_CHAIN, MATMUL_MFMA, MATMUL_MFMA_MAX_K = "matmul_chain", "matmul_mfma", 32768  # shl_mi355x_matmul's forms
ATTENTION_MFMA, ATTENTION_MAX_KEYS = "attention_mfma", 1024  # shl_mi355x_attention's kernel and its cap on the keys
ATTENTION_BIAS_MFMA = "attention_bias_mfma"  # shl_mi355x_attention_bias's kernel
ATTENTION_LAYOUT_MFMA, ATTENTION_BIAS_LAYOUT_MFMA = "attention_layout_mfma", "attention_bias_layout_mfma"  # shl_mi355x_attention_layout's
OP_SIGMOID, OP_HARD_SIGMOID, OP_SILU, OP_LEAKY_RELU, OP_MUL = 154, 78, 190, 84, 107
OP_RESIZE = 133
OP_DECONV2D, OP_DEPTHWISE_DECONV2D, OP_GROUP_DECONV2D = 54, 55, 56
LAYOUT_IOHW = 31
RESIZE_BILINEAR, RESIZE_NEAREST_NEIGHBOR, RESIZE_NEAREST_BICUBIC = 0, 1, 2  # enum csinn_resize_enum

SHL_NHWC, SHL_NCHW = 0, 1
SHL_I8, SHL_F16 = 0, 1
POOL_MAX, POOL_AVG = 0, 1
UNARY_SIGMOID, UNARY_HARD_SIGMOID, UNARY_SILU, UNARY_LEAKY_RELU = 0, 1, 2, 3
ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
ALGO_AUTO, ALGO_DIRECT, ALGO_IGEMM, ALGO_DW, ALGO_GEMV, ALGO_STEM = 0, 1, 2, 3, 4, 5
ALGO_DECONV_GATHER, ALGO_DECONV_PHASE = 8, 9


class MI355XError(RuntimeError):
    pass


# ---- struct mirrors --------------------------------------------------------------------------
class QuantInfo(C.Structure):
    _fields_ = [("zero_point", C.c_int32), ("scale", C.c_float), ("multiplier", C.c_int32),
                ("shift", C.c_int32), ("min", C.c_float), ("max", C.c_float)]


class Session(C.Structure):
    pass


class Tensor(C.Structure):
    _fields_ = [("data", C.c_void_p), ("dtype", C.c_int32), ("mtype", C.c_int32),
                ("dim", C.c_int32 * 8), ("dim_count", C.c_int32), ("is_const", C.c_uint32),
                ("name", C.c_char_p), ("layout", C.c_int32), ("quant_channel", C.c_int32),
                ("qinfo", C.POINTER(QuantInfo)), ("sess", C.POINTER(Session))]


class Model(C.Structure):
    _fields_ = [("bm_path", C.c_char_p), ("bm_addr", C.c_void_p), ("bm_size", C.c_size_t),
                ("save_mode", C.c_int32), ("priority", C.c_int32)]


Session._fields_ = [("base_dtype", C.c_int32), ("base_layout", C.c_int32),
                    ("base_api", C.c_int32), ("base_run_mode", C.c_int32),
                    ("base_quant_type", C.c_int32), ("model", Model),
                    ("debug_level", C.c_int32), ("profiler_level", C.c_int32),
                    ("input_num", C.c_int32), ("output_num", C.c_int32),
                    ("input", C.POINTER(C.POINTER(Tensor))),
                    ("output", C.POINTER(C.POINTER(Tensor))), ("td", C.c_void_p),
                    ("dynamic_shape", C.c_bool), ("trace", C.c_void_p)]


class Callback(C.Structure):
    _fields_ = [("init", C.c_void_p), ("est", C.c_void_p), ("exec", C.c_void_p),
                ("caps", C.c_void_p), ("perf", C.c_void_p)]


class ParamsBase(C.Structure):
    _fields_ = [("cb", C.POINTER(Callback)), ("name", C.c_char_p), ("layout", C.c_int32),
                ("api", C.c_int32), ("quant_type", C.c_int32), ("sess", C.POINTER(Session))]


class ConvExtra(C.Structure):
    _fields_ = [("kernel_tm", C.c_void_p), ("conv_mode", C.c_int32), ("fuse_zp2bias", C.c_int32)]


class Conv2dParams(C.Structure):
    _fields_ = [("base", ParamsBase), ("group", C.c_int32), ("stride_height", C.c_int32),
                ("stride_width", C.c_int32), ("pad_top", C.c_int32), ("pad_left", C.c_int32),
                ("pad_down", C.c_int32), ("pad_right", C.c_int32),
                ("dilation_height", C.c_int32), ("dilation_width", C.c_int32),
                ("out_pad_height", C.c_int32), ("out_pad_width", C.c_int32),
                ("conv_extra", ConvExtra)]


class FcExtra(C.Structure):
    _fields_ = [("fuse_zp2bias", C.c_int32)]


class FcParams(C.Structure):
    _fields_ = [("base", ParamsBase), ("units", C.c_int32), ("fc_extra", FcExtra)]


class ReluParams(C.Structure):
    _fields_ = [("base", ParamsBase), ("n", C.c_float), ("n_multiplier", C.c_int32),
                ("n_shift", C.c_int32)]


class DisoParams(C.Structure):
    _fields_ = [("base", ParamsBase)]


class SigmoidParams(C.Structure):
    _fields_ = [("base", ParamsBase)]


class ResizeParams(C.Structure):
    _fields_ = [("base", ParamsBase), ("resize_mode", C.c_int32), ("align_corners", C.c_bool)]


class SoftmaxParams(C.Structure):
    _fields_ = [("base", ParamsBase), ("axis", C.c_int32)]


class PoolParams(C.Structure):
    _fields_ = [("base", ParamsBase)] + [(n, C.c_int32) for n in (
        "pool_type", "filter_height", "filter_width", "filter_depth", "stride_height", "stride_width",
        "stride_depth", "pad_top", "pad_left", "pad_down", "pad_right", "pad_front", "pad_back",
        "ceil_mode")] + [("count_include_pad", C.c_bool)]


class ConcatParams(C.Structure):
    _fields_ = [("base", ParamsBase), ("inputs_count", C.c_int32), ("axis", C.c_int32)]


class SplitParams(C.Structure):
    _fields_ = [("base", ParamsBase), ("split_index", C.POINTER(C.c_int32)), ("output_num", C.c_int32), ("axis", C.c_int32)]


class ShuffleChannelParams(C.Structure):
    _fields_ = [("base", ParamsBase), ("group", C.c_int32)]


class TransposeParams(C.Structure):
    _fields_ = [("base", ParamsBase), ("permute", C.POINTER(C.c_int32)), ("permute_num", C.c_int32)]


class ReshapeParams(C.Structure):
    _fields_ = [("base", ParamsBase), ("shape", C.POINTER(C.c_int32)), ("shape_num", C.c_int32)]


class FlattenParams(C.Structure):
    _fields_ = [("base", ParamsBase), ("axis", C.c_int32)]


class PadParams(C.Structure):
    _fields_ = [("base", ParamsBase), ("pad_before", C.POINTER(C.c_int32)), ("pad_after", C.POINTER(C.c_int32)),
                ("pad_num", C.c_int32), ("pad_value", C.c_float), ("pad_mode", C.c_int32)]


class ReduceParams(C.Structure):
    """struct csinn_reduce_params (include/csinn/csinn_data_structure.h)"""
    _fields_ = [("base", ParamsBase), ("out_strides", C.POINTER(C.c_int32)), ("out_extents", C.POINTER(C.c_int32)),
                ("n", C.c_int32), ("inner_strides", C.POINTER(C.c_int32)), ("inner_extents", C.POINTER(C.c_int32)),
                ("m", C.c_int32), ("axis", C.POINTER(C.c_int32)), ("axis_count", C.c_int32), ("keepdims", C.c_bool)]


class MatmulParams(C.Structure):
    """struct csinn_matmul_params (include/csinn/csinn_data_structure.h)"""
    _fields_ = [("base", ParamsBase), ("trans_a", C.c_bool), ("trans_b", C.c_bool)]


class MatmulDesc(C.Structure):
    """struct shl_mi355x_matmul_desc (include/shl_mi355x.h)"""
    _fields_ = [("dtype", C.c_int32), ("batches", C.c_int32), ("m", C.c_int32), ("n", C.c_int32), ("k", C.c_int32),
                ("reserved0", C.c_int32),
                ("a_batch_stride", C.c_int64), ("a_row_stride", C.c_int64), ("a_k_stride", C.c_int64),
                ("b_batch_stride", C.c_int64), ("b_col_stride", C.c_int64), ("b_k_stride", C.c_int64),
                ("a_elems", C.c_int64), ("b_elems", C.c_int64), ("out_elems", C.c_int64),
                ("a_scale", C.c_float), ("a_zp", C.c_int32), ("b_scale", C.c_float), ("b_zp", C.c_int32),
                ("out_scale", C.c_float), ("out_zp", C.c_int32), ("reserved", C.c_int32 * 4)]


class AttentionDesc(C.Structure):
    """struct shl_mi355x_attention_desc (include/shl_mi355x.h)"""
    _fields_ = [(n, C.c_int32) for n in ("dtype", "batches", "s", "t", "d", "dv", "has_scale", "scale_is_first", "scale_raw",
                                         "reserved0")] + \
        [(n, C.c_float) for n in ("q_scale", "k_scale", "v_scale", "s_scale", "c_scale", "sc_scale", "p_scale", "out_scale")] + \
        [(n, C.c_int32) for n in ("q_zp", "k_zp", "v_zp", "s_zp", "c_zp", "sc_zp", "p_zp", "out_zp")] + \
        [("reserved", C.c_int32 * 4)]


class AttentionBiasDesc(C.Structure):
    """struct shl_mi355x_attention_bias_desc (include/shl_mi355x.h)"""
    _fields_ = [("b_ext1", C.c_int32), ("bias_is_first", C.c_int32), ("b_stride", C.c_int64 * 2), ("row_stride", C.c_int64),
                ("key_stride", C.c_int64), ("b_scale", C.c_float), ("b_zp", C.c_int32), ("sb_scale", C.c_float), ("sb_zp", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class ResidualDesc(C.Structure):
    """struct shl_mi355x_residual_desc (include/shl_mi355x.h)"""
    _fields_ = [("conv_first", C.c_int32), ("skip_scale", C.c_float), ("skip_zp", C.c_int32), ("sum_scale", C.c_float),
                ("sum_zp", C.c_int32), ("act", C.c_int32), ("out_scale", C.c_float), ("out_zp", C.c_int32)]


class ConvDesc(C.Structure):
    """struct shl_mi355x_conv_desc (include/shl_mi355x.h)"""
    _fields_ = [(n, C.c_int32) for n in (
        "layout", "dtype", "act", "algo", "batch", "in_h", "in_w", "in_c", "out_h", "out_w",
        "out_c", "kernel_h", "kernel_w", "stride_h", "stride_w", "pad_top", "pad_left",
        "dilation_h", "dilation_w", "group", "in_zp", "out_zp")] + \
        [("out_scale", C.c_float), ("reserved", C.c_int32 * 4)]


class PoolDesc(C.Structure):
    """struct shl_mi355x_pool_desc (include/shl_mi355x.h)"""
    _fields_ = [(n, C.c_int32) for n in (
        "kind", "dtype", "layout", "batch", "c", "in_h", "in_w", "out_h", "out_w", "kernel_h", "kernel_w",
        "stride_h", "stride_w", "pad_top", "pad_left", "count_include_pad", "in_zp", "out_zp")] + \
        [("in_scale", C.c_float), ("out_scale", C.c_float), ("reserved", C.c_int32 * 4)]


class ConcatDesc(C.Structure):
    """struct shl_mi355x_concat_desc (include/shl_mi355x.h)"""
    _fields_ = [("dtype", C.c_int32), ("n_inputs", C.c_int32), ("outer", C.c_int64), ("out_scale", C.c_float),
                ("out_zp", C.c_int32), ("reserved", C.c_int32 * 4)]


class SplitDesc(C.Structure):
    """struct shl_mi355x_split_desc (include/shl_mi355x.h)"""
    _fields_ = [("dtype", C.c_int32), ("n_outputs", C.c_int32), ("outer", C.c_int64), ("in_scale", C.c_float),
                ("in_zp", C.c_int32), ("reserved", C.c_int32 * 4)]


class AttentionLayoutDesc(C.Structure):
    """struct shl_mi355x_attention_layout_desc (include/shl_mi355x.h)"""
    _fields_ = [("heads", C.c_int32), ("moved", C.c_int32), ("q_stride", C.c_int32 * 3), ("k_stride", C.c_int32 * 3),
                ("v_stride", C.c_int32 * 3), ("out_stride", C.c_int32 * 3), ("reserved", C.c_int32 * 2)]


class ShuffleDesc(C.Structure):
    """struct shl_mi355x_shuffle_desc (include/shl_mi355x.h)"""
    _fields_ = [("dtype", C.c_int32), ("group", C.c_int32), ("outer", C.c_int64), ("c", C.c_int64), ("inner", C.c_int64),
                ("in_scale", C.c_float), ("in_zp", C.c_int32), ("out_scale", C.c_float), ("out_zp", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class TransposeDesc(C.Structure):
    """struct shl_mi355x_transpose_desc (include/shl_mi355x.h)"""
    _fields_ = [("dtype", C.c_int32), ("rank", C.c_int32), ("dim", C.c_int32 * 8), ("perm", C.c_int32 * 8),
                ("in_scale", C.c_float), ("in_zp", C.c_int32), ("out_scale", C.c_float), ("out_zp", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class MoveDesc(C.Structure):
    """struct shl_mi355x_move_desc (include/shl_mi355x.h)"""
    _fields_ = [("dtype", C.c_int32), ("in_scale", C.c_float), ("in_zp", C.c_int32), ("out_scale", C.c_float),
                ("out_zp", C.c_int32), ("reserved", C.c_int32 * 3)]


class PadDesc(C.Structure):
    """struct shl_mi355x_pad_desc (include/shl_mi355x.h)"""
    _fields_ = [("dtype", C.c_int32), ("dim", C.c_int32 * 4), ("before", C.c_int32 * 4), ("after", C.c_int32 * 4),
                ("pad_value", C.c_float), ("in_scale", C.c_float), ("in_zp", C.c_int32), ("out_scale", C.c_float),
                ("out_zp", C.c_int32), ("reserved", C.c_int32 * 4)]


class ReduceDesc(C.Structure):
    """struct shl_mi355x_reduce_desc (include/shl_mi355x.h)"""
    _fields_ = [("dtype", C.c_int32), ("kind", C.c_int32), ("init", C.c_int32), ("n_out", C.c_int32), ("n_inner", C.c_int32),
                ("out_extent", C.c_int32 * 8), ("out_stride", C.c_int32 * 8), ("inner_extent", C.c_int32 * 8),
                ("inner_stride", C.c_int32 * 8), ("reserved0", C.c_int32), ("in_elems", C.c_int64),
                ("in_scale", C.c_float), ("in_zp", C.c_int32), ("out_scale", C.c_float), ("out_zp", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class ResizeDesc(C.Structure):
    """struct shl_mi355x_resize_desc (include/shl_mi355x.h)"""
    _fields_ = [(n, C.c_int32) for n in ("dtype", "layout", "n", "c", "in_h", "in_w", "out_h", "out_w", "mode", "align_corners")] + \
        [("height_scale", C.c_float), ("width_scale", C.c_float), ("in_scale", C.c_float), ("out_scale", C.c_float),
         ("in_zp", C.c_int32), ("out_zp", C.c_int32), ("table", C.c_uint8 * 256), ("reserved", C.c_int32 * 4)]


class MulDesc(C.Structure):
    """struct shl_mi355x_mul_desc (include/shl_mi355x.h)"""
    _fields_ = [("dtype", C.c_int32), ("ngroups", C.c_int32), ("dim", C.c_int64 * 4), ("b_stride", C.c_int64 * 4),
                ("a_scale", C.c_float), ("b_scale", C.c_float), ("out_scale", C.c_float),
                ("a_zp", C.c_int32), ("b_zp", C.c_int32), ("out_zp", C.c_int32), ("a_is_second", C.c_int32),
                ("reserved", C.c_int32 * 4)]


ABI_STRUCTS = {"csinn_quant_info": QuantInfo, "csinn_tensor": Tensor, "csinn_session": Session,
               "csinn_callback": Callback, "csinn_params_base": ParamsBase,
               "csinn_conv2d_params": Conv2dParams, "csinn_fc_params": FcParams,
               "csinn_relu_params": ReluParams, "csinn_model": Model,
               "csinn_softmax_params": SoftmaxParams, "csinn_pool_params": PoolParams,
               "csinn_diso_params": DisoParams}


# ---- library loading -------------------------------------------------------------------------
def lib_path(name):
    return os.path.join(LIB_DIR, name)


_loaded = {}


def _cdll(path, mode=C.RTLD_GLOBAL):
    if path not in _loaded:
        if not os.path.exists(path):
            raise MI355XError("native library missing: %s (run python csi-nn2_amd/build.py)" % path)
        _loaded[path] = C.CDLL(path, mode=mode)
    return _loaded[path]


def load_hip():
    """libshl_mi355x.so with argument types declared."""
    lib = _cdll(lib_path("libshl_mi355x.so"))
    if getattr(lib, "_typed", False):
        return lib
    vp, sz, i32, f32 = C.c_void_p, C.c_size_t, C.c_int32, C.c_float
    sigs = {
        "shl_mi355x_abi_version": (C.c_int, []),
        "shl_mi355x_last_error": (C.c_char_p, []),
        "shl_mi355x_device_count": (C.c_int, []),
        "shl_mi355x_set_device": (C.c_int, [C.c_int]),
        "shl_mi355x_device_info": (C.c_int, [C.c_char_p, sz, C.POINTER(i32), C.POINTER(C.c_int64)]),
        "shl_mi355x_malloc": (vp, [sz]),
        "shl_mi355x_free": (C.c_int, [vp]),
        "shl_mi355x_is_device_ptr": (C.c_int, [vp]),
        "shl_mi355x_upload": (C.c_int, [vp, vp, sz, vp]),
        "shl_mi355x_download": (C.c_int, [vp, vp, sz, vp]),
        "shl_mi355x_copy": (C.c_int, [vp, vp, sz, vp]),
        "shl_mi355x_memset": (C.c_int, [vp, C.c_int, sz, vp]),
        "shl_mi355x_stream_create": (vp, []),
        "shl_mi355x_stream_destroy": (C.c_int, [vp]),
        "shl_mi355x_stream_sync": (C.c_int, [vp]),
        "shl_mi355x_event_create": (vp, []),
        "shl_mi355x_event_destroy": (C.c_int, [vp]),
        "shl_mi355x_event_record": (C.c_int, [vp, vp]),
        "shl_mi355x_event_elapsed_ms": (C.c_int, [vp, vp, C.POINTER(f32)]),
        "shl_mi355x_graph_begin": (C.c_int, [vp]),
        "shl_mi355x_graph_end": (vp, [vp]),
        "shl_mi355x_graph_launch": (C.c_int, [vp, vp]),
        "shl_mi355x_graph_destroy": (C.c_int, [vp]),
        "shl_mi355x_conv_plan_create": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, C.POINTER(vp)]),
        "shl_mi355x_conv_plan_create_wzp": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, C.POINTER(vp)]),
        "shl_mi355x_conv_plan_create_dw_channel": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, f32, f32, vp, C.POINTER(vp)]),
        "shl_mi355x_deconv_plan_create": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, C.POINTER(vp)]),
        "shl_mi355x_deconv_kernel_name": (C.c_char_p, [C.POINTER(ConvDesc)]),
        "shl_mi355x_deconv_geometry": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(i32), i32]),
        "shl_mi355x_debug_trace": (C.c_int, [vp, i32]),
        "shl_mi355x_debug_div_check": (C.c_int, [vp, i32, vp, vp]),
        "shl_mi355x_debug_running_sum": (C.c_int, [vp, i32, i32, vp]),
        "shl_mi355x_debug_f16_round_check": (C.c_int, [vp]),
        "shl_mi355x_debug_mfma_rate": (C.c_int, [i32, i32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "shl_mi355x_comm_available": (C.c_int, []),
        "shl_mi355x_comm_unique_id": (C.c_int, [vp]),
        "shl_mi355x_comm_create": (C.c_int, [vp, i32, i32, C.POINTER(vp)]),
        "shl_mi355x_comm_destroy": (C.c_int, [vp]),
        "shl_mi355x_comm_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "shl_mi355x_device_bus_id": (C.c_int, [C.c_char_p, sz]),
        "shl_mi355x_comm_bcast": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz), i32, i32, vp]),
        "shl_mi355x_conv_plan_destroy": (C.c_int, [vp]),
        "shl_mi355x_conv_plan_algo": (C.c_int, [vp]),
        "shl_mi355x_conv_plan_kernel_name": (C.c_char_p, [vp]),
        "shl_mi355x_conv_plan_bytes": (sz, [vp]),
        "shl_mi355x_conv_plan_const_block": (vp, [vp, C.POINTER(sz)]),
        "shl_mi355x_conv_plan_adopt_block": (C.c_int, [vp, vp]),
        "shl_mi355x_conv_forward": (C.c_int, [vp, vp, vp, i32, vp]),
        "shl_mi355x_pwdw_fusable": (C.c_int, [vp, vp, i32]),
        "shl_mi355x_pwdw_form": (C.c_int, [vp, vp, i32]),
        "shl_mi355x_pwdw_geometry": (C.c_int, [vp, vp, i32, C.POINTER(i32), i32]),
        "shl_mi355x_pwdw_launch_form": (C.c_int, [vp, vp, i32, C.POINTER(i32), i32]),
        "shl_mi355x_pool_conv_fusable": (C.c_int, [vp, i32, i32]),
        "shl_mi355x_pool_conv_forward": (C.c_int, [vp, vp, vp, i32, i32, f32, i32, f32, i32, vp]),
        "shl_mi355x_conv_pool_fusable": (C.c_int, [vp, i32]),
        "shl_mi355x_conv_pool_forward": (C.c_int, [vp, vp, vp, vp, i32, f32, i32, f32, i32, vp]),
        "shl_mi355x_conv_add_fusable": (C.c_int, [vp, i32]),
        "shl_mi355x_conv_add_forward": (C.c_int, [vp, vp, vp, vp, i32, C.POINTER(ResidualDesc), vp]),
        "shl_mi355x_conv_add_kernel_name": (C.c_char_p, [vp, i32]),
        "shl_mi355x_conv_add_by_default": (C.c_int, [vp, i32]),
        "shl_mi355x_conv_add_f16_fusable": (C.c_int, [vp, i32]),
        "shl_mi355x_conv_add_f16_forward": (C.c_int, [vp, vp, vp, vp, i32, C.POINTER(ResidualDesc), vp]),
        "shl_mi355x_conv_add_f16_kernel_name": (C.c_char_p, [vp, i32]),
        "shl_mi355x_conv_add_f16_by_default": (C.c_int, [vp, i32]),
        "shl_mi355x_conv_lut_fusable": (C.c_int, [vp, i32]),
        "shl_mi355x_conv_lut_kernel_name": (C.c_char_p, [vp, i32]),
        "shl_mi355x_conv_lut_by_default": (C.c_int, [vp, i32]),
        "shl_mi355x_conv_lut_forward": (C.c_int, [vp, vp, vp, i32, vp, vp]),
        "shl_mi355x_dwconv_lut_fusable": (C.c_int, [vp, i32]),
        "shl_mi355x_dwconv_lut_kernel_name": (C.c_char_p, [vp, i32]),
        "shl_mi355x_dwconv_lut_by_default": (C.c_int, [vp, i32]),
        "shl_mi355x_dwconv_lut_forward": (C.c_int, [vp, vp, vp, i32, vp, vp]),
        "shl_mi355x_last_igemm_flavour": (C.c_char_p, []),
        "shl_mi355x_conv_plan_set_no_stream_consumer": (C.c_int, [vp, i32]),
        "shl_mi355x_pwdw_forward": (C.c_int, [vp, vp, vp, vp, i32, vp]),
        "shl_mi355x_relu_i8": (C.c_int, [vp, vp, sz, f32, i32, f32, i32, i32, vp]),
        "shl_mi355x_relu_f16": (C.c_int, [vp, vp, sz, i32, vp]),
        "shl_mi355x_add": (C.c_int, [vp, vp, vp, sz, i32, f32, i32, f32, i32, f32, i32, vp]),
        "shl_mi355x_layout_convert": (C.c_int, [vp, vp, C.c_int64, i32, i32, i32, i32, vp]),
        "shl_mi355x_global_avgpool2d": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, f32, i32, f32, i32, vp]),
        "shl_mi355x_softmax": (C.c_int, [vp, vp, i32, C.c_int64, i32, C.c_int64, f32, i32, f32, i32, vp]),
        "shl_mi355x_pool2d": (C.c_int, [vp, vp, C.POINTER(PoolDesc), vp]),
        "shl_mi355x_pool2d_kernel_name": (C.c_char_p, [C.POINTER(PoolDesc)]),
        "shl_mi355x_concat": (C.c_int, [C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(f32), C.POINTER(i32), vp,
                                        C.POINTER(ConcatDesc), vp]),
        "shl_mi355x_concat_kernel_name": (C.c_char_p, [C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(f32), C.POINTER(i32),
                                                       vp, C.POINTER(ConcatDesc)]),
        "shl_mi355x_split": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(f32), C.POINTER(i32),
                                       C.POINTER(SplitDesc), vp]),
        "shl_mi355x_split_kernel_name": (C.c_char_p, [vp, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(f32), C.POINTER(i32),
                                                      C.POINTER(SplitDesc)]),
        "shl_mi355x_shuffle_channel": (C.c_int, [vp, vp, C.POINTER(ShuffleDesc), vp]),
        "shl_mi355x_shuffle_channel_kernel_name": (C.c_char_p, [vp, vp, C.POINTER(ShuffleDesc)]),
        "shl_mi355x_transpose": (C.c_int, [vp, vp, C.POINTER(TransposeDesc), vp]),
        "shl_mi355x_transpose_kernel_name": (C.c_char_p, [vp, vp, C.POINTER(TransposeDesc)]),
        "shl_mi355x_move": (C.c_int, [vp, vp, C.c_int64, C.POINTER(MoveDesc), vp]),
        "shl_mi355x_move_kernel_name": (C.c_char_p, [vp, vp, C.c_int64, C.POINTER(MoveDesc)]),
        "shl_mi355x_pad": (C.c_int, [vp, vp, C.POINTER(PadDesc), vp]),
        "shl_mi355x_pad_kernel_name": (C.c_char_p, [vp, vp, C.POINTER(PadDesc)]),
        "shl_mi355x_pad_element": (C.c_uint32, [C.POINTER(PadDesc)]),
        "shl_mi355x_reduce": (C.c_int, [vp, vp, C.POINTER(ReduceDesc), vp]),
        "shl_mi355x_reduce_kernel_name": (C.c_char_p, [vp, vp, C.POINTER(ReduceDesc)]),
        "shl_mi355x_matmul": (C.c_int, [vp, vp, vp, C.POINTER(MatmulDesc), vp]),
        "shl_mi355x_matmul_kernel_name": (C.c_char_p, [vp, vp, vp, C.POINTER(MatmulDesc)]),
        "shl_mi355x_matmul_is_exact": (C.c_int, [C.POINTER(MatmulDesc)]),
        "shl_mi355x_matmul_bias": (C.c_int, [vp, vp, vp, vp, C.POINTER(MatmulDesc), f32, i32, f32, i32, i32, vp]),
        "shl_mi355x_matmul_bias_kernel_name": (C.c_char_p, [vp, vp, vp, vp, C.POINTER(MatmulDesc)]),
        "shl_mi355x_attention": (C.c_int, [vp, vp, vp, vp, C.POINTER(AttentionDesc), vp]),
        "shl_mi355x_attention_kernel_name": (C.c_char_p, [vp, vp, vp, vp, C.POINTER(AttentionDesc)]),
        "shl_mi355x_attention_by_default": (C.c_int, [vp, vp, vp, vp, C.POINTER(AttentionDesc)]),
        "shl_mi355x_attention_bias": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(AttentionDesc), C.POINTER(AttentionBiasDesc), vp]),
        "shl_mi355x_attention_bias_kernel_name": (C.c_char_p, [vp, vp, vp, vp, vp, C.POINTER(AttentionDesc), C.POINTER(AttentionBiasDesc)]),
        "shl_mi355x_attention_bias_by_default": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(AttentionDesc), C.POINTER(AttentionBiasDesc)]),
        "shl_mi355x_attention_bias_geometry": (C.c_int, [C.POINTER(MulDesc), i32, i32, i32, C.POINTER(AttentionBiasDesc)]),
        "shl_mi355x_attention_layout": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(AttentionDesc), C.POINTER(AttentionBiasDesc),
                                                  C.POINTER(AttentionLayoutDesc), vp]),
        "shl_mi355x_attention_layout_kernel_name": (C.c_char_p, [vp, vp, vp, vp, vp, C.POINTER(AttentionDesc), C.POINTER(AttentionBiasDesc),
                                                                 C.POINTER(AttentionLayoutDesc)]),
        "shl_mi355x_attention_layout_by_default": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(AttentionDesc), C.POINTER(AttentionBiasDesc),
                                                             C.POINTER(AttentionLayoutDesc)]),
        "shl_mi355x_attention_layout_strides": (C.c_int, [C.POINTER(i32), i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), i32,
                                                          C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "shl_mi355x_unary_lut_i8": (C.c_int, [vp, vp, sz, vp, vp]),
        "shl_mi355x_unary_lut_i8_kernel_name": (C.c_char_p, [vp, vp]),
        "shl_mi355x_unary_f16": (C.c_int, [vp, vp, sz, i32, f32, vp]),
        "shl_mi355x_mul": (C.c_int, [vp, vp, vp, C.POINTER(MulDesc), vp]),
        "shl_mi355x_mul_kernel_name": (C.c_char_p, [C.POINTER(MulDesc), vp, vp, vp]),
        "shl_mi355x_add_bcast": (C.c_int, [vp, vp, vp, C.POINTER(MulDesc), vp]),
        "shl_mi355x_add_bcast_kernel_name": (C.c_char_p, [C.POINTER(MulDesc), vp, vp, vp]),
        "shl_mi355x_resize": (C.c_int, [vp, vp, C.POINTER(ResizeDesc), vp]),
        "shl_mi355x_resize_kernel_name": (C.c_char_p, [C.POINTER(ResizeDesc), vp, vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib._typed = True
    lib.EXPORTS = sorted(sigs)
    return lib


_FRONTEND_SIGS = {
    "csinn_alloc_session": (C.POINTER(Session), []),
    "csinn_free_session": (None, [C.POINTER(Session)]),
    "csinn_session_init": (None, [C.POINTER(Session)]),
    "csinn_session_deinit": (None, [C.POINTER(Session)]),
    "csinn_session_setup": (C.c_int, [C.POINTER(Session)]),
    "csinn_session_run": (C.c_int, [C.POINTER(Session)]),
    "csinn_set_input_number": (None, [C.c_int, C.POINTER(Session)]),
    "csinn_set_output_number": (None, [C.c_int, C.POINTER(Session)]),
    "csinn_set_input": (C.c_int, [C.c_int, C.POINTER(Tensor), C.POINTER(Session)]),
    "csinn_set_output": (C.c_int, [C.c_int, C.POINTER(Tensor), C.POINTER(Session)]),
    "csinn_get_output": (C.c_int, [C.c_int, C.POINTER(Tensor), C.POINTER(Session)]),
    "csinn_update_input": (C.c_int, [C.c_int, C.POINTER(Tensor), C.POINTER(Session)]),
    "csinn_update_output": (C.c_int, [C.c_int, C.POINTER(Tensor), C.POINTER(Session)]),
    "csinn_set_tensor_entry": (C.c_int, [C.POINTER(Tensor), C.POINTER(Session)]),
    "csinn_alloc_tensor": (C.POINTER(Tensor), [C.POINTER(Session)]),
    "csinn_free_tensor": (None, [C.POINTER(Tensor)]),
    "csinn_alloc_params": (C.c_void_p, [C.c_int, C.POINTER(Session)]),
    "csinn_free_params": (None, [C.c_void_p]),
    "csinn_tensor_size": (C.c_int, [C.POINTER(Tensor)]),
    "csinn_tensor_byte_size": (C.c_int, [C.POINTER(Tensor)]),
    "shl_register_op_callback": (None, [C.c_int, C.c_void_p]),
    "shl_register_runtime_callback": (None, [C.c_int, C.c_void_p]),
    "shl_mem_alloc": (C.c_void_p, [C.c_int64]),
    "shl_mem_free": (None, [C.c_void_p]),
    "shl_debug_set_level": (None, [C.c_int]),
}
_SISO_OPS = ("csinn_relu", "csinn_relu6", "csinn_global_avgpool2d", "csinn_softmax", "csinn_maxpool2d", "csinn_avgpool2d",
             "csinn_sigmoid", "csinn_hard_sigmoid", "csinn_silu", "csinn_leaky_relu", "csinn_resize", "csinn_shuffle_channel",
             "csinn_transpose", "csinn_reshape", "csinn_flatten", "csinn_pad",
             "csinn_mean", "csinn_sum", "csinn_max", "csinn_min", "csinn_reduce_mean", "csinn_reduce_sum", "csinn_reduce_max",
             "csinn_reduce_min", "csinn_global_maxpool2d")
_CONV_OPS = ["csinn_conv2d", "csinn_conv2d_relu", "csinn_conv2d_relu6", "csinn_depthwise_conv2d",
             "csinn_depthwise_conv2d_relu", "csinn_fullyconnected", "csinn_deconv2d"] + list(_SISO_OPS)


def load_frontend(kind="standalone", local=False, path=None):
    """The csinn_* front-end the backend plugs into: this repo's libcsinn_nn2.so ('standalone'), or --
    with `path` -- any library exporting the CSI-NN2 C API (INTEGRATION.md option A: the user's own
    libshl with the backend loaded next to it).  local=True keeps the library's symbols out of the
    global scope (needed when two front-ends live in one process: the backend library binds its
    front-end symbols to whichever was loaded globally first)."""
    mode = C.RTLD_LOCAL if local else C.RTLD_GLOBAL
    if path is not None:
        lib = _cdll(path, mode)
        kind = "external"
    elif kind == "standalone":
        lib = _cdll(lib_path("libcsinn_nn2.so"), mode)
    else:
        raise ValueError(kind)
    if getattr(lib, "_typed", False):
        return lib
    for name, (res, args) in _FRONTEND_SIGS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    tp = C.POINTER(Tensor)
    for op in _CONV_OPS:
        nargs = 3 if op in _SISO_OPS else 5
        for suffix in ("_init", ""):
            fn = getattr(lib, op + suffix)
            fn.restype = C.c_int
            fn.argtypes = [tp, tp] + ([C.c_void_p] if nargs == 3 else [tp, tp, C.c_void_p])
    for suffix in ("_init", ""):
        for op in ("csinn_add", "csinn_mul", "csinn_matmul"):
            fn = getattr(lib, op + suffix)
            fn.restype, fn.argtypes = C.c_int, [tp, tp, tp, C.c_void_p]
        fn = getattr(lib, "csinn_concat" + suffix)
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(tp), tp, C.c_void_p]
        fn = getattr(lib, "csinn_split" + suffix)
        fn.restype, fn.argtypes = C.c_int, [tp, C.POINTER(tp), C.c_void_p]
    lib._typed = True
    lib.kind = kind
    return lib


def load_backend(frontend):
    """Load the HIP library and the mi355x_opt backend next to `frontend` and register the
    backend in slot CSINN_MI355X.  Returns (hip_lib, opt_lib)."""
    hip = load_hip()
    opt = _cdll(lib_path("libshl_mi355x_opt.so"))
    if not getattr(opt, "_typed", False):
        opt.shl_target_init_mi355x.restype = None
        opt.shl_mi355x_set_stream.argtypes = [C.c_void_p]
        opt.shl_mi355x_get_stream.restype = C.c_void_p
        opt.shl_mi355x_release_params.argtypes = [C.c_void_p]
        opt.shl_mi355x_live_plans.argtypes = [C.POINTER(C.c_int64)]
        opt.shl_mi355x_plans_created.restype = C.c_int64
        opt.shl_target_init_mi355x_slot.argtypes = [C.c_int]
        opt.shl_mi355x_params_const_block.restype = C.c_void_p
        opt.shl_mi355x_params_const_block.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        opt.shl_mi355x_params_kernel_name.restype = C.c_char_p
        opt.shl_mi355x_params_kernel_name.argtypes = [C.c_void_p]
        opt.shl_mi355x_session_is_device_resident.argtypes = [C.POINTER(Session)]
        opt.shl_mi355x_session_fused_pairs.argtypes = [C.POINTER(Session)]
        opt.shl_mi355x_session_fused_pools.argtypes = [C.POINTER(Session)]
        opt.shl_mi355x_registry_get.restype = C.c_void_p
        opt.shl_mi355x_registry_get.argtypes = [C.c_void_p]
        opt.shl_mi355x_session_folded_activations.argtypes = [C.POINTER(Session)]
        opt.shl_mi355x_session_fused_linears.argtypes = [C.POINTER(Session)]
        opt.shl_mi355x_session_fused_attentions.argtypes = [C.POINTER(Session)]
        opt.shl_mi355x_session_fused_attention_biases.argtypes = [C.POINTER(Session)]
        opt.shl_mi355x_session_folded_head_moves.argtypes = [C.POINTER(Session)]
        opt.shl_mi355x_session_fused_residuals.argtypes = [C.POINTER(Session)]
        opt.shl_mi355x_session_fused_activations.argtypes = [C.POINTER(Session)]
        opt.shl_mi355x_session_stream.argtypes = [C.POINTER(Session)]
        opt.shl_mi355x_session_stream.restype = C.c_void_p
        opt.shl_mi355x_session_set_stream.argtypes = [C.POINTER(Session), C.c_void_p]
        opt.shl_mi355x_session_set_stream.restype = None
        opt.shl_mi355x_bcast_const_blocks.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int32,
                                                      C.POINTER(Session)]
        opt.shl_mi355x_params_adopt_blocks.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(Session)]
        table = C.POINTER(C.c_uint8)
        for op in ("sigmoid", "hard_sigmoid", "silu"):
            fn = getattr(opt, "shl_mi355x_%s_table_i8" % op)
            fn.restype, fn.argtypes = None, [C.c_float, C.c_int32, C.c_float, C.c_int32, table]
        opt.shl_mi355x_resize_table_i8.restype = None
        opt.shl_mi355x_resize_table_i8.argtypes = [C.c_float, C.c_int32, C.c_float, C.c_int32, table]
        opt.shl_mi355x_resize_scale.restype = C.c_float
        opt.shl_mi355x_resize_scale.argtypes = [C.c_int32, C.c_int32, C.c_int]
        opt.shl_mi355x_leaky_relu_table_i8.restype = None
        opt.shl_mi355x_leaky_relu_table_i8.argtypes = [C.c_float, C.c_int32, C.c_float, C.c_int32, C.c_float, table]
        opt.shl_mi355x_gate_mul_table_i8.restype = None
        opt.shl_mi355x_gate_mul_table_i8.argtypes = [C.c_int, C.c_float, C.c_int32, C.c_float, C.c_int32, C.c_int, C.c_float, C.c_int32,
                                                     table]
        opt._typed = True
    # the dispatch tables exist after the first csinn_alloc_session (source/nn2/setup.c:77-84)
    s = frontend.csinn_alloc_session()
    frontend.csinn_free_session(s)
    opt.shl_target_init_mi355x()
    return hip, opt


def check(status, hip=None, what="call"):
    if status != 0:
        msg = hip.shl_mi355x_last_error().decode() if hip is not None else ""
        raise MI355XError("%s failed with status %d: %s" % (what, status, msg))


# ---- tensor / params helpers -----------------------------------------------------------------
_NP2CSINN = {np.dtype(np.int8): DTYPE_INT8, np.dtype(np.int32): DTYPE_INT32,
             np.dtype(np.float16): DTYPE_FLOAT16, np.dtype(np.uint16): DTYPE_FLOAT16,
             np.dtype(np.float32): DTYPE_FLOAT32}


class Keep:
    """Keeps Python-owned buffers alive as long as the C structs that point to them."""

    def __init__(self):
        self.items = []

    def add(self, obj):
        self.items.append(obj)
        return obj


def make_tensor(fe, keep, dims, dtype, layout, data=None, scales=(1.0,), zps=(0,), is_const=0,
                name=b"t", sess=None, mtype=MEM_CPU, device_ptr=None):
    """csinn_alloc_tensor + field initialisation.  `data` is a numpy array (host) unless
    `device_ptr` gives an HBM address (mtype becomes DMABUF)."""
    t = fe.csinn_alloc_tensor(sess)
    tc = t.contents
    tc.dtype = dtype
    tc.layout = layout
    tc.dim_count = len(dims)
    for i, d in enumerate(dims):
        tc.dim[i] = int(d)
    tc.is_const = is_const
    tc.name = keep.add(C.c_char_p(name)).value
    n = len(scales)
    q = keep.add((QuantInfo * n)())
    for i in range(n):
        q[i].scale = float(scales[i])
        q[i].zero_point = int(zps[i] if len(zps) > 1 else zps[0])
    # replace the single record csinn_alloc_tensor made (left to the allocator: tiny leak-free
    # because we free it here)
    fe.shl_mem_free(C.cast(tc.qinfo, C.c_void_p))
    tc.qinfo = C.cast(q, C.POINTER(QuantInfo))
    tc.quant_channel = n
    if device_ptr is not None:
        tc.data = device_ptr
        tc.mtype = MEM_DMABUF
    elif data is not None:
        arr = keep.add(np.ascontiguousarray(data))
        tc.data = arr.ctypes.data
        tc.mtype = mtype
    keep.add(t)
    return t


def free_tensor(fe, t):
    t.contents.qinfo = None  # python-owned
    fe.csinn_free_tensor(t)


def conv_params(fe, keep, api, layout, stride=(1, 1), pad=(0, 0, 0, 0), dilation=(1, 1), group=1,
                fuse_zp2bias=0, sess=None, name=b"conv"):
    """pad = (top, left, down, right)"""
    p = fe.csinn_alloc_params(C.sizeof(Conv2dParams), sess)
    pc = C.cast(p, C.POINTER(Conv2dParams)).contents
    pc.base.api = api
    pc.base.layout = layout
    pc.base.name = keep.add(C.c_char_p(name)).value
    if sess is not None:
        pc.base.sess = sess
    pc.group = group
    pc.stride_height, pc.stride_width = stride
    pc.pad_top, pc.pad_left, pc.pad_down, pc.pad_right = pad
    pc.dilation_height, pc.dilation_width = dilation
    pc.conv_extra.fuse_zp2bias = fuse_zp2bias
    return p


def deconv_params(fe, keep, api, layout, stride=(2, 2), pad=(0, 0, 0, 0), out_pad=(0, 0), group=1, dilation=(1, 1), sess=None,
                  name=b"deconv"):
    """params block of csinn_deconv2d (a csinn_conv2d_params); pad = (top, left, down, right), out_pad = (height, width):
    the output size is the output tensor's, which the caller makes out_pad larger"""
    p = conv_params(fe, keep, api, layout, stride, pad, dilation, group, 0, sess, name)
    pc = C.cast(p, C.POINTER(Conv2dParams)).contents
    pc.out_pad_height, pc.out_pad_width = out_pad
    return p


def pool_params(fe, keep, api, layout, kernel=(2, 2), stride=(2, 2), pad=(0, 0, 0, 0), ceil_mode=0,
                count_include_pad=False, sess=None, name=b"pool"):
    """params block of csinn_maxpool2d / csinn_avgpool2d; pad = (top, left, down, right)"""
    p = fe.csinn_alloc_params(C.sizeof(PoolParams), sess)
    pc = C.cast(p, C.POINTER(PoolParams)).contents
    pc.base.api = api
    pc.base.layout = layout
    pc.base.name = keep.add(C.c_char_p(name)).value
    if sess is not None:
        pc.base.sess = sess
    pc.filter_height, pc.filter_width = kernel
    pc.stride_height, pc.stride_width = stride
    pc.pad_top, pc.pad_left, pc.pad_down, pc.pad_right = pad
    pc.ceil_mode = ceil_mode
    pc.count_include_pad = bool(count_include_pad)
    return p


def concat_params(fe, keep, api, layout, n, axis, sess=None, name=b"concat"):
    """params block of csinn_concat: n inputs along `axis` (-1: the last axis)"""
    p = fe.csinn_alloc_params(C.sizeof(ConcatParams), sess)
    pc = C.cast(p, C.POINTER(ConcatParams)).contents
    pc.base.api = api
    pc.base.layout = layout
    pc.base.name = keep.add(C.c_char_p(name)).value
    if sess is not None:
        pc.base.sess = sess
    pc.inputs_count = n
    pc.axis = axis
    return p


def split_params(fe, keep, api, layout, n, axis, split_index=None, sess=None, name=b"split"):
    """params block of csinn_split: n outputs along `axis` (< 0: from the back); split_index: the n - 1 boundaries, or None
    for chunks of ceil(dim / n)"""
    p = fe.csinn_alloc_params(C.sizeof(SplitParams), sess)
    pc = C.cast(p, C.POINTER(SplitParams)).contents
    pc.base.api = api
    pc.base.layout = layout
    pc.base.name = keep.add(C.c_char_p(name)).value
    if sess is not None:
        pc.base.sess = sess
    pc.output_num = n
    pc.axis = axis
    if split_index is not None:
        idx = keep.add((C.c_int32 * max(len(split_index), 1))(*split_index))
        pc.split_index = C.cast(idx, C.POINTER(C.c_int32))
    return p


def shuffle_channel_params(fe, keep, api, layout, group, sess=None, name=b"shuffle"):
    """params block of csinn_shuffle_channel"""
    p = fe.csinn_alloc_params(C.sizeof(ShuffleChannelParams), sess)
    pc = C.cast(p, C.POINTER(ShuffleChannelParams)).contents
    pc.base.api = api
    pc.base.layout = layout
    pc.base.name = keep.add(C.c_char_p(name)).value
    if sess is not None:
        pc.base.sess = sess
    pc.group = group
    return p


def _move_params(fe, keep, struct, api, layout, sess, name):
    p = fe.csinn_alloc_params(C.sizeof(struct), sess)
    pc = C.cast(p, C.POINTER(struct)).contents
    pc.base.api = api
    pc.base.layout = layout
    pc.base.name = keep.add(C.c_char_p(name)).value
    if sess is not None:
        pc.base.sess = sess
    return p, pc


def transpose_params(fe, keep, api, layout, permute, sess=None, name=b"transpose", permute_num=None):
    """params block of csinn_transpose: output dim k is input dim permute[k]"""
    p, pc = _move_params(fe, keep, TransposeParams, api, layout, sess, name)
    arr = keep.add((C.c_int32 * max(len(permute), 1))(*permute))
    pc.permute = C.cast(arr, C.POINTER(C.c_int32))
    pc.permute_num = len(permute) if permute_num is None else permute_num
    return p


def reshape_params(fe, keep, api, layout, shape, sess=None, name=b"reshape"):
    """params block of csinn_reshape: `shape` is what the output tensor's dims were derived from"""
    p, pc = _move_params(fe, keep, ReshapeParams, api, layout, sess, name)
    arr = keep.add((C.c_int32 * max(len(shape), 1))(*shape))
    pc.shape = C.cast(arr, C.POINTER(C.c_int32))
    pc.shape_num = len(shape)
    return p


def flatten_params(fe, keep, api, layout, axis=1, sess=None, name=b"flatten"):
    """params block of csinn_flatten"""
    p, pc = _move_params(fe, keep, FlattenParams, api, layout, sess, name)
    pc.axis = axis
    return p


def pad_params(fe, keep, api, layout, before, after, value=0.0, mode=PAD_CONSTANT, sess=None, name=b"pad", pad_num=None):
    """params block of csinn_pad: pads per dim in memory order"""
    p, pc = _move_params(fe, keep, PadParams, api, layout, sess, name)
    b = keep.add((C.c_int32 * max(len(before), 1))(*before))
    a = keep.add((C.c_int32 * max(len(after), 1))(*after))
    pc.pad_before, pc.pad_after = C.cast(b, C.POINTER(C.c_int32)), C.cast(a, C.POINTER(C.c_int32))
    pc.pad_num = len(before) if pad_num is None else pad_num
    pc.pad_value = value
    pc.pad_mode = mode
    return p


def reduce_groups(shape, axes):
    """(out_extents, out_strides, inner_extents, inner_strides) of a reduction of a dense tensor of `shape` over `axes`, in
    the tensor's dim order: what struct csinn_reduce_params and shl_mi355x_reduce_desc take (strides in elements)"""
    rank = len(shape)
    axes = sorted(a % rank for a in axes)
    assert len(set(axes)) == len(axes)
    stride = [1] * rank
    for k in range(rank - 2, -1, -1):
        stride[k] = stride[k + 1] * shape[k + 1]
    keep_dims = [k for k in range(rank) if k not in axes]
    return ([shape[k] for k in keep_dims], [stride[k] for k in keep_dims], [shape[k] for k in axes], [stride[k] for k in axes])


def reduce_params(fe, keep, api, layout, groups=None, axis=None, sess=None, name=b"reduce", axis_count=None):
    """params block of csinn_mean / _sum / _max / _min (groups: what reduce_groups returns, or four lists) and of
    csinn_reduce_mean / _sum / _max / _min (axis: a list, [-1] for the whole tensor)"""
    p, pc = _move_params(fe, keep, ReduceParams, api, layout, sess, name)
    ip = C.POINTER(C.c_int32)
    if groups is not None:
        oe, os_, ie, is_ = [keep.add((C.c_int32 * max(len(g), 1))(*g)) for g in groups]
        pc.out_extents, pc.out_strides = C.cast(oe, ip), C.cast(os_, ip)
        pc.inner_extents, pc.inner_strides = C.cast(ie, ip), C.cast(is_, ip)
        pc.n, pc.m = len(groups[0]), len(groups[2])
    axis = list(axis) if axis is not None else []
    arr = keep.add((C.c_int32 * max(len(axis), 1))(*axis))
    pc.axis = C.cast(arr, ip)
    pc.axis_count = len(axis) if axis_count is None else axis_count
    pc.keepdims = True
    return p


def matmul_params(fe, keep, api, layout, trans_a=False, trans_b=False, sess=None, name=b"matmul"):
    """params block of csinn_matmul"""
    p, pc = _move_params(fe, keep, MatmulParams, api, layout, sess, name)
    pc.trans_a, pc.trans_b = bool(trans_a), bool(trans_b)
    return p


def matmul_desc(dtype, a_shape, b_shape, trans_a=False, trans_b=False, a_q=(1.0, 0), b_q=(1.0, 0), out_q=(1.0, 0)):
    """shl_mi355x_matmul_desc of csinn_matmul on two dense tensors: the leading dims of each operand are one batch count,
    the transposes become strides, the reference's "dense" broadcast (one mat1 for every batch of mat0, no transposes) a batch
    stride of 0.  ValueError for the shapes the reference refuses.  dtype: SHL_I8 / SHL_F16; the records are (scale, zp)"""
    a_shape, b_shape = [int(v) for v in a_shape], [int(v) for v in b_shape]
    if len(a_shape) < 2 or len(b_shape) < 2:
        raise ValueError("matmul needs tensors of two or more dims")
    prod = lambda dims: int(np.prod(dims, dtype=np.int64))
    ba, bb = prod(a_shape[:-2]), prod(b_shape[:-2])
    m, k = (a_shape[-1], a_shape[-2]) if trans_a else (a_shape[-2], a_shape[-1])
    n, k1 = (b_shape[-2], b_shape[-1]) if trans_b else (b_shape[-1], b_shape[-2])
    if k1 != k:
        raise ValueError("the operands disagree on K: %d and %d" % (k, k1))
    if not (ba == bb or (ba > 1 and bb == 1 and not trans_a and not trans_b)):
        raise ValueError("batches %d and %d: a broadcast the reference refuses" % (ba, bb))
    d = MatmulDesc()
    d.dtype, d.batches, d.m, d.n, d.k = dtype, ba, m, n, k
    d.a_batch_stride, d.a_row_stride, d.a_k_stride = m * k, (1 if trans_a else k), (m if trans_a else 1)
    d.b_batch_stride, d.b_col_stride, d.b_k_stride = (0 if bb == 1 and ba > 1 else k * n), (k if trans_b else 1), (1 if trans_b else n)
    d.a_elems, d.b_elems, d.out_elems = prod(a_shape), prod(b_shape), ba * m * n
    (d.a_scale, d.a_zp), (d.b_scale, d.b_zp), (d.out_scale, d.out_zp) = a_q, b_q, out_q
    return d


def matmul(hip, a_dev, b_dev, out_dev, desc, stream=None):
    """enqueue out = a x b (device pointers) on `stream`; raises MI355XError on a refusal.  Returns the form that ran"""
    name = hip.shl_mi355x_matmul_kernel_name(a_dev, b_dev, out_dev, C.byref(desc)).decode()
    check(hip.shl_mi355x_matmul(a_dev, b_dev, out_dev, C.byref(desc), stream), hip, "shl_mi355x_matmul")
    return name


def tensor_array(keep, tensors):
    """struct csinn_tensor *[]: what csinn_concat takes as its inputs and csinn_split as its outputs"""
    return keep.add((C.POINTER(Tensor) * len(tensors))(*tensors))


def resize_params(fe, keep, api, layout, mode=RESIZE_NEAREST_NEIGHBOR, align_corners=False, sess=None, name=b"resize"):
    """params block of csinn_resize: the output size is the output tensor's"""
    p = fe.csinn_alloc_params(C.sizeof(ResizeParams), sess)
    pc = C.cast(p, C.POINTER(ResizeParams)).contents
    pc.base.api = api
    pc.base.layout = layout
    pc.base.name = keep.add(C.c_char_p(name)).value
    if sess is not None:
        pc.base.sess = sess
    pc.resize_mode = mode
    pc.align_corners = bool(align_corners)
    return p


def fc_params(fe, keep, api, units, fuse_zp2bias=0, sess=None, name=b"fc"):
    p = fe.csinn_alloc_params(C.sizeof(FcParams), sess)
    pc = C.cast(p, C.POINTER(FcParams)).contents
    pc.base.api = api
    pc.base.layout = LAYOUT_NC
    pc.base.name = keep.add(C.c_char_p(name)).value
    if sess is not None:
        pc.base.sess = sess
    pc.units = units
    pc.fc_extra.fuse_zp2bias = fuse_zp2bias
    return p


def siso_params(fe, keep, api, kind, layout=LAYOUT_NHWC, axis=1, sess=None, name=b"siso", n=0.0):
    """params block of a single-input single-output op: kind in relu | relu6 | pool | softmax | sigmoid | hard_sigmoid |
    silu | leaky_relu (n: its slope), or of add / mul"""
    ctype = {"relu": ReluParams, "relu6": ReluParams, "pool": PoolParams, "softmax": SoftmaxParams,
             "add": DisoParams, "mul": DisoParams, "sigmoid": SigmoidParams, "hard_sigmoid": SigmoidParams,
             "silu": SigmoidParams, "leaky_relu": ReluParams}[kind]
    p = fe.csinn_alloc_params(C.sizeof(ctype), sess)
    pc = C.cast(p, C.POINTER(ctype)).contents
    pc.base.api = api
    pc.base.layout = layout
    pc.base.name = keep.add(C.c_char_p(name)).value
    if sess is not None:
        pc.base.sess = sess
    if kind == "softmax":
        pc.axis = axis
    if kind == "relu6":
        pc.n = 6.0
    if kind == "leaky_relu":
        pc.n = n
    return p


def layer_session(fe, api, keep):
    """A layer-mode session (shl_get_p0_cb dereferences base->sess, so one is mandatory)."""
    s = fe.csinn_alloc_session()
    s.contents.base_api = api
    s.contents.base_run_mode = RM_LAYER
    s.contents.debug_level = 0
    keep.add(s)
    return s

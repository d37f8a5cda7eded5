/*
 * shl_mi355x.h -- C-ABI of libshl_mi355x.so, the HIP/gfx950 compute library
 * behind the source/mi355x_opt backend.
 *
 * Plain C: pointers, sizes and PODs only -- no HIP, C++ or torch types cross
 * this boundary.  The host backend (C, compiled by gcc) and any foreign-language
 * binding (ctypes, cgo, JNI ...) talk to the GPU exclusively through these
 * entry points.  Each compute entry point names the reference function it
 * replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - return value: 0 on success, a negative SHL_MI355X_E* code on failure;
 *     shl_mi355x_last_error() returns a human-readable message for the calling
 *     thread's last failure.  There is NO CPU fallback anywhere in this library:
 *     without a usable gfx950 device every compute call fails with
 *     SHL_MI355X_ENODEV.
 *   - `stream` is an opaque hipStream_t (NULL = the default stream).  All compute
 *     entry points only enqueue work; they never synchronise.
 *   - pointers named *_dev must be device-accessible (hipMalloc / torch CUDA
 *     tensor storage); pointers named *_host are ordinary host memory.
 */
#ifndef SHL_MI355X_H_
#define SHL_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHL_MI355X_ABI_VERSION 1

enum shl_mi355x_status {
    SHL_MI355X_OK = 0,
    SHL_MI355X_ENODEV = -1,   /* no gfx950 device / HIP runtime unusable */
    SHL_MI355X_EINVAL = -2,   /* malformed descriptor or NULL pointer */
    SHL_MI355X_ENOTSUP = -3,  /* descriptor valid but no kernel covers it */
    SHL_MI355X_EHIP = -4,     /* a HIP runtime call failed (see last_error) */
    SHL_MI355X_ENOMEM = -5
};

enum shl_mi355x_layout {
    SHL_MI355X_NHWC = 0, /* activations [N,H,W,C]; conv kernel OHWI; dw kernel 1HWO */
    SHL_MI355X_NCHW = 1  /* activations [N,C,H,W]; conv kernel OIHW; dw kernel O1HW */
};

enum shl_mi355x_dtype {
    SHL_MI355X_I8 = 0,  /* int8 activations/weights, int32 bias, int32 accumulation */
    SHL_MI355X_F16 = 1  /* IEEE binary16 activations/weights/bias, fp32 accumulation */
};

enum shl_mi355x_act {
    SHL_MI355X_ACT_NONE = 0,
    SHL_MI355X_ACT_RELU = 1, /* reference/convolution_relu.c:34-71 semantics */
    SHL_MI355X_ACT_RELU6 = 2 /* reference/convolution_relu6.c:21-43 semantics */
};

enum shl_mi355x_algo {
    SHL_MI355X_ALGO_AUTO = 0,
    SHL_MI355X_ALGO_DIRECT = 1, /* one thread per output, any shape (VALU) */
    SHL_MI355X_ALGO_IGEMM = 2,  /* LDS-staged implicit GEMM on MFMA */
    SHL_MI355X_ALGO_DW = 3,     /* bandwidth-tuned depthwise kernel */
    SHL_MI355X_ALGO_GEMV = 4,   /* fullyconnected, small batch (reserved) */
    SHL_MI355X_ALGO_STEM = 5,   /* 3x3 conv with 3 input channels (image stem), v_dot4 */
    SHL_MI355X_ALGO_DW_CHANNEL = 6, /* CSINN_OP_DEPTHWISE_CONV2D_CHANNEL: int64 accumulation (plan_create_dw_channel) */
    /* grouped convolution (1 < group, not depthwise) with shl_ref_group_conv2d_quant's slice semantics
     * (source/reference/convolution.c:271-354, 476-508), ONE launch per layer:
     *   NCHW  image j, group i reads input planes (j G + i) C/G .. and writes output planes (j G + i) Cout/G .. (the
     *         usual grouped convolution);
     *   NHWC  the buffers are G consecutive tensors [N, H, W, C/G] -> [N, Ho, Wo, Cout/G] (NOT channel-interleaved
     *         groups): restated literally, identical results are the contract.
     * Never chosen by ALGO_AUTO: a descriptor with group > 1 alone cannot say which of the two the caller means */
    SHL_MI355X_ALGO_GROUP = 7,
    /* transposed convolution (shl_mi355x_deconv_plan_create; never chosen for a convolution descriptor) */
    SHL_MI355X_ALGO_DECONV_GATHER = 8, /* one output element per thread, any shape (VALU) */
    SHL_MI355X_ALGO_DECONV_PHASE = 9   /* one ordinary small convolution per output phase on MFMA, no LDS */
};

/* ------------------------------------------------------------------------------------
 * Problem descriptor shared by conv2d, depthwise_conv2d and fullyconnected
 * (fullyconnected == 1x1 convolution over a [batch,1,1,in_nodes] NHWC tensor).
 * Mirrors the fields the reference reads from csinn_tensor.dim[] and
 * struct csinn_conv2d_params (csinn_data_structure.h:591-610).
 * ------------------------------------------------------------------------------------ */
struct shl_mi355x_conv_desc {
    int32_t layout; /* enum shl_mi355x_layout */
    int32_t dtype;  /* enum shl_mi355x_dtype */
    int32_t act;    /* enum shl_mi355x_act */
    int32_t algo;   /* enum shl_mi355x_algo; AUTO lets the library choose */
    int32_t batch, in_h, in_w, in_c;
    int32_t out_h, out_w, out_c;
    int32_t kernel_h, kernel_w;
    int32_t stride_h, stride_w;
    int32_t pad_top, pad_left;
    int32_t dilation_h, dilation_w;
    int32_t group;       /* 1: conv2d; == in_c: depthwise (out_c = in_c * multiplier) */
    int32_t in_zp;       /* int8 only: input zero point */
    int32_t out_zp;      /* int8 only: output zero point */
    float out_scale;     /* int8: output scale; f16: output qinfo scale (1.0 = none) */
    int32_t reserved[4]; /* must be zero */
};

/* ------------------------------------------------------------------------------------
 * A prepared convolution: packed weights + per-output-channel epilogue tables in HBM.
 * Built once per layer (the backend's `init` callback), reused by every `exec`.
 * Opaque to the caller.
 * ------------------------------------------------------------------------------------ */
typedef struct shl_mi355x_conv_plan shl_mi355x_conv_plan;

/* ---- library / device ------------------------------------------------------------- */
int shl_mi355x_abi_version(void);
const char *shl_mi355x_last_error(void);
/* number of visible gfx950 devices (0 when the HIP runtime finds none) */
int shl_mi355x_device_count(void);
int shl_mi355x_set_device(int ordinal);
/* "gfx950:sramecc+:xnack-", compute-unit count, HBM bytes of the current device */
int shl_mi355x_device_info(char *arch, size_t arch_len, int32_t *cu_count, int64_t *hbm_bytes);
/* PCI bus id "dddd:bb:dd.f" of the current device (hipDeviceGetPCIBusId): what tells the ranks of a multi-GPU job
 * that they really sit on distinct devices before they enter a collective */
int shl_mi355x_device_bus_id(char *buf, size_t len);

/* ---- memory and streams (stand in for hipMalloc/hipMemcpyAsync/hipStream*) --------- */
void *shl_mi355x_malloc(size_t bytes);
int shl_mi355x_free(void *ptr_dev);
/* 1 if `ptr` is device memory of the current process, 0 if host/unknown */
int shl_mi355x_is_device_ptr(const void *ptr);
int shl_mi355x_upload(void *dst_dev, const void *src_host, size_t bytes, void *stream);
int shl_mi355x_download(void *dst_host, const void *src_dev, size_t bytes, void *stream);
int shl_mi355x_copy(void *dst_dev, const void *src_dev, size_t bytes, void *stream);
int shl_mi355x_memset(void *dst_dev, int byte_value, size_t bytes, void *stream);
void *shl_mi355x_stream_create(void);
int shl_mi355x_stream_destroy(void *stream);
int shl_mi355x_stream_sync(void *stream);

/* ---- timing on a stream (HIP events) ------------------------------------------------ */
void *shl_mi355x_event_create(void);
int shl_mi355x_event_destroy(void *event);
int shl_mi355x_event_record(void *event, void *stream);
/* waits for `stop`, then returns milliseconds between the two records */
int shl_mi355x_event_elapsed_ms(void *start, void *stop, float *ms);

/* ---- hipGraph capture of a launch sequence (launch-bound layer chains) --------------- */
int shl_mi355x_graph_begin(void *stream);
/* ends capture on `stream` and instantiates; returns an opaque executable graph or NULL */
void *shl_mi355x_graph_end(void *stream);
int shl_mi355x_graph_launch(void *graph_exec, void *stream);
int shl_mi355x_graph_destroy(void *graph_exec);

/* ---- conv2d / depthwise_conv2d / fullyconnected -------------------------------------- */

/*
 * Build the device-resident plan for one layer.
 *
 *   kernel_host   weights exactly as the csinn kernel tensor holds them
 *                 (OHWI / 1HWO for NHWC, OIHW / O1HW for NCHW; [units,in] for FC),
 *                 int8 or binary16.
 *   mult_host     int8: out_c floats, s_in * s_kernel[oc]   (reference: the product of
 *                 int8_to_float_base scales, source/nn2/utils.c:499-502)
 *                 f16 : NULL
 *   bias_host     out_c floats: the bias already converted to fp32 exactly as the
 *                 reference does ((float)b * s_bias[oc], source/nn2/utils.c:509-512, plus
 *                 the fuse_zp2bias correction of reference/convolution.c:375-395), or NULL
 *                 for "no bias"
 *
 * Replaces the per-call work of shl_ref_conv_callback_base
 * (source/reference/utils.c:639-655: dequantise kernel + bias on every call) and plays the
 * role of the optimised backends' init-time weight reorder + zero-point fold
 * (source/thead_rvv/int8/convolution.c:161-190).
 */
int shl_mi355x_conv_plan_create(const struct shl_mi355x_conv_desc *desc,
                                const void *kernel_host, const float *mult_host,
                                const float *bias_host, void *stream,
                                shl_mi355x_conv_plan **plan_out);
/* The same with ASYMMETRIC int8 weights: kernel_zp[oc] = zero point of output channel oc's kernel record (out_c
 * entries; a per-tensor record repeated).  The reference dequantises weights as ((float)w - zero_point) * scale
 * (int8_to_float_base, source/nn2/utils.c:499-502, through nchw/nhwc_int8_to_float :920-945), so shl_ref_conv2d_quant
 * (source/reference/convolution.c:370-400) accepts CSINN_QUANT_INT8_ASYM kernels.  With any non-zero entry the plan runs
 * on the one-output-per-thread kernels (ALGO_DIRECT / ALGO_GROUP: sum (q - zp_in)(w - zp_k) over in-image taps); with
 * all zeros (or NULL) it is shl_mi355x_conv_plan_create. */
int shl_mi355x_conv_plan_create_wzp(const struct shl_mi355x_conv_desc *desc, const void *kernel_host,
                                    const float *mult_host, const float *bias_host, const int32_t *kernel_zp,
                                    void *stream, shl_mi355x_conv_plan **plan_out);
/* ---- multi-GPU: the one collective of the path ---------------------------------
 * The batch shards over the GPUs of a node with no collective on the data path; the only exchange is the
 * one-time broadcast of the plans' constant blocks from the rank that packed the weights.  RCCL
 * (ncclBroadcast over xGMI) behind the C-ABI; librccl.so is opened on first use, so single-GPU
 * processes never load it.
 *   comm_available   1 when librccl.so and its entry points were found
 *   comm_unique_id   rank `root`: 128 opaque bytes (ncclUniqueId) to hand to every peer out of band
 *   comm_create      collective over all ranks with the same 128 bytes -> opaque communicator
 *   comm_bcast       blocks_dev[i] (bytes[i] bytes, same sizes on every rank) from `root` to all, enqueued on
 *                    `stream` as ONE ncclGroup (a few large messages, not one collective per layer)
 */
int shl_mi355x_comm_available(void);
int shl_mi355x_comm_unique_id(void *id128);
int shl_mi355x_comm_create(const void *id128, int32_t rank, int32_t world, void **comm_out);
int shl_mi355x_comm_destroy(void *comm);
/* what RCCL itself says about a communicator: ncclCommCount / ncclCommUserRank / ncclCommCuDevice */
int shl_mi355x_comm_info(void *comm, int32_t *nranks, int32_t *rank, int32_t *device);
int shl_mi355x_comm_bcast(void *comm, void *const *blocks_dev, const size_t *bytes, int32_t count, int32_t root,
                          void *stream);

/* Diagnostics: with SHL_MI355X_DEBUG bit 128 set, workgroup 0 of the ping-pong implicit-GEMM kernel
 * (conv_igemm_pp.hip) records s_memtime at its phase boundaries; copies up to 1024 stamps to `host`
 * (slots 0..511 wave 0, 512..1023 wave 4).  tools/pp_trace.py prints them. */
int shl_mi355x_debug_trace(uint64_t *host, int32_t count);

/* Self check of the int8 epilogue's division by the output scale (csrc/common.h div_by_scale: multiply + two fma
 * corrections, bit-identical to the IEEE division of shl_ref's requantisation, source/nn2/utils.c:550-560 via
 * `x / scale`): for each of the `n` divisors every significand of the dividend is compared with the hardware's
 * correctly rounded division.  *mismatches = number of differing quotients, first_pair[0..1] = one (f, s). */
int shl_mi355x_debug_div_check(const float *divisors_host, int32_t n, uint64_t *mismatches, float *first_pair);
/* Tests only.  The float running sum of softmax, acc = (float)((double)acc + term[j]) for j = 0 .. count - 1 from
 * acc = 0, on crafted terms (csrc/pool_softmax.hip): the wave-parallel scan, or with literal != 0 the one-lane loop.
 * 1 <= count <= 8192; the terms are what softmax produces: non-negative, +inf or NaN.  *sum_host = acc. */
int shl_mi355x_debug_running_sum(const double *terms_host, int32_t count, int32_t literal, float *sum_host);
/* Tests only.  The binary16 epilogues round with one hardware conversion + a fix-up instead of the ~25 integer
 * operations of float32_to_float16_base (source/nn2/utils.c:576-620): every one of the 2^32 float32 bit patterns is
 * pushed through both the one-value and the packed two-value shortcut (csrc/common.h) and compared with the literal
 * restatement.  out3[0] = mismatches, out3[1] = patterns the packed shortcut admits, out3[2] = one offending pattern. */
int shl_mi355x_debug_f16_round_check(uint64_t *out3);
/* Measured issue rate of a matrix instruction on every CU (four accumulator chains per wave, 1 or 2 waves per SIMD):
 * form 0 = v_mfma_i32_32x32x32_i8 (what the int8 kernels issue), 1 = v_mfma_i32_32x32x16_i8 (the form BASELINE.json's
 * north_star names; half the K at the same pass count), 2 = v_mfma_f32_32x32x16_f16.  *tops = TOP/s (TFLOP/s) of the
 * whole device, *ns_per_mfma = nanoseconds per instruction and SIMD.  bench.py prints both int8 forms. */
int shl_mi355x_debug_mfma_rate(int32_t form, int32_t waves_per_simd, double *tops, double *ns_per_mfma);

/*
 * Plan for CSINN_OP_DEPTHWISE_CONV2D_CHANNEL{,_RELU,_RELU6} (int8, NCHW, kernel O1HW): the reference's one
 * integer-accumulating convolution, shl_ref_depthwise_conv2d_channel_nchw_i8
 * (source/reference/convolution_channel.c:172-255) + shl_ref_quantize_channel_i8
 * (source/reference/utils.c:175-180, 205-210).
 *   kernel_scale / kernel_zp   out_c per-channel records of the kernel tensor
 *   bias_i32                   RAW int32 bias (added to the 64-bit accumulator unscaled), or NULL
 *   in_scale                   the input record's float scale
 *   out_scale_ms               the output scale the reference derives from the record's multiplier /
 *                              shift (shl_ref_get_scale, utils.c:132-137); desc->out_scale stays the
 *                              record's float scale, which the fused relu / relu6 step uses
 * The plan runs through shl_mi355x_conv_forward / _destroy like any other.
 */
int shl_mi355x_conv_plan_create_dw_channel(const struct shl_mi355x_conv_desc *desc, const void *kernel_host,
                                           const float *kernel_scale, const int32_t *kernel_zp,
                                           const int32_t *bias_i32, float in_scale, float out_scale_ms,
                                           void *stream, shl_mi355x_conv_plan **plan_out);

/*
 * Plan for a transposed convolution: CSINN_OP_DECONV2D / CSINN_OP_DEPTHWISE_DECONV2D, shl_ref_deconv2d_quant /
 * shl_ref_depthwise_deconv2d_quant (source/reference/deconvolution.c:21-175, 334-369).
 *   out[n, iy*stride_h - pad_top + ky, ix*stride_w - pad_left + kx, oc] += in[n, iy, ix, ic] * w[oc, ky, kx, ic]
 * with the epilogue of shl_mi355x_conv_forward (int8: exact int32 sum of (q - in_zp) * w, then mult / bias / requantise /
 * relu; binary16: fp32 sum in the reference's order, its own rounding).  desc->in_* and out_* are the deconvolution's own
 * input and output; the output extents are free (output_padding is a larger output, positions that no tap reaches hold
 * the bias alone) up to the typo guard
 *       out_h <= (in_h - 1) * stride_h + kernel_h + stride_h      (and the same in w)
 * -- no padding lets the operator reach further than (in - 1) * stride + kernel, one more stride is room for any
 * output_padding; larger is SHL_MI355X_EINVAL, as are non-positive extents.  group is 1 or in_c (depthwise: out_c == in_c),
 * dilation must be 1, desc->algo is ignored: anything else is SHL_MI355X_ENOTSUP.  Every refusal happens before the first
 * device call.
 *   kernel_host   group 1: [O, Kh, Kw, I] (NHWC) / [I, O, Kh, Kw] (NCHW); depthwise: [1, Kh, Kw, C] / [C, 1, Kh, Kw]
 *   mult_host     int8: out_c floats s_in * s_kernel[oc];  bias_host: out_c floats or NULL -- as for shl_mi355x_conv_plan_create
 * Two kernel forms (csrc/deconv.hip): "deconv_phase_*" (MFMA; NHWC, group 1, in_c * element size a multiple
 * of 32, int8 tables in the range of the fast epilogue) and "deconv_gather_*" (everything).  SHL_MI355X_DECONV_FORM=gather
 * | phase forces one; a forced phase form on a layer it does not take is SHL_MI355X_ENOTSUP.
 * The plan runs through shl_mi355x_conv_forward / _destroy / _algo / _kernel_name / _bytes / _const_block / _adopt_block
 * like any other and is independent of the batch; the pool and pair fusion queries answer 0 for it.
 */
int shl_mi355x_deconv_plan_create(const struct shl_mi355x_conv_desc *desc, const void *kernel_host, const float *mult_host,
                                  const float *bias_host, void *stream, shl_mi355x_conv_plan **plan_out);
/* the kernel the rules (and the switch) choose for the descriptor, without a device: "" when the descriptor is refused.
 * (A plan whose int8 tables lie outside 2^-40 .. 2^40 runs the gather form whatever this says.) */
const char *shl_mi355x_deconv_kernel_name(const struct shl_mi355x_conv_desc *desc);
/* The phase decomposition of the descriptor, read-only and without a device, so that it can be checked on the CPU:
 *   out[0] form (0 gather, 1 phase), out[1] P = stride_h * stride_w phases, then per phase (py major)
 *   py, px, taps in y, taps in x, phase rows, phase columns       -- phase (py, px) owns the outputs with
 *       (oy + pad_top) % stride_h == py and (ox + pad_left) % stride_w == px, its taps are ky = py + j * stride_h < Kh
 *   then the tiles of 32 pixels x 32 channels over all phases for desc->batch images, and the workgroups of the phase
 *   form's launch (four tiles each, every phase given the largest phase's share).  count >= 4 + 6 * P. */
int shl_mi355x_deconv_geometry(const struct shl_mi355x_conv_desc *desc, int32_t *out, int32_t count);

int shl_mi355x_conv_plan_destroy(shl_mi355x_conv_plan *plan);
/* the algorithm the plan resolved to (enum shl_mi355x_algo) and its kernel name */
int shl_mi355x_conv_plan_algo(const shl_mi355x_conv_plan *plan);
const char *shl_mi355x_conv_plan_kernel_name(const shl_mi355x_conv_plan *plan);
/* Which instantiation of the wave / regs / tile implicit-GEMM kernels the calling thread launched last, fused or not: the
 * family, its flavour (the wave kernel's K split; the tile kernel's size, ring depth and tap addressing), the requantisation
 * code and the post-op, e.g. "wave/ks4/epi4+add", "regs/epi0", "tile/128x128/pipe8/utap/epi1+lut", "tile/256x64/pipe0/anytap/epi3";
 * "" before any such launch.  Host side; for tests that must know which kernel they ran.  The pointer is to a thread-local
 * buffer that the thread's next such launch overwrites: read or copy it before launching again */
const char *shl_mi355x_last_igemm_flavour(void);
/* bytes of packed weights + tables resident in HBM for this plan */
size_t shl_mi355x_conv_plan_bytes(const shl_mi355x_conv_plan *plan);
/*
 * Weight broadcast support: expose the plan's constant HBM block so that the
 * caller can ncclBroadcast it from rank 0; contents are position-independent.
 */
void *shl_mi355x_conv_plan_const_block(shl_mi355x_conv_plan *plan, size_t *bytes);
/* After the block was overwritten by a weight broadcast: adopt the sender's host-derived epilogue choices (exact
 * power-of-two fold, multiply-and-correct division, activation-as-clamp bounds, row-patch wave roles) from the 64-byte
 * record at the end of the block, so that tables and code path always come from the same rank. */
int shl_mi355x_conv_plan_adopt_block(shl_mi355x_conv_plan *plan, void *stream);

/*
 * Enqueue one forward pass: out = act(requant(conv(in))).
 *
 * int8 : bit-exact restatement of shl_ref_conv2d_quant / shl_ref_depthwise_conv2d_quant /
 *        shl_ref_fullyconnected_quant (source/reference/convolution.c:370-400, :416-460,
 *        fullyconnected.c:54-87) in exact integer arithmetic with an fp32 epilogue
 *        (see DESIGN.md "numerical contract").
 * f16  : same functions, dtype FLOAT16; fp32 accumulation, reference rounding on store.
 *
 * `batch` overrides desc.batch for this call (<= the plan's batch is NOT required: the plan
 * is batch independent); pass 0 to use the plan's batch.
 */
int shl_mi355x_conv_forward(const shl_mi355x_conv_plan *plan, const void *input_dev,
                            void *output_dev, int32_t batch, void *stream);

/* global_avgpool2d + the convolution / fullyconnected layer that consumes the pooled [N, 1, 1, C] map, in ONE launch
 * (MobileNetV1's tail; int8 NHWC, at most 64 pooled pixels and 8 images): `input_dev` is the POOL's input [N][pixels][C],
 * (in_scale, in_zp) its record, (mid_scale, mid_zp) the pooled tensor's record (= the plan's input record).  Bit-identical to
 * shl_mi355x_global_avgpool2d followed by shl_mi355x_conv_forward (the same operations in the reference's order:
 * source/reference/global_averagepool.c:46-50, averagepool.c:21-119).  _fusable: 1 when the plan and the sizes qualify. */
int shl_mi355x_pool_conv_fusable(const shl_mi355x_conv_plan *plan, int32_t batch, int32_t pixels);
int shl_mi355x_pool_conv_forward(const shl_mi355x_conv_plan *plan, const void *input_dev, void *output_dev, int32_t batch,
                                 int32_t pixels, float in_scale, int32_t in_zp, float mid_scale, int32_t mid_zp, void *stream);
/* The other order at the end of a classifier's body: a pointwise 1x1 convolution (int8 NHWC, a map of at most 64 pixels, 256 / 512 /
 * 1024 input channels) + the global_avgpool2d that consumes it, as ONE launch (csrc/conv1x1_latency.hip: the workgroup that owns a
 * 32-channel slice of an image holds all of its pixels, so it pools them right away).  `map_dev` receives the convolution's own
 * output tensor and may be NULL when only the pooled tensor is read; (mid_scale, mid_zp) is the convolution's output record (= the
 * pooling layer's input record), (out_scale, out_zp) the pooled tensor's.  Bit-identical to shl_mi355x_conv_forward followed by
 * shl_mi355x_global_avgpool2d (source/reference/convolution.c:370-400, global_averagepool.c:46-50, averagepool.c:21-119).
 * _fusable: 1 when the plan and the batch qualify (SHL_MI355X_CONVPOOL=0 turns it off). */
int shl_mi355x_conv_pool_fusable(const shl_mi355x_conv_plan *plan, int32_t batch);
int shl_mi355x_conv_pool_forward(const shl_mi355x_conv_plan *plan, const void *input_dev, void *map_dev, void *pool_dev, int32_t batch,
                                 float mid_scale, int32_t mid_zp, float out_scale, int32_t out_zp, void *stream);
/* The tail of a skip connection -- conv2d [+ its folded activation] -> add(conv_out, skip) -> [relu | relu6] -- as ONE launch of
 * the convolution (csrc/conv_igemm.hip, csrc/residual_step.h): int8, NHWC, plans of SHL_MI355X_ALGO_IGEMM.  `skip_dev` has the
 * output's shape and layout.  Between requantisation and store the kernel applies the add's and the activation's element
 * functions to the byte the convolution would have stored, so the launch equals shl_mi355x_conv_forward, shl_mi355x_add and
 * shl_mi355x_relu_i8 one after the other bit for bit, for every record.  The convolution's own output record is the plan's.
 * Two kernel families carry the post-op, the wave kernel and the tile kernels; a fused launch ignores the plan's tuned
 * variant and picks between them by the size rule, SHL_MI355X_RESIDUAL_FORM=wave|tile (read per call) forces one.
 * SHL_MI355X_EINVAL before anything is enqueued: a NULL argument, an `act` outside 0 .. 2, a scale that is no positive finite
 * number, an output that overlaps the input or the skip tensor (the skip tensor may BE the input), a batch that gives 2^31 or
 * more output pixels.  SHL_MI355X_ENOTSUP: a plan that is not int8 / NHWC / implicit GEMM, or a transposed convolution. */
struct shl_mi355x_residual_desc {
    int32_t conv_first;            /* the convolution's output is the add's first operand (else its second) */
    float skip_scale;  int32_t skip_zp;  /* the other operand's record */
    float sum_scale;   int32_t sum_zp;   /* the add's output record (= the activation's input record) */
    int32_t act;                   /* 0 none (the sum is the result), 1 relu, 2 relu6 */
    float out_scale;   int32_t out_zp;   /* the activation's output record; ignored when act == 0 */
};
/* 1 when the plan and the batch qualify (batch 0: the plan's) */
int shl_mi355x_conv_add_fusable(const shl_mi355x_conv_plan *plan, int32_t batch);
int shl_mi355x_conv_add_forward(const shl_mi355x_conv_plan *plan, const void *input_dev, const void *skip_dev, void *output_dev,
                                int32_t batch, const struct shl_mi355x_residual_desc *desc, void *stream);
/* the family a fused launch of this plan runs at `batch`, with the post-op behind it: "wave+add" or "tile+add" (the activation
 * is a field of the record, not another kernel); "" where the fused launch is not supported.  Pure host code */
const char *shl_mi355x_conv_add_kernel_name(const shl_mi355x_conv_plan *plan, int32_t batch);
/* 1 for the shape classes where the fused launch was measured faster than the launches it replaces by more than their
 * run-to-run spread (profiles/residual_notes.md): what a session fuses without being asked */
int shl_mi355x_conv_add_by_default(const shl_mi355x_conv_plan *plan, int32_t batch);
/* The same tail behind a binary16 convolution, entry points of their own: binary16, NHWC, plans of SHL_MI355X_ALGO_IGEMM (the
 * four above keep refusing a binary16 plan, these refuse every other one with SHL_MI355X_ENOTSUP, "", 0 and 0).  The descriptor
 * is the same struct; only `conv_first` and `act` are read -- binary16 tensors of a fused tail have scale 1 and the scale fields
 * are not validated.  On the four halves the convolution would have stored (its folded relu / relu6 and its rounding included)
 * the kernel runs the element functions of shl_mi355x_add (the same-shape add, whose NaN is the hardware's pick -- `conv_first`
 * decides which of two NaNs goes through) and shl_mi355x_relu_f16, so the launch equals shl_mi355x_conv_forward, shl_mi355x_add
 * and shl_mi355x_relu_f16 one after the other bit for bit, NaNs and infinities included, wherever the convolution alone runs
 * the same accumulation order: the wave and tile kernels add the K steps up in one order, the wave kernel's split-K form (few
 * tiles, K rows of 256 bytes and more) in another, and the other binary16 families (row-patch, ping-pong, gemv) in theirs, as
 * they always did among themselves -- fp32 sums of the same products, rounded once to binary16.
 * SHL_MI355X_EINVAL before anything is enqueued: a NULL argument, an `act` outside 0 .. 2, a batch that gives 2^31 or more
 * output pixels, a skip pointer that is not 2-byte aligned, a buffer that wraps around the address space, an output that
 * overlaps the input or the skip tensor (sizes count 2-byte elements).  SHL_MI355X_RESIDUAL_FORM forces the family likewise;
 * _by_default: the classes of profiles/residual_f16_notes.md */
int shl_mi355x_conv_add_f16_fusable(const shl_mi355x_conv_plan *plan, int32_t batch);
int shl_mi355x_conv_add_f16_forward(const shl_mi355x_conv_plan *plan, const void *input_dev, const void *skip_dev, void *output_dev,
                                    int32_t batch, const struct shl_mi355x_residual_desc *desc, void *stream);
const char *shl_mi355x_conv_add_f16_kernel_name(const shl_mi355x_conv_plan *plan, int32_t batch);
int shl_mi355x_conv_add_f16_by_default(const shl_mi355x_conv_plan *plan, int32_t batch);
/* An int8 activation that is a 256-entry table -- sigmoid / hard_sigmoid / silu / leaky_relu behind the convolution, or the
 * gate of a swish / hard-swish, mul(x, act(x)), which depends on x's byte alone -- as ONE launch of the convolution
 * (csrc/conv_igemm.hip, csrc/lut_step.h): int8, NHWC, plans of SHL_MI355X_ALGO_IGEMM.  `table` is HOST memory, 256 bytes,
 * entry (uint8_t)q for input byte q, as shl_mi355x_unary_lut_i8 takes it; it travels by value in the kernel arguments, so the
 * launch allocates nothing and is capturable.  Between requantisation and store the kernel looks up the byte the
 * convolution would have stored (folded relu / relu6 and saturation included), so the launch equals shl_mi355x_conv_forward
 * followed by shl_mi355x_unary_lut_i8 with the same table byte for byte, for ANY 256 bytes.
 * Two kernel families carry the post-op, the wave kernel and the tile kernels; a fused launch ignores the plan's tuned
 * variant and picks between them by the size rule, SHL_MI355X_ACT_FORM=wave|tile (read per call) forces one; there is no fused
 * launch while SHL_MI355X_IGEMM forces a family.
 * SHL_MI355X_EINVAL before anything is enqueued: a NULL argument, an output that overlaps the input, a batch that gives 2^31
 * or more output pixels.  SHL_MI355X_ENOTSUP: a plan that is not int8 / NHWC / implicit GEMM, or a transposed convolution. */
/* 1 when the plan and the batch qualify (batch 0: the plan's) */
int shl_mi355x_conv_lut_fusable(const shl_mi355x_conv_plan *plan, int32_t batch);
/* the family a fused launch of this plan runs at `batch`, with the post-op behind it: "wave+lut" or "tile+lut"; "" where the
 * fused launch is not supported.  Pure host code */
const char *shl_mi355x_conv_lut_kernel_name(const shl_mi355x_conv_plan *plan, int32_t batch);
/* 1 for the shape classes where the fused launch was measured faster than the two launches it replaces by more than their
 * run-to-run spread (profiles/act_fuse_notes.md): what a session fuses without being asked */
int shl_mi355x_conv_lut_by_default(const shl_mi355x_conv_plan *plan, int32_t batch);
int shl_mi355x_conv_lut_forward(const shl_mi355x_conv_plan *plan, const void *input_dev, void *output_dev, int32_t batch,
                                const uint8_t table[256], void *stream);
/* The same post-op behind a DEPTHWISE layer, as ONE launch of the depthwise kernel (csrc/dwconv.hip, csrc/dwconv_mfma.hip):
 * int8, NHWC, plans of SHL_MI355X_ALGO_DW (depth multiplier 1).  The four entries above keep refusing such a plan; these
 * four refuse every other one.  `table` as above, by value in the kernel arguments (nothing allocated, capturable) and 256
 * bytes of LDS per workgroup.  The kernel is the one shl_mi355x_conv_forward runs for the same plan and batch -- the dot4
 * kernel, the matrix-core kernel (its size rule and SHL_MI355X_DWMFMA honoured) or the generic one for kernels other than
 * 3x3 -- and looks up the dword its unfused store would have written, so the launch equals shl_mi355x_conv_forward followed
 * by shl_mi355x_unary_lut_i8 with the same table byte for byte, for ANY 256 bytes.
 * SHL_MI355X_EINVAL before anything is enqueued: a NULL argument, an output that overlaps the input, a batch that gives 2^31
 * or more output pixels.  SHL_MI355X_ENOTSUP: a plan that is not int8 / NHWC / depthwise (NCHW, binary16, implicit GEMM,
 * depth multiplier above 1, per-channel depthwise, a transposed convolution), an output row beyond the dot4 kernel's grid. */
/* 1 when the plan and the batch qualify (batch 0: the plan's) */
int shl_mi355x_dwconv_lut_fusable(const shl_mi355x_conv_plan *plan, int32_t batch);
/* the kernel a fused launch of this plan runs at `batch`, with the post-op behind it: "dwconv_dot4+lut", "dwconv_mfma+lut" or
 * "dwconv_nhwc+lut"; "" where the fused launch is not supported.  Pure host code */
const char *shl_mi355x_dwconv_lut_kernel_name(const shl_mi355x_conv_plan *plan, int32_t batch);
/* 1 for the shape classes where the fused launch was measured faster than the two launches it replaces by more than their
 * run-to-run spread (profiles/dw_act_fuse_notes.md): what a session fuses without being asked */
int shl_mi355x_dwconv_lut_by_default(const shl_mi355x_conv_plan *plan, int32_t batch);
int shl_mi355x_dwconv_lut_forward(const shl_mi355x_conv_plan *plan, const void *input_dev, void *output_dev, int32_t batch,
                                  const uint8_t table[256], void *stream);
/* A hint from the owner of the graph: this depthwise layer's output does NOT feed a pointwise layer the bandwidth form
 * (depthwise -> pointwise in one launch, large batches) takes -- the latency form (pointwise -> depthwise) then keeps the
 * layer instead of yielding it (shl_mi355x_pwdw_fusable asks plan pairs, it cannot see a layer's consumer). */
int shl_mi355x_conv_plan_set_no_stream_consumer(shl_mi355x_conv_plan *plan, int32_t on);
/*
 * Pointwise 1x1 + the depthwise 3x3 that consumes its output, as ONE launch (int8 NHWC): a workgroup
 * owns a 32-channel slice of shl_ref_conv2d_quant's output over a small pixel patch, keeps the int8
 * result in LDS and runs shl_ref_depthwise_conv2d_quant on those channels from there -- same bits as
 * the two plans back to back; the pointwise output (the largest tensors of a MobileNet) is never
 * written.  `input_dev` is the pointwise layer's input, `output_dev` the depthwise layer's output.
 *
 * The same two entry points take the pair in the OTHER order -- first plan = a depthwise 3x3 layer, second plan =
 * the pointwise layer consuming it (32 / 64 / 128 / 256 channels, int8 NHWC, throughput batches; csrc/dwpw_stream.hip):
 * the requantised depthwise tile is the pointwise layer's MFMA operand and never leaves the chip.  `input_dev` is
 * always the first layer's input and `output_dev` the second layer's output; the plans say which order it is.
 */
int shl_mi355x_pwdw_fusable(const shl_mi355x_conv_plan *pw, const shl_mi355x_conv_plan *dw, int32_t batch);
/* which fused kernel would run the pair: 0 none (= not fusable), else the form's number (conv_plan.hip:pwdw_kernel_for: 1 latency
 * form, 3 stem + depthwise, 4 / 5 binary16 NCHW, 6 dwpw_stream, 7 dwpw_resident) -- for tools and tests that name the kernel */
int shl_mi355x_pwdw_form(const shl_mi355x_conv_plan *pw, const shl_mi355x_conv_plan *dw, int32_t batch);
/* the geometry the latency form (1) would run the pair with, read-only, for tools and tests: out[0..11] = rectangles per image
 * along y and x, a rectangle's output rows and columns, the extra rows of the first / last rectangle along y and the extra columns
 * of the first / last along x (0 or 1: a border rectangle's patch has a row / column of padding, which costs no pointwise work),
 * 32-pixel MFMA tiles per workgroup, K split, pixels of the largest in-image window, workgroups of the launch.  `count` >= 12.
 * SHL_MI355X_ENOTSUP when the pair runs another form or none. */
int shl_mi355x_pwdw_geometry(const shl_mi355x_conv_plan *pw, const shl_mi355x_conv_plan *dw, int32_t batch, int32_t *out, int32_t count);
/* which instantiation of the latency form (1) would launch for the pair, read-only, for tools and tests: out[0] = one of the
 * kinds below, out[1..4] = what a fixed form was compiled for -- K sub-steps per wave, K split, tiles per wave, tiles per window
 * (all 0 for the run-time form).  FIXED_EXACT: the window has exactly tiles-per-wave x wave-groups tiles; FIXED_PADDED: fewer, the
 * form reads the count at run time; NT: the window's own, uneven count is compiled in.  SHL_MI355X_PWDW_GENERIC=1 gives RUNTIME
 * everywhere.  `count` >= 5.  SHL_MI355X_ENOTSUP when the pair runs another form or none. */
enum {
    SHL_MI355X_PWDW_LAUNCH_RUNTIME = 0,
    SHL_MI355X_PWDW_LAUNCH_FIXED_PADDED = 1,
    SHL_MI355X_PWDW_LAUNCH_FIXED_EXACT = 2,
    SHL_MI355X_PWDW_LAUNCH_NT = 3
};
int shl_mi355x_pwdw_launch_form(const shl_mi355x_conv_plan *pw, const shl_mi355x_conv_plan *dw, int32_t batch, int32_t *out, int32_t count);
int shl_mi355x_pwdw_forward(const shl_mi355x_conv_plan *pw, const shl_mi355x_conv_plan *dw,
                            const void *input_dev, void *output_dev, int32_t batch, void *stream);

/* ---- elementwise neighbours of the path ---------------------------------- */
/* relu / relu6 on a quantised int8 tensor: shl_ref_relu_quant / shl_ref_relu6_quant
 * (source/reference/relu.c:21-43, relu6.c:21-43) */
int shl_mi355x_relu_i8(const int8_t *input_dev, int8_t *output_dev, size_t count,
                       float in_scale, int32_t in_zp, float out_scale, int32_t out_zp,
                       int32_t relu6, void *stream);

/* binary16 relu / relu6 (same reference functions, dtype FLOAT16, qinfo scale 1) */
int shl_mi355x_relu_f16(const uint16_t *input_dev, uint16_t *output_dev, size_t count, int32_t relu6,
                        void *stream);

/* elementwise add of two same-shape tensors (residual connection): shl_ref_add_quant
 * (source/reference/add.c:21-41): dequantise both, fp32 add, requantise.  f16: scales ignored. */
int shl_mi355x_add(const void *input0_dev, const void *input1_dev, void *output_dev, size_t count,
                   int32_t dtype, float scale0, int32_t zp0, float scale1, int32_t zp1, float out_scale,
                   int32_t out_zp, void *stream);

/* global average pooling over H*W (`pixels`) of an int8 / binary16 tensor:
 * shl_ref_global_avgpool2d_quant (source/reference/global_averagepool.c:21-50 ->
 * averagepool.c:21-119), same fp32 summation order.  Output is [N, C] (NHWC [N,1,1,C] or NCHW
 * [N,C,1,1]).  f16: the scale arguments are ignored. */
int shl_mi355x_global_avgpool2d(const void *input_dev, void *output_dev, int32_t dtype, int32_t layout,
                                int32_t batch, int32_t channels, int32_t pixels, float in_scale,
                                int32_t in_zp, float out_scale, int32_t out_zp, void *stream);

/* windowed max / average pooling of an int8 / binary16 tensor: shl_ref_maxpool2d_quant / shl_ref_avgpool2d_quant
 * (source/reference/maxpool.c:21-124, averagepool.c:21-138), bit for bit for any scales.  The window of output
 * (oy, ox) starts at (oy * stride_h - pad_top, ox * stride_w - pad_left) and is clamped to the image; out_h / out_w
 * are the OUTPUT TENSOR's dims (ceil_mode, pad_down and pad_right act through them only).  avg divides by the number
 * of in-image taps, or by kernel_h * kernel_w with count_include_pad.  f16: scales and zero points are ignored.
 * A shape in which some window holds no input element is refused (SHL_MI355X_EINVAL).  Enqueues only: no allocation,
 * no synchronisation (capturable in a hipGraph). */
enum shl_mi355x_pool_kind {
    SHL_MI355X_POOL_MAX = 0,
    SHL_MI355X_POOL_AVG = 1
};

struct shl_mi355x_pool_desc {
    int32_t kind;   /* shl_mi355x_pool_kind */
    int32_t dtype;  /* SHL_MI355X_I8 / SHL_MI355X_F16 */
    int32_t layout; /* SHL_MI355X_NHWC / SHL_MI355X_NCHW */
    int32_t batch, c, in_h, in_w, out_h, out_w;
    int32_t kernel_h, kernel_w, stride_h, stride_w, pad_top, pad_left;
    int32_t count_include_pad;
    int32_t in_zp, out_zp;
    float in_scale, out_scale;
    int32_t reserved[4]; /* must be zero */
};

int shl_mi355x_pool2d(const void *in_dev, void *out_dev, const struct shl_mi355x_pool_desc *d, void *stream);
/* the kernel form the rules choose for `d` ("pool2d_nhwc_vec", "pool2d_nchw_row", "pool2d_generic"; "" for an
 * invalid descriptor).  Pure host code: touches no device */
const char *shl_mi355x_pool2d_kernel_name(const struct shl_mi355x_pool_desc *d);

/* concat of n_inputs int8 / binary16 tensors along one axis: shl_ref_concat_quant (source/reference/concat.c:21-76), bit
 * for bit.  The output is viewed as [outer][row], row = sum of len[i]; input i is [outer][len[i]] (len[i] = its axis dim
 * times the product of the dims behind the axis, in elements) and lands at column sum of len[0..i).  Every input is
 * dequantised with its own record and requantised with the output's (int8; an input whose record equals the output's is
 * copied as bytes once that round trip was checked to be the identity); binary16 passes through the reference's
 * float32 -> binary16 conversion (infinities saturate to +-65504, every NaN becomes 0x7FFF / 0xFFFF), scales and zero
 * points are ignored.  Inputs of len 0 are skipped; the same buffer may be given more than once; the output must not
 * overlap an input.  Up to 8 inputs travel in one launch, more in further launches.  Enqueues only: no allocation, no
 * upload, no synchronisation (capturable in a hipGraph). */
struct shl_mi355x_concat_desc {
    int32_t dtype;    /* SHL_MI355X_I8 / SHL_MI355X_F16 */
    int32_t n_inputs; /* >= 1, no upper bound */
    int64_t outer;    /* product of the dims in front of the axis */
    float out_scale;
    int32_t out_zp;
    int32_t reserved[4]; /* must be zero */
};

int shl_mi355x_concat(const void *const *in_dev, const int64_t *len, const float *in_scale, const int32_t *in_zp,
                      void *out_dev, const struct shl_mi355x_concat_desc *d, void *stream);
/* the kernel form the rules choose ("concat_vec": 16 bytes per thread, when every len[i] in bytes is a multiple of 16
 * and every pointer is 16-byte aligned; "concat_generic": one element per thread; "" for invalid arguments).  Pure host
 * code: looks at the pointers' values only, touches no device */
const char *shl_mi355x_concat_kernel_name(const void *const *in_dev, const int64_t *len, const float *in_scale,
                                          const int32_t *in_zp, const void *out_dev,
                                          const struct shl_mi355x_concat_desc *d);

/* split of an int8 / binary16 tensor along one axis into n_outputs tensors: shl_ref_split_quant
 * (source/reference/split.c:74-92), bit for bit -- the mirror of concat.  The input is viewed as [outer][row], row = sum of
 * len[i]; output i is [outer][len[i]] (len[i] = its axis dim times the product of the dims behind the axis, in elements,
 * > 0) and holds columns sum of len[0..i) onwards.  Every output has its OWN record: the input is dequantised with its
 * record and requantised with the output's (int8; an output whose record equals the input's is copied as bytes once that
 * round trip was checked to be the identity); binary16 passes through the reference's float32 -> binary16 conversion
 * (infinities saturate to +-65504, every NaN becomes 0x7FFF / 0xFFFF), scales and zero points are ignored.  No output may
 * overlap the input or another output.  Up to 8 outputs travel in one launch, more in further launches.  Enqueues only: no
 * allocation, no upload, no synchronisation (capturable in a hipGraph). */
struct shl_mi355x_split_desc {
    int32_t dtype;     /* SHL_MI355X_I8 / SHL_MI355X_F16 */
    int32_t n_outputs; /* >= 1, no upper bound */
    int64_t outer;     /* product of the dims in front of the axis */
    float in_scale;
    int32_t in_zp;
    int32_t reserved[4]; /* must be zero */
};

int shl_mi355x_split(const void *in_dev, void *const *out_dev, const int64_t *len, const float *out_scale,
                     const int32_t *out_zp, const struct shl_mi355x_split_desc *d, void *stream);
/* the kernel form the rules choose ("split_vec": 16 bytes per thread, when every len[i] in bytes is a multiple of 16 and
 * every pointer is 16-byte aligned; "split_generic": one element per thread; "" for invalid arguments).
 * SHL_MI355X_SPLIT_FORM=generic forces the literal form; forcing `vec` where the arguments do not admit it gives generic.
 * Pure host code: looks at the pointers' values only, touches no device */
const char *shl_mi355x_split_kernel_name(const void *in_dev, void *const *out_dev, const int64_t *len, const float *out_scale,
                                         const int32_t *out_zp, const struct shl_mi355x_split_desc *d);

/* shuffle_channel: shl_ref_shuffle_channel_quant (source/reference/shuffle_channel.c), bit for bit.  The tensor is viewed
 * as [outer][c][inner] (NHWC: outer = N H W, inner = 1; NCHW: outer = N, inner = H W); with gc = c / group,
 * out[.., j * group + k, ..] = in[.., k * gc + j, ..] for j < gc, k < group.  Elements travel as split's do: int8 dequantised
 * and requantised (a byte copy for equal records whose round trip is the identity), binary16 through the reference's
 * conversion.  c % group != 0, group < 1 and an output that overlaps the input are refused.  Enqueues only: no allocation,
 * no upload, no synchronisation (capturable in a hipGraph). */
struct shl_mi355x_shuffle_desc {
    int32_t dtype; /* SHL_MI355X_I8 / SHL_MI355X_F16 */
    int32_t group;
    int64_t outer, c, inner;
    float in_scale;
    int32_t in_zp;
    float out_scale;
    int32_t out_zp;
    int32_t reserved[4]; /* must be zero */
};

int shl_mi355x_shuffle_channel(const void *in_dev, void *out_dev, const struct shl_mi355x_shuffle_desc *d, void *stream);
/* the kernel form the rules choose; "" for invalid arguments.  Pure host code, touches no device.
 *   "shuffle_plane_16" / "shuffle_plane_4"   inner in bytes a multiple of 16 / of 4, pointers aligned alike: pieces of a
 *                                            plane are copied plane to plane
 *   "shuffle_pixel_16" / "shuffle_pixel_4"   inner == 1, c in bytes a multiple of 16 / of 4 and at most 8192, pointers
 *                                            aligned alike: a workgroup permutes a run of pixels through LDS
 *   "shuffle_generic"                        one element per thread
 * SHL_MI355X_SHUFFLE_FORM=generic | plane | pixel forces a form; one the arguments do not admit gives generic */
const char *shl_mi355x_shuffle_channel_kernel_name(const void *in_dev, const void *out_dev,
                                                   const struct shl_mi355x_shuffle_desc *d);

/* The operators that only change a tensor's order or shape: transpose, pad, and the flat move behind reshape / flatten.  In
 * the reference all of them go through shl_ref_siso_callback_base -- dequantise, move, requantise with the output's record
 * -- so elements travel as split's do: int8 q_out = sat8(rint(((q - zp_in) * s_in) / s_out) + zp_out) (a byte copy for equal
 * records whose round trip is the identity, div_by_scale where the records admit it, the hardware's division otherwise);
 * binary16 through the reference's conversion (infinities saturate to +-65504, every NaN becomes 0x7FFF / 0xFFFF), scales
 * and zero points ignored.  The output may not overlap the input.  All enqueue only: no allocation, no upload, no
 * synchronisation (capturable in a hipGraph). */
#define SHL_MI355X_MAX_DIM 8

/* transpose: shl_ref_transpose (source/reference/transpose.c), bit for bit: output dim k is input dim perm[k].  rank
 * 1 .. 8, perm a permutation of 0 .. rank - 1, dims >= 0; anything else is SHL_MI355X_EINVAL before anything is enqueued.
 * The layer is canonicalised on the host -- dims of extent 1 dropped, dims adjacent in the same order in input and output
 * merged -- and one of four forms runs:
 *   "transpose_flat"      the canonical permutation is the identity and both pointers are 16-byte aligned: 16 bytes per
 *                         thread, the last thread finishing a tail of fewer than 16 bytes by elements
 *   "transpose_rows_16" / "transpose_rows_4"   the innermost canonical dim stays innermost and a run of it in bytes is a
 *                         multiple of 16 / of 4, pointers aligned alike: one piece per thread in output order, the outer
 *                         coordinates taken apart by division
 *   "transpose_tile_4" / "_4_1" / "_1_4" / "_1"   the output's innermost canonical dim is not the input's: 64 x 64-element
 *                         tiles over (input's innermost, output's innermost) through LDS, reads along the input's
 *                         contiguous dim, writes along the output's, every other dim a batch coordinate; edge tiles are
 *                         masked.  A side whose extent in bytes is a multiple of 4 and whose pointer is 4-byte aligned
 *                         moves dwords, the other one element per lane (ragged extents: 7 x 7 maps, 85-value heads):
 *                         _4 dwords on both sides, _4_1 dword loads and element stores, _1_4 the reverse, _1 elements
 *   "transpose_generic"   one output element per thread
 * SHL_MI355X_TRANSPOSE_FORM=generic | tile | rows forces a form; one the arguments do not admit gives generic. */
struct shl_mi355x_transpose_desc {
    int32_t dtype; /* SHL_MI355X_I8 / SHL_MI355X_F16 */
    int32_t rank;
    int32_t dim[SHL_MI355X_MAX_DIM];  /* the INPUT's dims */
    int32_t perm[SHL_MI355X_MAX_DIM]; /* output dim k = input dim perm[k] */
    float in_scale;
    int32_t in_zp;
    float out_scale;
    int32_t out_zp;
    int32_t reserved[4]; /* must be zero */
};

int shl_mi355x_transpose(const void *in_dev, void *out_dev, const struct shl_mi355x_transpose_desc *d, void *stream);
/* the kernel form the rules choose; "" for invalid arguments.  Pure host code, touches no device */
const char *shl_mi355x_transpose_kernel_name(const void *in_dev, const void *out_dev,
                                             const struct shl_mi355x_transpose_desc *d);

/* the flat requantised move of `elems` elements: what reshape and flatten are (the reference copies
 * csinn_tensor_byte_size(input) bytes between the two conversions).  Runs "transpose_flat" when both pointers are 16-byte
 * aligned, "transpose_rows_4" when they are 4-byte aligned and the bytes a multiple of 4, else "transpose_generic";
 * SHL_MI355X_TRANSPOSE_FORM applies. */
struct shl_mi355x_move_desc {
    int32_t dtype; /* SHL_MI355X_I8 / SHL_MI355X_F16 */
    float in_scale;
    int32_t in_zp;
    float out_scale;
    int32_t out_zp;
    int32_t reserved[3]; /* must be zero */
};

int shl_mi355x_move(const void *in_dev, void *out_dev, int64_t elems, const struct shl_mi355x_move_desc *d, void *stream);
const char *shl_mi355x_move_kernel_name(const void *in_dev, const void *out_dev, int64_t elems,
                                        const struct shl_mi355x_move_desc *d);

/* constant pad of a 4-d tensor: shl_ref_pad_f32 (source/reference/pad.c) between the two conversions, bit for bit.  Dim k
 * of the output is before[k] + dim[k] + after[k], in memory order -- NCHW and NHWC differ only in what the caller calls the
 * dims.  The pad element is computed ONCE on the host as the reference's conversion of the float32 pad_value with the
 * OUTPUT's record: int8 sat8(rint(v / s_out) + zp_out), binary16 float32_to_float16_base(v) (-inf: 0xFBFF).  Negative
 * pads or dims are SHL_MI355X_EINVAL.  Two forms:
 *   "pad_vec"      16 bytes per thread in output order.  With j the innermost dim that is padded (dim 0 when none is) and U
 *                  the bytes of one step along it (the dims behind it times the element size): before[j] * U, dim[j] * U
 *                  and after[j] * U are multiples of 16 and both pointers 16-byte aligned -- every piece then is all pad or
 *                  all interior, and an interior piece's source is aligned.  NHWC with H / W padding only meets it whenever
 *                  C in bytes is a multiple of 16 (W * C then is too)
 *   "pad_generic"  one output element per thread
 * SHL_MI355X_PAD_FORM=generic forces the literal form. */
struct shl_mi355x_pad_desc {
    int32_t dtype; /* SHL_MI355X_I8 / SHL_MI355X_F16 */
    int32_t dim[4]; /* the INPUT's dims */
    int32_t before[4], after[4];
    float pad_value;
    float in_scale;
    int32_t in_zp;
    float out_scale;
    int32_t out_zp;
    int32_t reserved[4]; /* must be zero */
};

int shl_mi355x_pad(const void *in_dev, void *out_dev, const struct shl_mi355x_pad_desc *d, void *stream);
const char *shl_mi355x_pad_kernel_name(const void *in_dev, const void *out_dev, const struct shl_mi355x_pad_desc *d);
/* the pad element as the kernels write it (low byte / low half): pure host code */
uint32_t shl_mi355x_pad_element(const struct shl_mi355x_pad_desc *d);

/* Reductions: sum, mean, max and min of an int8 / binary16 tensor over any set of dims -- what CSINN_OP_MEAN / _SUM / _MAX /
 * _MIN (shl_ref_*_stride_f32), CSINN_OP_REDUCE_MEAN / _SUM / _MAX / _MIN (shl_ref_reduce_*_f32) and
 * CSINN_OP_GLOBAL_MAXPOOL2D are behind shl_ref_siso_callback_base, bit for bit.  Output o (0 .. product of out_extent - 1)
 * reads in[index(o, out) + index(i, inner)] for i = 0 .. product of inner_extent - 1 IN THAT ORDER, index() being the
 * reference's mixed-radix index (shl_ref_get_reduction_index: the first group is the outermost digit), strides in input
 * elements.  sum / mean: a float32 chain from 0 in that order, mean ends with one division by the count.  max / min: the C
 * library's fmax / fmin in that order (a NaN loses, of two NaNs the first stays, of +0 and -0 the later one), from -FLT_MAX /
 * +FLT_MAX (SHL_MI355X_REDUCE_INIT_FLT_MAX: the stride family, global_maxpool2d -- a row of NaNs gives -FLT_MAX, which
 * binary16 rounds to -65504) or from the row's first element (SHL_MI355X_REDUCE_INIT_FIRST: the axis family); `init` is
 * ignored by sum and mean.  Elements: int8 (q - zp_in) * s_in, binary16 exact; outputs: int8 sat8(rint(x / s_out) + zp_out),
 * binary16 the reference's conversion.
 * SHL_MI355X_EINVAL before anything is enqueued: more than 8 groups in a list; a negative extent or stride, an inner extent
 * below 1; in_elems below 1 or 2^31 and above; 2^31 or more outputs or elements per output; an index that reaches in_elems;
 * a pointer not aligned to its elements; an output that overlaps the input; more than SHL_MI355X_REDUCE_GROUPS groups left in
 * a list after canonicalisation (extent-1 groups dropped, a group merged into the one before it when that one's stride is
 * this one's extent times its stride).  No outputs (an outer extent of 0): SHL_MI355X_OK, nothing enqueued.  Enqueues only:
 * no allocation, no synchronisation (capturable in a hipGraph).  Forms:
 *   SHL_MI355X_REDUCE_ROWS     the innermost canonical inner group has stride 1: a workgroup stages windows of its rows
 *                              into LDS with 16-byte loads (element loads where a row's head or tail is off the 16-byte
 *                              grid), one lane per row then adds in order.  The staging chunk is
 *                              SHL_MI355X_REDUCE_CHUNK_BYTES per row and pass
 *   SHL_MI355X_REDUCE_COLS     else, the innermost canonical outer group has stride 1: one output per thread, coalesced
 *                              loads issued in batches ahead of the additions
 *   SHL_MI355X_REDUCE_GENERIC  one output per thread, every index by division
 * SHL_MI355X_REDUCE_FORM=generic forces the last. */
#define SHL_MI355X_REDUCE_GROUPS 4
#define SHL_MI355X_REDUCE_CHUNK_BYTES 256
#define SHL_MI355X_REDUCE_ROWS "reduce_rows"
#define SHL_MI355X_REDUCE_COLS "reduce_cols"
#define SHL_MI355X_REDUCE_GENERIC "reduce_generic"
enum { SHL_MI355X_REDUCE_SUM = 0, SHL_MI355X_REDUCE_MEAN = 1, SHL_MI355X_REDUCE_MAX = 2, SHL_MI355X_REDUCE_MIN = 3 };
enum { SHL_MI355X_REDUCE_INIT_FLT_MAX = 0, SHL_MI355X_REDUCE_INIT_FIRST = 1 };

struct shl_mi355x_reduce_desc {
    int32_t dtype; /* SHL_MI355X_I8 / SHL_MI355X_F16 */
    int32_t kind;  /* SHL_MI355X_REDUCE_SUM .. _MIN */
    int32_t init;  /* SHL_MI355X_REDUCE_INIT_* */
    int32_t n_out, n_inner;
    int32_t out_extent[SHL_MI355X_MAX_DIM], out_stride[SHL_MI355X_MAX_DIM];
    int32_t inner_extent[SHL_MI355X_MAX_DIM], inner_stride[SHL_MI355X_MAX_DIM];
    int32_t reserved0; /* must be zero */
    int64_t in_elems;  /* elements of the input tensor: no index may reach it */
    float in_scale;
    int32_t in_zp;
    float out_scale;
    int32_t out_zp;
    int32_t reserved[4]; /* must be zero */
};

int shl_mi355x_reduce(const void *in_dev, void *out_dev, const struct shl_mi355x_reduce_desc *d, void *stream);
/* the kernel form the rules choose; "" for invalid arguments.  Pure host code, touches no device */
const char *shl_mi355x_reduce_kernel_name(const void *in_dev, const void *out_dev, const struct shl_mi355x_reduce_desc *d);

/* Batched matrix product of two int8 / binary16 tensors: out[b][i][j] = sum over k of A[b][i][k] * B[b][k][j] -- what
 * CSINN_OP_MATMUL (shl_ref_matmul_f32 behind shl_ref_diso_callback_base, source/reference/matmul.c) computes.  The
 * caller turns the layer into strides, in elements: element (b, i, k) of A is at b a_batch_stride + i a_row_stride +
 * k a_k_stride, element (b, k, j) of B at b b_batch_stride + j b_col_stride + k b_k_stride; trans_a / trans_b swap an
 * operand's two strides, the reference's "dense" broadcast (one B for every batch of A) is b_batch_stride == 0.  The output
 * is dense: [batches][m][n].  Two forms (shl_mi355x_matmul_kernel_name says which the rule picks):
 *   SHL_MI355X_MATMUL_CHAIN  one output per thread, the reference's own float32 chain: int8 operands dequantised as
 *                            ((float)q - zp) * scale, one fused multiply-add per step (the reference's build contracts
 *                            `total += a * b`), k ascending, then
 *                            sat8(rint(x / s_out) + zp_out); binary16 exact widening and the reference's conversion.
 *                            Bit-identical to the reference for any records and any strides
 *   SHL_MI355X_MATMUL_MFMA   64 x 64 output tiles on the matrix cores.  int8: S = sum (qa - za)(qb - zb) exactly in int32,
 *                            f = (float)S * mult with mult = a_scale * b_scale rounded once, sat8(rint(f / s_out) + zp_out);
 *                            equal to the reference bit for bit when shl_mi355x_matmul_is_exact(), within 1 LSB otherwise.
 *                            binary16: exact products, float32 accumulation in another order than the chain's.  Needs
 *                            every operand to have a unit stride (k or row / column) and, int8, k <= 32768
 * SHL_MI355X_MATMUL_FORM=chain|mfma forces a form (mfma: where its geometry fits, else chain); read per call.
 * binary16 operands carry no records: the scales and zero points are ignored.
 * SHL_MI355X_EINVAL before anything is enqueued: batches, m, n or k below 1; a negative stride; a_elems / b_elems /
 * out_elems below 1 or 2^31 and above; out_elems other than batches * m * n; an index that reaches a_elems / b_elems;
 * pointers not aligned to their elements; the output overlapping an operand.  Enqueues only: no allocation, no
 * synchronisation (capturable in a hipGraph). */
#define SHL_MI355X_MATMUL_CHAIN "matmul_chain"
#define SHL_MI355X_MATMUL_MFMA "matmul_mfma"
#define SHL_MI355X_MATMUL_MFMA_MAX_K 32768

struct shl_mi355x_matmul_desc {
    int32_t dtype; /* SHL_MI355X_I8 / SHL_MI355X_F16 */
    int32_t batches;
    int32_t m, n, k;
    int32_t reserved0; /* must be zero */
    int64_t a_batch_stride, a_row_stride, a_k_stride; /* elements */
    int64_t b_batch_stride, b_col_stride, b_k_stride;
    int64_t a_elems, b_elems, out_elems; /* elements of the three tensors */
    float a_scale;
    int32_t a_zp;
    float b_scale;
    int32_t b_zp;
    float out_scale;
    int32_t out_zp;
    int32_t reserved[4]; /* must be zero */
};

int shl_mi355x_matmul(const void *a_dev, const void *b_dev, void *out_dev, const struct shl_mi355x_matmul_desc *d, void *stream);
/* the kernel form the rules choose; "" for invalid arguments.  Pure host code, touches no device */
const char *shl_mi355x_matmul_kernel_name(const void *a_dev, const void *b_dev, const void *out_dev,
                                          const struct shl_mi355x_matmul_desc *d);
/* 1 when the int8 mfma form is PROVEN equal to the reference's chain for every input: with each scale written m 2^e, m
 * odd, k * max(127 - za, za + 128) * max(127 - zb, zb + 128) * ma * mb < 2^24 -- every dequantised value, product and partial
 * sum of the chain then is exact.  Depends on k and the records only.  0 otherwise, for binary16 and for a NULL descriptor */
int shl_mi355x_matmul_is_exact(const struct shl_mi355x_matmul_desc *d);

/* A linear layer as converters export it -- MatMul(x, W) followed by Add(., bias[n]) -- as ONE launch: shl_mi355x_matmul with
 * the add in its store.  Per output the kernel computes the intermediate exactly as shl_mi355x_matmul would store it under
 * the record (mid_scale, mid_zp) -- int8: sat8(rint(f / mid_scale) + mid_zp), binary16: the rounded half, NaN rule included
 * -- keeps it in a register and applies shl_mi355x_add_bcast's arithmetic with bias[j], j the output's column, the same
 * for every batch and row: by construction the result equals shl_mi355x_matmul followed by shl_mi355x_add_bcast bit for bit,
 * in both forms and dtypes, whatever the records.  d->out_scale / out_zp are the record of the FINAL output (the add's),
 * bias_scale / bias_zp the bias's; bias_is_first: the bias is the add layer's first input (of two binary16 NaNs the second
 * input's goes through).  binary16 ignores every record.  bias_dev holds n elements of d's dtype; it must be aligned to its
 * elements and must not overlap the output.  Validation and form rule are shl_mi355x_matmul's; the kernels report as
 * "matmul_chain_bias" / "matmul_mfma_bias".  Enqueues only (capturable in a hipGraph). */
#define SHL_MI355X_MATMUL_CHAIN_BIAS "matmul_chain_bias"
#define SHL_MI355X_MATMUL_MFMA_BIAS "matmul_mfma_bias"
int shl_mi355x_matmul_bias(const void *a_dev, const void *b_dev, const void *bias_dev, void *out_dev,
                           const struct shl_mi355x_matmul_desc *d, float bias_scale, int32_t bias_zp, float mid_scale,
                           int32_t mid_zp, int32_t bias_is_first, void *stream);
const char *shl_mi355x_matmul_bias_kernel_name(const void *a_dev, const void *b_dev, const void *bias_dev, const void *out_dev,
                                               const struct shl_mi355x_matmul_desc *d);

/* The core of an attention block -- scores = Q K^T, [scores * constant], softmax over the keys, P V -- as ONE launch.  All
 * four tensors are dense, int8 or binary16: q[batches][s][d], k[batches][t][d] (the trans_b operand of Q K^T),
 * v[batches][t][dv], out[batches][s][dv]; a head is a batch.  The result equals, bit for bit and in both dtypes, the calls it
 * replaces: shl_mi355x_matmul (q, k with swapped strides; output record s_*) in its mfma form, then -- has_scale --
 * shl_mi355x_mul by a one-element constant (raw element scale_raw under c_*; output record sc_*), then shl_mi355x_softmax
 * along the last axis (output record p_*), then shl_mi355x_matmul (p, v; output record out_*) in its mfma form.  Equality is
 * by construction, as for shl_mi355x_matmul_bias: every intermediate is computed exactly as the unfused kernel would store it
 * -- the int8 byte under its record, the rounded half with the NaN rule --, stays in LDS and goes through the next layer's own
 * element function; both products run the mfma form's instructions on its fragment layout, k ascending in 64-byte slabs,
 * so binary16 sums are added in matmul_mfma's order.  scale_is_first: the constant is the mul layer's FIRST input (of two
 * binary16 NaNs the second input's goes through).  binary16 ignores every record.
 * A workgroup owns 32 query rows of one batch: four waves run the products, and 4, 8 or 16 -- as many as the grid leaves
 * room for on the chip and the LDS holds -- share the softmax, a row per wave at a time.  The 32 x t scores live in LDS, so t
 * is capped: SHL_MI355X_ATTENTION_MAX_KEYS.  At the cap in binary16 the kernel holds, in bytes: 32 rows x (2048 + 16) of
 * scores 66048 + a running-sum row of (1024 + 256) doubles per wave, 40960 for four + operand slabs (32 + 128) x 80 12800 +
 * row sums 512 = 120320 with four waves, 161280 of 163840 with the eight a small grid gets there (int8: 33280 + 40960 + 12800 +
 * 512 + per wave an exponential table of 256 doubles and one of 256 bytes, 9216 for four = 96768; with eight waves 146944).
 * d and dv are bounded by matmul's own rules only (int8: d <= 32768, zero points inside int8).
 * SHL_MI355X_EINVAL before anything is enqueued: a NULL argument; a dtype that is neither; batches, s, t, d or dv below 1; t
 * above the cap; a tensor (the scores included) of 2^31 or more elements; pointers not aligned to their elements; the output
 * overlapping an operand; has_scale / scale_is_first other than 0 or 1; a scale_raw that is no element of the dtype; non-zero
 * reserved fields.  SHL_MI355X_ENOTSUP when shl_mi355x_matmul's form rule gives either product the chain form (fewer than 64
 * steps of k with at most 65536 outputs, what the mfma form cannot take, SHL_MI355X_MATMUL_FORM=chain): equality holds
 * against the mfma form only, so the fused kernel exists only there.  Enqueues only: no allocation, no upload, no
 * synchronisation (capturable in a hipGraph). */
#define SHL_MI355X_ATTENTION_MFMA "attention_mfma"
#define SHL_MI355X_ATTENTION_MAX_KEYS 1024

struct shl_mi355x_attention_desc {
    int32_t dtype; /* SHL_MI355X_I8 / SHL_MI355X_F16 */
    int32_t batches;
    int32_t s, t, d, dv;
    int32_t has_scale;      /* 0: softmax reads the stored scores; 1: the scores times the constant */
    int32_t scale_is_first; /* the constant is the mul layer's first input */
    int32_t scale_raw;      /* the constant's raw element: an int8 value, or the 16 bits of a binary16 */
    int32_t reserved0;      /* must be zero */
    float q_scale, k_scale, v_scale;
    float s_scale;  /* the scores as Q K^T stores them */
    float c_scale;  /* the constant */
    float sc_scale; /* the scaled scores */
    float p_scale;  /* the probabilities */
    float out_scale;
    int32_t q_zp, k_zp, v_zp, s_zp, c_zp, sc_zp, p_zp, out_zp;
    int32_t reserved[4]; /* must be zero */
};

int shl_mi355x_attention(const void *q_dev, const void *k_dev, const void *v_dev, void *out_dev,
                         const struct shl_mi355x_attention_desc *d, void *stream);
/* "attention_mfma", or "" for what the call refuses.  Pure host code, touches no device */
const char *shl_mi355x_attention_kernel_name(const void *q_dev, const void *k_dev, const void *v_dev, const void *out_dev,
                                             const struct shl_mi355x_attention_desc *d);
/* 1 when the call names a kernel AND the shape belongs to a class in which the fused launch was measured faster than the four
 * launches it replaces (profiles/attention_notes.md: heads of at most 32 on at least 768 keys): what a session fuses without
 * being asked.  The call itself serves every shape that names a kernel.  Pure host code */
int shl_mi355x_attention_by_default(const void *q_dev, const void *k_dev, const void *v_dev, const void *out_dev,
                                    const struct shl_mi355x_attention_desc *d);

/* The same core with an additive bias or mask on the scores -- Q K^T, [scores * constant], + bias, softmax, P V -- as ONE
 * launch: a padding mask [B,1,1,T], a relative position bias [1,H,S,T], a causal mask [1,1,S,T].  `d` is the descriptor
 * above, unchanged; has_scale says whether the add reads the scaled scores (record sc_*) or the stored ones (s_*).  The bias
 * is int8 or binary16 like the rest, under the record b_*; the sum is stored -- in LDS -- under sb_*, and the softmax reads
 * that record.  The bias element of batch bi = i0 * b_ext1 + i1, query row and key is
 *     bias[i0 * b_stride[0] + i1 * b_stride[1] + row * row_stride + key * key_stride],
 * every stride in elements and 0 where the bias is broadcast (a stride along an extent of 1 is not read).
 * shl_mi355x_attention_bias_geometry derives these fields from the collapsed groups of the add's own descriptor.
 * The result equals, bit for bit, shl_mi355x_matmul -> [shl_mi355x_mul] -> shl_mi355x_add_bcast (a: the scores, b: the
 * bias, a_is_second = bias_is_first, the geometry the strides state) -> shl_mi355x_softmax -> shl_mi355x_matmul on the same
 * buffers: the sum is add_step.h's element function on the value the multiply (or the product) would have stored, in the
 * int8 variant (one fused multiply-add or the hardware's division) that shl_mi355x_add_bcast takes for the same three
 * records; binary16: of two NaNs the layer's second input's goes through, inf + -inf is 0xFFFF.
 * The bias pointer needs its element's alignment only; q, k, v and the output keep the rules above.  No LDS beyond
 * shl_mi355x_attention's.  SHL_MI355X_EINVAL before anything is enqueued: whatever shl_mi355x_attention refuses so; a NULL
 * bias or bias descriptor; a negative stride; b_ext1 below 1 or not dividing batches; a largest bias index of 2^31 or more;
 * bias_is_first other than 0 or 1; non-zero reserved fields; a bias pointer not aligned to its elements; the output
 * overlapping the bias.  SHL_MI355X_ENOTSUP where shl_mi355x_attention returns it.  Enqueues only: no allocation, no upload,
 * no synchronisation (capturable in a hipGraph). */
#define SHL_MI355X_ATTENTION_BIAS_MFMA "attention_bias_mfma"

struct shl_mi355x_attention_bias_desc {
    int32_t b_ext1;        /* the inner extent of the batch index: bi = i0 * b_ext1 + i1; divides batches */
    int32_t bias_is_first; /* the bias is the add layer's first input */
    int64_t b_stride[2];   /* what one step of i0 / i1 moves in the bias, in elements */
    int64_t row_stride;    /* ... one query row */
    int64_t key_stride;    /* ... one key */
    float b_scale;         /* the bias */
    int32_t b_zp;
    float sb_scale;        /* the sum: the softmax's input */
    int32_t sb_zp;
    int32_t reserved[4];   /* must be zero */
};

int shl_mi355x_attention_bias(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev, void *out_dev,
                              const struct shl_mi355x_attention_desc *d, const struct shl_mi355x_attention_bias_desc *bd,
                              void *stream);
/* "attention_bias_mfma", or "" for what the call refuses.  Pure host code, touches no device */
const char *shl_mi355x_attention_bias_kernel_name(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev,
                                                  const void *out_dev, const struct shl_mi355x_attention_desc *d,
                                                  const struct shl_mi355x_attention_bias_desc *bd);
/* 1 when the call names a kernel AND the shape belongs to a class in which the biased launch was measured faster than the
 * five launches it replaces (profiles/attention_bias_notes.md: heads of at most 32 on at least 768 keys when the grid is at
 * most 256 workgroups of 32 query rows, and on at most 64 keys when it is at least 3072): what a session fuses without being
 * asked.  Pure host code */
int shl_mi355x_attention_bias_by_default(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev,
                                         const void *out_dev, const struct shl_mi355x_attention_desc *d,
                                         const struct shl_mi355x_attention_bias_desc *bd);
struct shl_mi355x_mul_desc;
/* b_ext1 and the four strides of *bd from the collapsed groups of the add's descriptor `m` (its a the scores
 * [batches][s][t], its b the bias); the other fields of *bd are left alone.  SHL_MI355X_OK, SHL_MI355X_EINVAL when the
 * groups do not describe [batches][s][t], SHL_MI355X_ENOTSUP for a bias that varies in a way i0, i1, row and key cannot
 * express (a group boundary inside the rows or the keys, more than two batch groups).  Pure host code */
int shl_mi355x_attention_bias_geometry(const struct shl_mi355x_mul_desc *m, int32_t batches, int32_t s, int32_t t,
                                       struct shl_mi355x_attention_bias_desc *bd);

/* The same core -- with a bias (bias_dev and bd given) or without (both NULL) -- on operands where the projections left
 * them: a model's q, k and v are [B, S, H D], split into heads by a reshape and a transpose(0,2,1,3) each, and the output is
 * merged again by the inverse pair.  Those eight layers do no arithmetic; this launch reads and writes through strides
 * instead.  `d` (and `bd`) are the descriptors above, unchanged: batches = B H.  For each of q, k, v and out the layout
 * descriptor holds three strides in elements, {outer, head, row}: with the batch index bi = i0 * heads + i1, element
 * (bi, row, col) of an operand is at
 *     base[i0 * outer + i1 * head + row * row_stride + col],
 * the innermost dim (d, d, dv, dv) keeps stride 1.  [B, S, H D] read as [B H][S][D] is {S H D, D, H D} with heads = H; the
 * dense layout is {0, rows * inner, inner} with heads = batches.  Inputs may have any strides that are not negative -- 0, rows
 * that overlap, q, k and v inside one packed [B, S, 3, H, D] projection.  The output's elements must be distinct (its four
 * (extent, stride) pairs, sorted by stride, each stride at least the extent times the stride below it; extents of 1 do not
 * count); gaps between them are allowed and are not written.
 * `moved` (bit 0 q, 1 k, 2 v, 3 out) says which operands replace a chain of shl_mi355x_move / shl_mi355x_transpose.  Those
 * are not the identity in binary16: an infinity arrives as +-65504, every NaN as 0x7FFF with its sign.  Where an input's bit
 * is set the kernel applies that rule to what it loads, so that the launch equals the movers followed by the dense call for
 * any bits; with the bit clear the operand is read raw, and the launch equals the dense call on a copy permuted by the
 * host.  The output's bit changes nothing: a stored half is finite or one of those two NaNs already.  int8 operands are
 * always read raw (a mover whose two records differ requantises: such a layer is not a layout).
 * 16-byte loads serve an operand whose pointer is 16-byte aligned and whose inner extent and strides (those along an extent
 * above 1) are multiples of 16 bytes; every other operand is read by elements.  The kernel, its LDS and its cap on t are shl_mi355x_attention's.
 * SHL_MI355X_EINVAL before anything is enqueued: whatever the descriptor or the bias makes shl_mi355x_attention[_bias] refuse
 * (the dense ranges aside: an operand's range here is that of its strides); a NULL layout descriptor; one of bias_dev and bd
 * NULL and the other not; heads below 1 or not dividing batches; a negative stride; an operand whose largest index is 2^31 or
 * more; moved bits beyond the four; non-zero reserved fields; output elements that overlap each other; the output's range
 * overlapping an operand's or the bias's.  SHL_MI355X_ENOTSUP exactly where shl_mi355x_attention returns it.  Enqueues only:
 * no allocation, no upload, no synchronisation (capturable in a hipGraph). */
#define SHL_MI355X_ATTENTION_LAYOUT_MFMA "attention_layout_mfma"
#define SHL_MI355X_ATTENTION_BIAS_LAYOUT_MFMA "attention_bias_layout_mfma"

struct shl_mi355x_attention_layout_desc {
    int32_t heads; /* the inner extent of the batch index: bi = i0 * heads + i1; divides batches */
    int32_t moved; /* bit 0 q, 1 k, 2 v, 3 out: the operand stands for a chain of movers (binary16: their special-value rule) */
    int32_t q_stride[3], k_stride[3], v_stride[3], out_stride[3]; /* {outer, head, row}, in elements */
    int32_t reserved[2]; /* must be zero */
};

int shl_mi355x_attention_layout(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev, void *out_dev,
                                const struct shl_mi355x_attention_desc *d, const struct shl_mi355x_attention_bias_desc *bd,
                                const struct shl_mi355x_attention_layout_desc *ld, void *stream);
/* "attention_layout_mfma", with a bias "attention_bias_layout_mfma", or "" for what the call refuses.  Pure host code */
const char *shl_mi355x_attention_layout_kernel_name(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev,
                                                    const void *out_dev, const struct shl_mi355x_attention_desc *d,
                                                    const struct shl_mi355x_attention_bias_desc *bd,
                                                    const struct shl_mi355x_attention_layout_desc *ld);
/* 1 when the call names a kernel AND the shape belongs to a class in which one layout launch was measured faster, in int8
 * and in binary16, than the eight mover launches and the core they surround (profiles/attention_layout_notes.md; dv = d:
 * heads of 32 to 64 on 49 to 197 keys from 21 workgroups of 32 query rows on, and heads of at most 32 on at least 768 keys while the grid is at most 256 workgroups
 * of 32 query rows): what a session folds without being asked.  Pure host code */
int shl_mi355x_attention_layout_by_default(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev,
                                           const void *out_dev, const struct shl_mi355x_attention_desc *d,
                                           const struct shl_mi355x_attention_bias_desc *bd,
                                           const struct shl_mi355x_attention_layout_desc *ld);
/* The three strides of the [batches][rows][cols] view that a chain of movers makes of a dense tensor: src_dim[src_rank], then
 * nsteps steps in order.  Step i has step_rank[i] values at step_v + i * SHL_MI355X_MAX_DIM: with step_is_transpose[i] the
 * permutation (output dim k is input dim perm[k]; at most one step may be one), else a reshape's target dims.  swap_last2
 * exchanges the last two dims of the result once more (a K that reaches Q K^T as [..][d][t] and is read without trans_b).  The
 * last two dims are the rows and the columns, the product of the others is *batches; *heads and stride[3] = {outer, head, row}
 * are the layout descriptor's.  For the output, describe the DESTINATION and the chain behind the core inverted.
 * SHL_MI355X_OK; SHL_MI355X_EINVAL for arguments that describe no view; SHL_MI355X_ENOTSUP for a view the strides cannot
 * express (an inner stride other than 1, rows or columns in more than one piece, batch dims in more than two).  Pure host
 * code */
int shl_mi355x_attention_layout_strides(const int32_t *src_dim, int32_t src_rank, int32_t nsteps, const int32_t *step_is_transpose,
                                        const int32_t *step_rank, const int32_t *step_v, int32_t swap_last2, int32_t *batches,
                                        int32_t *rows, int32_t *cols, int32_t *heads, int32_t stride[3]);

/* nearest-neighbour / bilinear resize of a 4-d int8 / binary16 tensor: shl_ref_resize_quant
 * (source/reference/resize.c:464-468), bit for bit.  height_scale / width_scale are the reference's own floats, computed by
 * the CALLER as ONE float division each: (float)in / out, with align_corners (float)(in - 1) / (out - 1)
 * (shl_mi355x_resize_scale, shl_mi355x_backend.h, does it); the source coordinate of output row y is the float product
 * y * height_scale.  Nearest: min((int)floor(.), in - 1), with align_corners (int)round(.); a gather, every element
 * dequantised and requantised -- int8 through `table` (table[(uint8_t)q] = the output byte of input byte q:
 * shl_mi355x_resize_table_i8 builds it; not read when the records are equal and that round trip is the identity),
 * binary16 through the reference's float32 -> binary16 conversion (infinities saturate to +-65504, every NaN becomes
 * 0x7FFF / 0xFFFF).  Bilinear: four taps (y0 = floor(.), y1 = min(y0 + 1, in - 1), the same along x), the products
 * v w_y w_x summed in the reference's order with its build's fused multiply-adds, no tap skipped at weight zero.  f16:
 * scales and zero points are ignored.  Every image of a batch is computed on its own (the reference's NCHW nearest
 * routines are not, resize.c:179).  align_corners with an output extent of 1 and bicubic are refused
 * (SHL_MI355X_EINVAL), and so is an output that overlaps the input.  Enqueues only: no allocation, no upload, no
 * synchronisation (capturable in a hipGraph). */
enum shl_mi355x_resize_mode {
    SHL_MI355X_RESIZE_BILINEAR = 0, /* the values of enum csinn_resize_enum */
    SHL_MI355X_RESIZE_NEAREST = 1,
    SHL_MI355X_RESIZE_BICUBIC = 2 /* refused */
};

struct shl_mi355x_resize_desc {
    int32_t dtype;  /* SHL_MI355X_I8 / SHL_MI355X_F16 */
    int32_t layout; /* SHL_MI355X_NHWC / SHL_MI355X_NCHW */
    int32_t n, c, in_h, in_w, out_h, out_w;
    int32_t mode;          /* shl_mi355x_resize_mode */
    int32_t align_corners; /* 0 / 1 */
    float height_scale, width_scale;
    float in_scale, out_scale;
    int32_t in_zp, out_zp;
    uint8_t table[256];  /* int8 nearest only */
    int32_t reserved[4]; /* must be zero */
};

int shl_mi355x_resize(const void *in_dev, void *out_dev, const struct shl_mi355x_resize_desc *d, void *stream);
/* the kernel form the rules choose: "resize_nhwc_vec" (NHWC, C * element size a multiple of 16, both pointers 16-byte
 * aligned: 16 bytes of a pixel's channels per thread), "resize_nchw_row" (NCHW, the output pointer 4-byte aligned: whole
 * dwords of an output row per thread), "resize_generic" (one output per thread; SHL_MI355X_RESIZE_FORM=generic forces it);
 * "" for invalid arguments.  Pure host code: looks at the pointers' values only, touches no device */
const char *shl_mi355x_resize_kernel_name(const struct shl_mi355x_resize_desc *d, const void *in_dev, const void *out_dev);

/* int8 unary operator by table: out[i] = table[(uint8_t)in[i]].  Serves sigmoid / hard_sigmoid / silu / leaky_relu (and any
 * other int8 -> int8 function of one element): with one quantisation record per tensor the reference's
 * dequantise -> f -> requantise (shl_ref_siso_callback_base, source/reference/utils.c:609-621) has 256 possible results,
 * which the backend computes on the host (shl_mi355x_*_table_i8, shl_mi355x_backend.h).  `table` is HOST memory, 256
 * bytes, read during the call: it travels by value in the kernel arguments (no allocation, nothing to keep alive; a
 * captured graph holds its own copy).  16 bytes per lane when both pointers are 16-byte aligned, one byte per thread
 * otherwise; any count.  Enqueues only. */
int shl_mi355x_unary_lut_i8(const int8_t *input_dev, int8_t *output_dev, size_t count, const uint8_t *table, void *stream);
/* "unary_lut_i8_vec" / "unary_lut_i8_byte": the form those pointers get.  Pure host code */
const char *shl_mi355x_unary_lut_i8_kernel_name(const void *input_dev, const void *output_dev);

/* binary16 unary operators, qinfo scale 1: f16 -> f32, the reference's formula in the reference's precision
 * (source/reference/sigmoid.c:33, hard_sigmoid.c:31-37, silu.c:33, leaky_relu.c:33: double exp, one rounding to float;
 * hard_sigmoid's 0.2 x + 0.5 as the one fused multiply-add the reference's build makes of it),
 * the reference's float -> binary16 rounding.  `alpha`: leaky_relu's slope (params->n), ignored by the others. */
enum shl_mi355x_unary_kind {
    SHL_MI355X_UNARY_SIGMOID = 0,
    SHL_MI355X_UNARY_HARD_SIGMOID = 1,
    SHL_MI355X_UNARY_SILU = 2,
    SHL_MI355X_UNARY_LEAKY_RELU = 3
};
int shl_mi355x_unary_f16(const uint16_t *input_dev, uint16_t *output_dev, size_t count, int32_t kind, float alpha,
                         void *stream);

/* elementwise product with one broadcast operand: shl_ref_mul_quant (source/reference/mul.c:21-40): both operands
 * dequantised, one fp32 product, requantised; bit for bit.  `a` has the output's shape; `b` is broadcast to it by the
 * reference's rule (shl_ref_broadcast_to_shape_f32, utils.c:692-785: ranks right-aligned, every dim of b equals the
 * output's or is 1).  The caller collapses the output's dims to at most 4 groups of neighbouring dims along which b
 * either varies or is broadcast: dim[g] is group g's size (outermost first), b_stride[g] what one step along it moves in
 * b, in elements (0: broadcast).  [N,H,W,C] x [N,1,1,C]: dim {N, H W, C}, b_stride {C, 0, 1}; [N,C,H,W] x [1,C,1,1]:
 * dim {N, C, H W}, b_stride {0, 1, 0}; same shape: dim {count}, b_stride {1}; a scalar: dim {count}, b_stride {0}.
 * f16: scales and zero points are ignored; a NaN comes out as 0x7FFF with the sign x86 gives it.  The output must not
 * overlap an operand.  Enqueues only: no allocation, no
 * upload, no synchronisation (capturable in a hipGraph). */
struct shl_mi355x_mul_desc {
    int32_t dtype;   /* SHL_MI355X_I8 / SHL_MI355X_F16 */
    int32_t ngroups; /* 1 .. 4 */
    int64_t dim[4];
    int64_t b_stride[4];
    float a_scale, b_scale, out_scale;
    int32_t a_zp, b_zp, out_zp;
    int32_t a_is_second; /* a is the layer's SECOND input, b its first (the product commutes; of two binary16 NaNs the
                            reference hands on its second input's) */
    int32_t reserved[4]; /* must be zero */
};

int shl_mi355x_mul(const void *a_dev, const void *b_dev, void *out_dev, const struct shl_mi355x_mul_desc *d, void *stream);
/* the kernel form the rules choose: "mul_vec" (16 bytes per lane: b same-shape, a scalar, or varying only along an
 * unbroadcast innermost group of whole 16-byte pieces; a, out and a non-scalar b 16-byte aligned), "mul_row" (the
 * innermost group is broadcast: one b value per run; a and out 16-byte aligned), "mul_generic" (one output per thread;
 * SHL_MI355X_MUL_FORM=generic forces it); "" for invalid arguments.  Pure host code: looks at the pointers' values only */
const char *shl_mi355x_mul_kernel_name(const struct shl_mi355x_mul_desc *d, const void *a_dev, const void *b_dev,
                                       const void *out_dev);

/* elementwise sum with one broadcast operand: shl_ref_add_quant (source/reference/add.c:21-41) on a layer whose operands
 * differ in shape (a bias [.., N] + [N], an attention mask [B,H,T,T] + [1,H,T,T], a positional embedding): both operands
 * dequantised, one fp32 sum, requantised; bit for bit.  Geometry, descriptor, validation and kernel forms are
 * shl_mi355x_mul's ("add_vec", "add_row", "add_generic"; SHL_MI355X_ADD_FORM=generic forces the last).  a_is_second: a is
 * the layer's second input (the sum commutes; of two binary16 NaNs the reference hands on its second input's, and
 * inf + -inf comes out as 0xFFFF).  f16: scales and zero points are ignored.  Enqueues only: no allocation, no upload, no
 * synchronisation (capturable in a hipGraph).  Two same-shape tensors may equally go through shl_mi355x_add. */
int shl_mi355x_add_bcast(const void *a_dev, const void *b_dev, void *out_dev, const struct shl_mi355x_mul_desc *d, void *stream);
/* the kernel form the rules choose, "" for invalid arguments.  Pure host code: looks at the pointers' values only */
const char *shl_mi355x_add_bcast_kernel_name(const struct shl_mi355x_mul_desc *d, const void *a_dev, const void *b_dev,
                                             const void *out_dev);

/* softmax along one axis of a tensor viewed as [outer, count, inner]:
 * shl_ref_softmax_quant (source/reference/softmax.c:21-72): float max, double exp, float running
 * sum in index order.  count <= 8192. */
int shl_mi355x_softmax(const void *input_dev, void *output_dev, int32_t dtype, int64_t outer, int32_t count,
                       int64_t inner, float in_scale, int32_t in_zp, float out_scale, int32_t out_zp,
                       void *stream);

/* NCHW <-> NHWC re-layout of an activation tensor in HBM (int8: elem_bytes 1, fp16: 2):
 * shl_ref_nchw_to_nhwc_* / shl_ref_nhwc_to_nchw_* of source/reference/utils.c, which the
 * reference's own NCHW convolution uses on non-x86 builds (convolution.c:123-135).
 * `pixels` = H*W.  to_nhwc != 0: [N,C,HW] -> [N,HW,C]; to_nhwc == 0: the inverse. */
int shl_mi355x_layout_convert(const void *src_dev, void *dst_dev, int64_t batch, int32_t channels,
                              int32_t pixels, int32_t elem_bytes, int32_t to_nhwc, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SHL_MI355X_H_ */

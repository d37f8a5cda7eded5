// lut_validate.h -- the host side of a table activation folded into the convolution's launch (shl_mi355x_conv_lut_*, and
// shl_mi355x_dwconv_lut_* for a depthwise layer, at the end): what is
// wrong with a call, which of the two carrying kernel families a forced launch names, and the shape classes a session fuses
// without being asked.  Pure host code that touches no device and includes no HIP header, so that a stand-alone program can
// compile it with the sanitizers (tests/test_act_fuse_cpu.py, tests/test_dw_act_fuse_cpu.py).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "shl_mi355x.h"

namespace shl {

// what the checks need to know of a plan (conv_plan.hip fills it from the plan; a test from numbers)
struct LutPlanFacts {
    int32_t present;  // the plan pointer is not NULL
    int32_t dtype, layout, algo;
    int64_t in_pixels, in_c;    // per image: H * W, C
    int64_t out_pixels, out_c;  // per image: Ho * Wo, Co
    int32_t plan_batch;
};

// SHL_MI355X_OK, or the status of the refusal with its text in *msg.  Nothing is enqueued and no device is touched.  Any 256
// bytes are a table
static inline int lut_validate(const LutPlanFacts *p, const void *in_dev, const void *out_dev, int32_t batch, const uint8_t *table,
                               const char **msg)
{
    *msg = NULL;
    if (!p || !p->present || !in_dev || !out_dev || !table) return *msg = "NULL argument", SHL_MI355X_EINVAL;
    if (p->algo == SHL_MI355X_ALGO_DECONV_GATHER || p->algo == SHL_MI355X_ALGO_DECONV_PHASE)
        return *msg = "the plan is a transposed convolution", SHL_MI355X_ENOTSUP;
    if (p->dtype != SHL_MI355X_I8 || p->layout != SHL_MI355X_NHWC || p->algo != SHL_MI355X_ALGO_IGEMM)
        return *msg = "the plan is not int8 / NHWC / implicit GEMM", SHL_MI355X_ENOTSUP;
    const int64_t n = batch > 0 ? batch : p->plan_batch;
    if (n < 0 || n * p->out_pixels > 0x7FFFFFFFll) return *msg = "the batch gives 2^31 or more output pixels", SHL_MI355X_EINVAL;
    const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)(n * p->out_pixels * p->out_c);
    const uintptr_t i0 = (uintptr_t)in_dev, i1 = i0 + (uintptr_t)(n * p->in_pixels * p->in_c);
    if (o1 < o0 || i1 < i0) return *msg = "a buffer that wraps around the address space", SHL_MI355X_EINVAL;
    if (i0 < o1 && o0 < i1) return *msg = "the output overlaps the input", SHL_MI355X_EINVAL;
    return SHL_MI355X_OK;
}

// SHL_MI355X_ACT_FORM: "wave" | "tile" forces the family of a fused launch, anything else (or unset) leaves the size rule
static inline const char *lut_forced_form(const char *env)
{
    if (env && !strcmp(env, "wave")) return "wave";
    if (env && !strcmp(env, "tile")) return "tile";
    return NULL;
}

// The shape classes a session fuses by default: those where the fused launch was MEASURED faster than conv_forward (in the
// family the plan's rules and tuner pick) followed by unary_lut_i8, by more than the larger of the two run-to-run spreads
// (tools/act_bench.py, profiles/act_fuse_notes.md).
// M = N Ho Wo output pixels, Co output channels, kbytes = bytes of a packed weight row, taps = Kh Kw, strided: a stride above 1,
// tile: the family of the fused launch (else wave).  fused / unfused (the larger of the two spreads):
//   wave, Co >= 64, 196 <= M <= 12544    six shapes at batch 1 -- 3x3 s2 32 -> 64 @160, 1x1 64 -> 64 @80, 3x3 128 -> 128 @40, 1x1
//                                        512 -> 512 @20, 16 -> 96 @112, 112 -> 672 @14: 0.73 - 0.89 (0 - 2 %): in
//   tile, 1x1, Co >= 96, M >= 6272       512 -> 512 @20, 16 -> 96 @112, 112 -> 672 @14 at batch 32: 0.92 (4 %), 0.87 (5 %), 0.78
//                                        (3 %): in
//   tile, 1x1, Co < 96                   64 -> 64 @80 at batch 32: 0.97 inside a spread of 4 % (the unfused chain runs
//                                        conv1x1_stream): out
//   tile, 3x3, stride 2, K rows <= 320   32 -> 64 @160 at batch 32: 0.88 (6 %): in
//   tile, 3x3, anything else             128 -> 128 @40 at batch 32: 1.08 (the row-patch kernel the unfused chain runs beats the
//                                        tile kernel by more than the second launch costs): out
// Nothing else was measured -- fewer than 64 output channels or maps under 196 pixels on the wave kernel, other kernel sizes --
// and stays out.  SHL_MI355X_ACT_FUSE=1 fuses every one the kernel takes
constexpr int64_t LUT_WAVE_MIN_CO = 64, LUT_WAVE_MIN_M = 196, LUT_WAVE_MAX_M = 12544;
constexpr int64_t LUT_TILE_MIN_CO = 96, LUT_TILE_MIN_M = 6272, LUT_TILE_S2_MAX_KBYTES = 320;

static inline bool lut_default(int64_t M, int64_t Co, int64_t kbytes, int64_t taps, bool strided, bool tile)
{
    if (!tile) return (taps == 1 || taps == 9) && Co >= LUT_WAVE_MIN_CO && M >= LUT_WAVE_MIN_M && M <= LUT_WAVE_MAX_M;
    if (M < LUT_TILE_MIN_M) return false;
    if (taps == 1) return Co >= LUT_TILE_MIN_CO;
    return taps == 9 && strided && kbytes <= LUT_TILE_S2_MAX_KBYTES;
}

// ---- the same post-op in the depthwise launch (shl_mi355x_dwconv_lut_*; dwconv.hip, dwconv_mfma.hip)

// the kernel of a depthwise launch, as launch_dwconv picks it
enum { DW_LUT_DOT4 = 0, DW_LUT_MFMA = 1, DW_LUT_NHWC = 2 };

// SHL_MI355X_OK, or the status of the refusal with its text in *msg, as lut_validate; the scope is int8 / NHWC / ALGO_DW (depth
// multiplier 1).  out_w: the output's width; kernel: DW_LUT_* for the call's batch -- the dot4 kernel's grid is (N Ho) rows by
// ceil(Wo C / 4 / 256) blocks, and launch_dwconv refuses a row of more than 65535 blocks
static inline int dw_lut_validate(const LutPlanFacts *p, int64_t out_w, int32_t kernel, const void *in_dev, const void *out_dev,
                                  int32_t batch, const uint8_t *table, const char **msg)
{
    *msg = NULL;
    if (!p || !p->present || !in_dev || !out_dev || !table) return *msg = "NULL argument", SHL_MI355X_EINVAL;
    if (p->algo == SHL_MI355X_ALGO_DECONV_GATHER || p->algo == SHL_MI355X_ALGO_DECONV_PHASE)
        return *msg = "the plan is a transposed convolution", SHL_MI355X_ENOTSUP;
    if (p->dtype != SHL_MI355X_I8 || p->layout != SHL_MI355X_NHWC || p->algo != SHL_MI355X_ALGO_DW || p->in_c != p->out_c)
        return *msg = "the plan is not int8 / NHWC / depthwise", SHL_MI355X_ENOTSUP;
    const int64_t n = batch > 0 ? batch : p->plan_batch;
    if (n < 0 || n * p->out_pixels > 0x7FFFFFFFll) return *msg = "the batch gives 2^31 or more output pixels", SHL_MI355X_EINVAL;
    if (kernel == DW_LUT_DOT4 && (out_w < 0 || (out_w * (p->out_c / 4) + 255) / 256 > 65535))
        return *msg = "an output row of more than 65535 blocks of the dot4 kernel", SHL_MI355X_ENOTSUP;
    const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)(n * p->out_pixels * p->out_c);
    const uintptr_t i0 = (uintptr_t)in_dev, i1 = i0 + (uintptr_t)(n * p->in_pixels * p->in_c);
    if (o1 < o0 || i1 < i0) return *msg = "a buffer that wraps around the address space", SHL_MI355X_EINVAL;
    if (i0 < o1 && o0 < i1) return *msg = "the output overlaps the input", SHL_MI355X_EINVAL;
    return SHL_MI355X_OK;
}

// The shape classes a session fuses by default, by lut_default's criterion: the fused launch MEASURED faster than conv_forward
// followed by unary_lut_i8 on the same build, by more than the larger of the two run-to-run spreads (tools/dw_act_bench.py,
// profiles/dw_act_fuse_notes.md).  M = N Ho Wo output pixels, C channels, taps = Kh Kw, kernel: DW_LUT_*; the class variable is
// E = M C, the bytes the second launch would read and write again.  The depthwise layers in front of a hard-swish / swish in
// MobileNetV3-Large and EfficientNet-B0 at batch 1 and 32, three runs; fused / unfused (the larger of the two spreads):
//   dot4, 36064 <= E <= 1806336       eight 3x3 shapes at batch 1 (49 x 1152 .. 12544 x 32): 0.68 - 0.71 (0 - 3 %; one window of 11 %);
//                                     240 @28 s2, 200 @14, 184 @14, 1152 @7 at batch 32: 0.72 - 0.75 (1 - 3 %): in
//   dot4, E = 14450688                144 @56 at batch 32: 0.83 - 0.84 inside a spread of 13 - 15 %: out
//   mfma, 3010560 <= E <= 12845056    480 @14, 672 @14, 32 @112 at batch 32: 0.77 - 0.81 (2 - 7 %): in
//   nhwc, 5x5, 32928 <= E <= 4214784  seven 5x5 shapes at batch 1: 0.83 - 0.85 (0 - 2 %); 672 @14 s2, 960 @7, 1152 @7, 144 @56 s2,
//                                     480 @14, 672 @14 at batch 32: 0.84 - 0.91 (2 - 6 %): in
//   nhwc, 5x5, E = 6021120            240 @28 at batch 32: 0.93 - 0.94 under spreads of 4 - 6 %, the margin is the spread: out
// Nothing else was measured -- other kernel sizes on the generic kernel, sizes outside the ranges, the matrix-core kernel forced
// onto small maps -- and stays out.  The stride did not tell any two classes apart.  SHL_MI355X_ACT_FUSE=1 fuses every one the
// kernels take
constexpr int64_t DW_LUT_DOT4_MIN_E = 36064, DW_LUT_DOT4_MAX_E = 1806336;
constexpr int64_t DW_LUT_MFMA_MIN_E = 3010560, DW_LUT_MFMA_MAX_E = 12845056;
constexpr int64_t DW_LUT_NHWC_MIN_E = 32928, DW_LUT_NHWC_MAX_E = 4214784;

static inline bool dw_lut_default(int64_t M, int64_t C, int64_t taps, bool strided, int32_t kernel)
{
    (void)strided;
    if (M <= 0 || C <= 0 || M > 0x7FFFFFFFll || C > 0x7FFFFFFFll) return false;
    const int64_t E = M * C;
    if (kernel == DW_LUT_DOT4) return taps == 9 && E >= DW_LUT_DOT4_MIN_E && E <= DW_LUT_DOT4_MAX_E;
    if (kernel == DW_LUT_MFMA) return taps == 9 && E >= DW_LUT_MFMA_MIN_E && E <= DW_LUT_MFMA_MAX_E;
    if (kernel == DW_LUT_NHWC) return taps == 25 && E >= DW_LUT_NHWC_MIN_E && E <= DW_LUT_NHWC_MAX_E;
    return false;
}

}  // namespace shl

// lut_validate.h -- the host side of a table activation folded into the convolution's launch (shl_mi355x_conv_lut_*): what is
// wrong with a call, which of the two carrying kernel families a forced launch names, and the shape classes a session fuses
// without being asked.  Pure host code that touches no device and includes no HIP header, so that a stand-alone program can
// compile it with the sanitizers (tests/test_act_fuse_cpu.py).
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

}  // namespace shl

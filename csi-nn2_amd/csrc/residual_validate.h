// residual_validate.h -- the host side of the fused residual tail (shl_mi355x_conv_add_*): what is wrong with a call and which
// of the two carrying kernel families a forced launch names.  Pure host code that touches no device and includes no HIP
// header, so that a stand-alone program can compile it with the sanitizers (tests/test_residual_cpu.py).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "shl_mi355x.h"

namespace shl {

// what the checks need to know of a plan (conv_plan.hip fills it from the plan; a test from numbers)
struct ResidualPlanFacts {
    int32_t present;  // the plan pointer is not NULL
    int32_t dtype, layout, algo;
    int64_t in_pixels, in_c;    // per image: H * W, C
    int64_t out_pixels, out_c;  // per image: Ho * Wo, Co
    int32_t plan_batch;
};

// SHL_MI355X_OK, or the status of the refusal with its text in *msg.  Nothing is enqueued and no device is touched
static inline int residual_validate(const ResidualPlanFacts *p, const void *in_dev, const void *skip_dev, const void *out_dev,
                                    int32_t batch, const shl_mi355x_residual_desc *d, const char **msg)
{
    *msg = NULL;
    if (!p || !p->present || !in_dev || !skip_dev || !out_dev || !d) return *msg = "NULL argument", SHL_MI355X_EINVAL;
    if (p->algo == SHL_MI355X_ALGO_DECONV_GATHER || p->algo == SHL_MI355X_ALGO_DECONV_PHASE)
        return *msg = "the plan is a transposed convolution", SHL_MI355X_ENOTSUP;
    if (p->dtype != SHL_MI355X_I8 || p->layout != SHL_MI355X_NHWC || p->algo != SHL_MI355X_ALGO_IGEMM)
        return *msg = "the plan is not int8 / NHWC / implicit GEMM", SHL_MI355X_ENOTSUP;
    if (d->act < 0 || d->act > 2) return *msg = "act is none of 0, 1, 2", SHL_MI355X_EINVAL;
    const float scales[3] = {d->skip_scale, d->sum_scale, d->act ? d->out_scale : 1.0f};
    for (int i = 0; i < 3; ++i)
        if (!(scales[i] > 0.0f) || !isfinite(scales[i])) return *msg = "a scale that is no positive finite number", SHL_MI355X_EINVAL;
    const int64_t n = batch > 0 ? batch : p->plan_batch;
    if (n < 0 || n * p->out_pixels > 0x7FFFFFFFll) return *msg = "the batch gives 2^31 or more output pixels", SHL_MI355X_EINVAL;
    const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)(n * p->out_pixels * p->out_c);
    const uintptr_t i0 = (uintptr_t)in_dev, i1 = i0 + (uintptr_t)(n * p->in_pixels * p->in_c);
    const uintptr_t s0 = (uintptr_t)skip_dev, s1 = s0 + (uintptr_t)(n * p->out_pixels * p->out_c);
    if (o1 < o0 || i1 < i0 || s1 < s0) return *msg = "a buffer that wraps around the address space", SHL_MI355X_EINVAL;
    if (i0 < o1 && o0 < i1) return *msg = "the output overlaps the input", SHL_MI355X_EINVAL;
    if (s0 < o1 && o0 < s1) return *msg = "the output overlaps the skip tensor", SHL_MI355X_EINVAL;
    return SHL_MI355X_OK;
}

// The binary16 launch (shl_mi355x_conv_add_f16_*): the same order of refusals on a binary16 / NHWC / implicit-GEMM plan.  Of
// the descriptor only conv_first and act are read -- a binary16 tensor of a fused tail has scale 1, the scale fields are not
// looked at --, byte sizes count 2-byte elements, and the skip pointer must be 2-byte aligned (the kernels read halves)
static inline int residual_f16_validate(const ResidualPlanFacts *p, const void *in_dev, const void *skip_dev, const void *out_dev,
                                        int32_t batch, const shl_mi355x_residual_desc *d, const char **msg)
{
    *msg = NULL;
    if (!p || !p->present || !in_dev || !skip_dev || !out_dev || !d) return *msg = "NULL argument", SHL_MI355X_EINVAL;
    if (p->algo == SHL_MI355X_ALGO_DECONV_GATHER || p->algo == SHL_MI355X_ALGO_DECONV_PHASE)
        return *msg = "the plan is a transposed convolution", SHL_MI355X_ENOTSUP;
    if (p->dtype != SHL_MI355X_F16 || p->layout != SHL_MI355X_NHWC || p->algo != SHL_MI355X_ALGO_IGEMM)
        return *msg = "the plan is not binary16 / NHWC / implicit GEMM", SHL_MI355X_ENOTSUP;
    if (d->act < 0 || d->act > 2) return *msg = "act is none of 0, 1, 2", SHL_MI355X_EINVAL;
    const int64_t n = batch > 0 ? batch : p->plan_batch;
    if (n < 0 || n * p->out_pixels > 0x7FFFFFFFll) return *msg = "the batch gives 2^31 or more output pixels", SHL_MI355X_EINVAL;
    if (((uintptr_t)skip_dev & 1) != 0) return *msg = "the skip tensor is not 2-byte aligned", SHL_MI355X_EINVAL;
    const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)(2 * n * p->out_pixels * p->out_c);
    const uintptr_t i0 = (uintptr_t)in_dev, i1 = i0 + (uintptr_t)(2 * n * p->in_pixels * p->in_c);
    const uintptr_t s0 = (uintptr_t)skip_dev, s1 = s0 + (uintptr_t)(2 * n * p->out_pixels * p->out_c);
    if (o1 < o0 || i1 < i0 || s1 < s0) return *msg = "a buffer that wraps around the address space", SHL_MI355X_EINVAL;
    if (i0 < o1 && o0 < i1) return *msg = "the output overlaps the input", SHL_MI355X_EINVAL;
    if (s0 < o1 && o0 < s1) return *msg = "the output overlaps the skip tensor", SHL_MI355X_EINVAL;
    return SHL_MI355X_OK;
}

// SHL_MI355X_RESIDUAL_FORM: "wave" | "tile" forces the family of a fused launch, anything else (or unset) leaves the size rule
static inline const char *residual_forced_form(const char *env)
{
    if (env && !strcmp(env, "wave")) return "wave";
    if (env && !strcmp(env, "tile")) return "tile";
    return NULL;
}

// The shape classes a session fuses by default: those where the fused launch was MEASURED faster than the launches it
// replaces by more than the run-to-run spread of those launches in the same call (tools/residual_bench.py,
// profiles/residual_notes.md; fused / unfused, spread of the unfused chain).
// M = N Ho Wo output pixels, Co output channels, kbytes = bytes of a packed weight row, taps = Kh Kw, tile: the family of the
// fused launch (else wave).
//   wave, K rows of 256 bytes and more   0.60 - 0.82 on seven shapes (spread 0 - 4 %): in
//   wave, shorter K rows, Co >= 64       64 -> 256 @56 at batch 1: 0.74 (1 %): in
//   wave, shorter K rows, Co < 64        MobileNetV2's 144 -> 24 @56 and 192 -> 32 @28: 0.91 and 0.99, the second within a
//                                        percent of nothing: out
//   tile, 1x1, M >= 25088                256 -> 1024 @14 and 64 -> 256 @56 at batch 128: 0.83 (9 %) and 0.83 (3 %): in
//   tile, 1x1, fewer pixels              512 -> 2048 @7 at batch 128 (M = 6272): 0.95 inside a spread of 10 %: out
//   tile, 3x3                            64 @56 and 512 @7 at batch 128: 0.97 (4 %) and 1.07 (the row-patch kernel the unfused
//                                        chain runs beats the tile kernel by more than the two launches cost): out
// Nothing else was measured and stays out.  SHL_MI355X_RESIDUAL=1 fuses every tail the kernel takes
constexpr int64_t RESIDUAL_WAVE_MIN_KBYTES = 256;
constexpr int64_t RESIDUAL_WAVE_MIN_CO = 64;
constexpr int64_t RESIDUAL_TILE_MIN_M = 25088;

static inline bool residual_default(int64_t M, int64_t Co, int64_t kbytes, int64_t taps, bool tile)
{
    if (tile) return taps == 1 && M >= RESIDUAL_TILE_MIN_M;
    return kbytes >= RESIDUAL_WAVE_MIN_KBYTES || Co >= RESIDUAL_WAVE_MIN_CO;
}

// binary16 (shl_mi355x_conv_add_f16_by_default): the same criterion on the binary16 launches (tools/residual_f16_bench.py,
// profiles/residual_f16_notes.md; fused / unfused, spread of the unfused chain).  kbytes counts 2-byte elements.
//   wave (batch 1), every shape measured   ResNet-50's four expansions 0.74, 0.84 (8 %), 0.65, 0.67; ResNet-18's four 3x3 tails
//                                          0.50 (against the row-patch kernel), 0.76, 0.82, 0.87; MobileNetV2's five projections
//                                          0.77 - 0.82; spreads 0 - 1 % but the one named.  K rows of 128 bytes to 9 KiB, 24
//                                          to 2048 channels, 49 to 3136 pixels: in, from the shortest K row measured
//   tile, 1x1, M >= 100352, Co >= 256      64 -> 256 @56 and 128 -> 512 @28 at batch 128: 0.55 and 0.86 (0 %): in
//   tile, 1x1, fewer pixels                256 -> 1024 @14 and 512 -> 2048 @7 at batch 128: 1.03 and 0.99 (1 %; the unfused
//                                          chain runs the ping-pong kernel): out
//   tile, 1x1, fewer channels              MobileNetV2's five projections at batch 128 (24 - 160 channels): 1.46 - 1.70, the
//                                          tail's conversions on the few waves of a small grid cost more than the add's launch: out
//   tile, 3x3                              ResNet-18's four at batch 128: 1.09 - 1.35 (the row-patch kernel of the unfused chain): out
// Nothing else was measured and stays out.  SHL_MI355X_RESIDUAL=1 fuses every tail the kernel takes
constexpr int64_t RESIDUAL_F16_WAVE_MIN_KBYTES = 128;
constexpr int64_t RESIDUAL_F16_TILE_MIN_M = 100352;
constexpr int64_t RESIDUAL_F16_TILE_MIN_CO = 256;

static inline bool residual_f16_default(int64_t M, int64_t Co, int64_t kbytes, int64_t taps, bool tile)
{
    if (tile) return taps == 1 && M >= RESIDUAL_F16_TILE_MIN_M && Co >= RESIDUAL_F16_TILE_MIN_CO;
    return kbytes >= RESIDUAL_F16_WAVE_MIN_KBYTES;
}

}  // namespace shl

// requant_move.h -- "dequantise, move, requantise" of one element, shared by the kernels that only move data (split.hip,
// shuffle.hip).  The same arithmetic as concat.hip's concat_rq / concat_fix_f16x2:
//   int8      q_out = sat8(rint(((q - zp_in) * s_in) / s_out) + zp_out)     (int8_to_float_base, float_to_int8_base)
//   binary16  float32_to_float16_base(float16_to_float32_base(h)): every finite value and both zeros come back unchanged,
//             +-inf become +-65504 (0x7BFF / 0xFBFF), every NaN becomes 0x7FFF / 0xFFFF by its sign
#pragma once
#include <math.h>

#include "common.h"

namespace shl {

bool requant_is_identity(float s, int32_t zp);  // pool2d.hip

// how an int8 element travels: MOVE_RAW copies the byte (equal records, the round trip proven to be the identity),
// MOVE_FMA divides through div_by_scale (common.h), MOVE_DIV through the hardware's division
enum { MOVE_RAW = 0, MOVE_FMA = 1, MOVE_DIV = 2 };

template <bool FMA>
__device__ __forceinline__ int move_rq(int q, float si, float zi, float so, float zo, float inv_so)
{
    const float x = __fmul_rn(__fsub_rn((float)q, zi), si);  // int8_to_float_base (source/nn2/utils.c:499-502)
    const float d = FMA ? div_by_scale(x, so, inv_so) : __fdiv_rn(x, so);
    return sat8_from_float(__fadd_rn(rintf(d), zo));  // float_to_int8_base (:550-560)
}

template <bool FMA>
__device__ __forceinline__ uint32_t move_rq4(uint32_t w, float si, float zi, float so, float zo, float inv_so)
{
    return pack4_i8(move_rq<FMA>((int8_t)w, si, zi, so, zo, inv_so), move_rq<FMA>((int8_t)(w >> 8), si, zi, so, zo, inv_so),
                    move_rq<FMA>((int8_t)(w >> 16), si, zi, so, zo, inv_so), move_rq<FMA>((int8_t)(w >> 24), si, zi, so, zo, inv_so));
}

// four packed int8 values by `mode`
__device__ __forceinline__ uint32_t move_i8x4(uint32_t w, int mode, float si, float zi, float so, float zo, float inv_so)
{
    if (mode == MOVE_RAW) return w;
    return mode == MOVE_FMA ? move_rq4<true>(w, si, zi, so, zo, inv_so) : move_rq4<false>(w, si, zi, so, zo, inv_so);
}

// two packed binary16 values through float16 -> float32 -> float32_to_float16_base: a half whose magnitude bits reach
// 0x7C00 is an infinity (-> 0x7BFF) or a NaN (-> 0x7FFF), the sign stays; everything below comes back unchanged
__device__ __forceinline__ uint32_t move_fix_f16x2(uint32_t w)
{
    const uint32_t m = w & 0x7FFF7FFFu;
    const uint32_t special = (m + 0x04000400u) & 0x80008000u;  // per half: m >= 0x7C00 (no carry leaves a half)
    if (special == 0u) return w;
    const uint32_t mask = (special >> 15) * 0xFFFFu;
    const uint32_t nan = (((m + 0x03FF03FFu) & 0x80008000u) >> 15) * 0xFFFFu;  // per half: m > 0x7C00
    const uint32_t repl = 0x7BFF7BFFu | (nan & 0x04000400u) | (w & 0x80008000u);
    return (w & ~mask) | (repl & mask);
}

// one dword of either dtype
template <bool F16>
__device__ __forceinline__ uint32_t move_word(uint32_t w, int mode, float si, float zi, float so, float zo, float inv_so)
{
    if constexpr (F16) return move_fix_f16x2(w);
    else return move_i8x4(w, mode, si, zi, so, zo, inv_so);
}

// i / d and i % d of non-negative values: in 32 bits where the caller knows that both fit (`small`, uniform over the
// launch) -- the 64-bit division is a subroutine of some hundred instructions, and these kernels do little else
__device__ __forceinline__ int64_t move_divmod(int64_t i, int64_t d, bool small, int64_t &rem)
{
    if (small) {
        const uint32_t q = (uint32_t)i / (uint32_t)d;
        rem = (int64_t)((uint32_t)i - q * (uint32_t)d);
        return (int64_t)q;
    }
    const int64_t q = i / d;
    rem = i - q * d;
    return q;
}

// div_by_scale(x, so, RN(1 / so)) == x / so for every x = (q - zp) * s this record can produce (common.h; the range
// conv_plan.hip:fma_division_ok admits: 2^-40 <= so <= 2^40, |x| <= 2^60, x finite)
static inline bool move_fma_ok(float s, int32_t zp, float so)
{
    if (!(so >= 0x1p-40f && so <= 0x1p40f)) return false;
    const double bound = (128.0 + fabs((double)zp)) * fabs((double)s);
    return bound <= 0x1p60;  // also NaN
}

}  // namespace shl

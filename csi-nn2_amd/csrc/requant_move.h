// requant_move.h -- "dequantise, move, requantise" of one element, shared by the kernels that only move data (slab.hip,
// shuffle.hip, pad.hip, transpose.hip):
//   int8      q_out = sat8(rint(((q - zp_in) * s_in) / s_out) + zp_out)     (int8_to_float_base, float_to_int8_base)
//   binary16  float32_to_float16_base(float16_to_float32_base(h)): every finite value and both zeros come back unchanged,
//             +-inf become +-65504 (0x7BFF / 0xFBFF), every NaN becomes 0x7FFF / 0xFFFF by its sign
#pragma once
#include <math.h>
#include <string.h>

#include "common.h"

namespace shl {

bool requant_is_identity(float s, int32_t zp);  // pool2d.hip

// how an int8 element travels: MOVE_RAW copies the byte (equal records, the round trip proven to be the identity),
// MOVE_FMA divides through div_by_scale (common.h), MOVE_DIV through the hardware's division
enum { MOVE_RAW = 0, MOVE_FMA = 1, MOVE_DIV = 2 };

// both records of a move and how its int8 elements travel (move_rec() below fills it)
struct MoveRec {
    float si, zi, so, zo, inv_so;
    int32_t mode;
};

template <bool FMA>
__device__ __forceinline__ int move_rq(int q, const MoveRec &r)
{
    const float x = __fmul_rn(__fsub_rn((float)q, r.zi), r.si);  // int8_to_float_base (source/nn2/utils.c:499-502)
    const float d = FMA ? div_by_scale(x, r.so, r.inv_so) : __fdiv_rn(x, r.so);
    return sat8_from_float(__fadd_rn(rintf(d), r.zo));  // float_to_int8_base (:550-560)
}

template <bool FMA>
__device__ __forceinline__ uint32_t move_rq4(uint32_t w, const MoveRec &r)
{
    return pack4_i8(move_rq<FMA>((int8_t)w, r), move_rq<FMA>((int8_t)(w >> 8), r), move_rq<FMA>((int8_t)(w >> 16), r),
                    move_rq<FMA>((int8_t)(w >> 24), r));
}

// four packed int8 values by the record's mode
__device__ __forceinline__ uint32_t move_i8x4(uint32_t w, const MoveRec &r)
{
    if (r.mode == MOVE_RAW) return w;
    return r.mode == MOVE_FMA ? move_rq4<true>(w, r) : move_rq4<false>(w, r);
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
__device__ __forceinline__ uint32_t move_word(uint32_t w, const MoveRec &r)
{
    if constexpr (F16) return move_fix_f16x2(w);
    else return move_i8x4(w, r);
}

// a piece of 16 or of 4 bytes
template <typename W, bool F16>
__device__ __forceinline__ W move_piece(W v, const MoveRec &r)
{
    if constexpr (sizeof(W) == 16) {
        v.x = move_word<F16>(v.x, r), v.y = move_word<F16>(v.y, r), v.z = move_word<F16>(v.z, r), v.w = move_word<F16>(v.w, r);
        return v;
    } else {
        return move_word<F16>(v, r);
    }
}

// one element by the record's mode, in the low bits
template <bool F16>
__device__ __forceinline__ uint32_t move_elem(uint32_t v, const MoveRec &r)
{
    if constexpr (F16) {
        return move_fix_f16x2(v & 0xFFFFu);
    } else {
        if (r.mode == MOVE_RAW) return v & 0xFFu;
        const int q = (int8_t)v;
        return (uint32_t)(r.mode == MOVE_FMA ? move_rq<true>(q, r) : move_rq<false>(q, r)) & 0xFFu;
    }
}

// one element by the literal formula, whatever the mode
template <bool F16>
__device__ __forceinline__ uint32_t move_literal(uint32_t v, const MoveRec &r)
{
    if constexpr (F16) return float_to_f16_bits_ref(f16_bits_to_float((uint16_t)v));
    else return (uint32_t)move_rq<false>((int8_t)v, r) & 0xFFu;
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
    return fma_div_ok((128.0 + fabs((double)zp)) * fabs((double)s), so);
}

// The one rule for how an int8 element travels.  may_copy: the form moves bytes it need not look at (the literal forms
// never do); the identity is only asked about records that compare equal
static inline MoveRec move_rec(float in_scale, int32_t in_zp, float out_scale, int32_t out_zp, bool may_copy)
{
    MoveRec r;
    r.si = in_scale, r.zi = (float)in_zp;
    r.so = out_scale, r.zo = (float)out_zp, r.inv_so = 1.0f / out_scale;
    if (may_copy && in_zp == out_zp && memcmp(&in_scale, &out_scale, sizeof(float)) == 0 && requant_is_identity(in_scale, in_zp))
        r.mode = MOVE_RAW;
    else r.mode = move_fma_ok(in_scale, in_zp, out_scale) ? MOVE_FMA : MOVE_DIV;
    return r;
}

// ---- host idioms of the movers ------------------------------------------------------------------------------
// do the half-open byte ranges [a, a + an) and [b, b + bn) share a byte?  (an empty range shares none)
static inline bool ranges_overlap(const void *a, int64_t an, const void *b, int64_t bn)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)an, b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)bn;
    return a0 < a1 && b0 < b1 && a0 < b1 && b0 < a1;
}

// true, with the error set, when a launch of `groups` workgroups would not fit the grid
static inline bool grid_refused(const char *op, int64_t groups)
{
    if (groups <= 0x7FFFFFFFll) return false;
    set_error("%s: %lld workgroups exceed the grid", op, (long long)groups);
    return true;
}

}  // namespace shl

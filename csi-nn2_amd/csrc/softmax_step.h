// softmax_step.h -- the steps of softmax (shl_ref_softmax_f32, source/reference/softmax.c:21-66, inside
// shl_ref_siso_callback_base) for the two places that compute it: softmax_kernel (pool_softmax.hip) and the softmax phase of the
// fused attention kernel (attention.hip): the dequantising load and requantising store, the exponential of one element and the
// reference's float running sum as a one-wave scan.  One definition, so that the fused launch equals shl_mi355x_softmax by
// construction.
#pragma once
#include <math.h>

#include "common.h"

namespace shl {

// int8_to_float_base (source/nn2/utils.c:499-502)
__device__ __forceinline__ float dequant_i8(int q, float zi, float si) { return __fmul_rn(__fsub_rn((float)q, zi), si); }

// float_to_int8_base (source/nn2/utils.c:550-560)
__device__ __forceinline__ int requant_i8(float v, float so, float zo) { return sat8_from_float(__fadd_rn(rintf(__fdiv_rn(v, so)), zo)); }

__device__ __forceinline__ float load_dequant(const void *in, int64_t idx, int dtype, float si, float zi)
{
    if (dtype == SHL_MI355X_I8) return dequant_i8(static_cast<const int8_t *>(in)[idx], zi, si);
    return f16_bits_to_float(static_cast<const uint16_t *>(in)[idx]);
}

__device__ __forceinline__ void store_requant(void *out, int64_t idx, float v, int dtype, float so, float zo)
{
    if (dtype == SHL_MI355X_I8) static_cast<int8_t *>(out)[idx] = (int8_t)requant_i8(v, so, zo);
    else static_cast<uint16_t *>(out)[idx] = float_to_f16_bits_ref(v);
}

// one element's term of the sum: exp(double(x - max)), the difference in float (softmax.c:44)
__device__ __forceinline__ double softmax_exp(float x, float m) { return exp((double)__fsub_rn(x, m)); }

// The reference's running sum  acc = (float)((double)acc + e[j]),  j = 0 .. cnt-1  (softmax.c:21-66) is a
// chain of three dependent double-precision instructions per element: ~15 us for 1 000 classes on one lane.
// It is nevertheless NOT inherently sequential.  While acc stays inside one binade [2^E, 2^(E+1)) it is
// m * u with u = 2^(E-23) and an integer m in [2^23, 2^24), and one step is
//     d    = RN_double(m u + e)         the sum stays in the binade, where doubles are spaced u * 2^-29:
//                                       d / u = m + t'  with  t' = RN_{2^-29}(e / u)  -- m is an integer, so
//                                       t' (ties included: m * 2^29 is even) does not depend on m
//     acc' = RN_float(d) = (m + rint(t')) u            unless t' is exactly half-way (then m's parity decides)
// so the integer increments k_j = rint(t'_j) of a whole block of elements are independent of each other and
// the block advances by their prefix sum.  A wave evaluates 64 elements per round (t' = ((2^E + e) - 2^E) / u
// in double arithmetic, exact), scans the increments and stops at the first element that either is a tie
// or would carry acc out of the binade (m + prefix >= 2^24, conservatively); that element takes the literal
// step and the next round starts from the new acc (and binade).  Bit-identical to the literal loop:
// tests/test_tail_sweeps.py feeds both forms crafted terms (tests/softmax_sum_cases.py: ties, binade exits,
// inf / NaN, a subnormal sum) through shl_mi355x_debug_running_sum and compares each with a numpy loop;
// tests/test_softmax_scan.py compares the two forms' softmax outputs.
__device__ __forceinline__ double readlane_f64(double x, int l)  // (l wave-uniform)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

// Round 6: the same scheme in INTEGER arithmetic, four consecutive elements per lane and round (256 per round).  A round is one
// wave's chain of dependent instructions, and in double precision (ldexp, floor, rint, compares: ~10 f64 instructions per element at
// a quarter of the fp32 rate) it cost ~520 cycles -- 19 rounds = 9 850 of the kernel's 16 000 ticks for 1 000 classes
// (tools/dev/r06_sm_trace.sh).  With x = RN_double(2^E + e):
//   * x's exponent field is still E's  <=>  e did not carry the sum out of the binade ("big" above);
//   * x's 52 mantissa bits ARE (x - 2^E) / 2^(E-52) = t' * 2^29: integer part = bits 29 .. 51, fraction = bits 0 .. 28 --
//     rint(t') = integer part + (fraction > 2^28), a tie is fraction == 2^28 (it stops the round: the rounding of a tie is never used);
//   * m is acc's own significand (float bits), and acc' = (m + prefix) * 2^(E-23) is assembled from bits as well.
// One f64 addition per element is all the floating point left in a round.
// (`e` is padded with 256 zeros behind its cnt elements: a zero adds nothing and never stops a round, so no lane tests validity.
// A tie or an element that leaves the binade simply takes the increment 2^24, which trips the one stop criterion m + prefix >= 2^24
// at exactly that element.  What a round costs is its INSTRUCTION COUNT -- one wave issues an instruction per ~5.8 cycles,
// scalar or vector -- hence the shape of this loop.)
__device__ __forceinline__ float running_sum_exact(const double *e, int cnt, int lane)
{
    float acc = 0.f;  // wave-uniform
    int j = 0;
    while (j < cnt) {
        const uint32_t abits = __float_as_uint(acc);
        const uint32_t aexp = abits >> 23;  // (sign included: a negative acc does not exist, NaN / inf take the literal path)
        if (aexp == 0u || aexp >= 0xffu) {   // zero, subnormal (or not a positive finite number): literal step
            acc = (float)((double)acc + e[j]);
            ++j;
            continue;
        }
        const uint32_t m = (abits & 0x007fffffu) | 0x00800000u;  // acc = m * 2^(E-23), E = aexp - 127
        const uint32_t base_hi = (aexp + (1023u - 127u)) << 20;  // the double 2^E (low word 0)
        const double base = __hiloint2double((int)base_hi, 0);
        const uint32_t limit = 0x01000000u - m;                  // the round stops at the first prefix >= limit
        const double *ep = e + j + 4 * lane;
        double ev[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) ev[k] = ep[k];
        uint32_t P[4];  // inclusive prefix of the increments inside the lane, saturated at 2^24 (every prefix in front of the
                        // first stop is < 2^24 and exact)
        uint32_t s4 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double x = base + ev[k];
            const uint32_t hi = (uint32_t)__double2hiint(x), lo = (uint32_t)__double2loint(x);
            const uint32_t frac = lo & 0x1fffffffu;
            const uint32_t ip = ((hi << 3) | (lo >> 29)) & 0x007fffffu;
            // exponent (or sign) field moved: >= 2^(E+1), inf or NaN; fraction exactly one half: a tie
            const bool stop = ((hi ^ base_hi) > 0x000fffffu) || frac == 0x10000000u;
            // (branch-free on purpose: hipcc otherwise wraps the three instructions of the regular case in an exec-mask branch)
            const uint32_t inc = ip + (frac > 0x10000000u ? 1u : 0u) + (stop ? 0x01000000u : 0u);
            s4 = min(s4 + inc, 0x01000000u);
            P[k] = s4;
        }
        // inclusive prefix sum of the lanes' totals over the wave (<= 64 * 2^24: no overflow in 32 bits), on DPP:
        // row_shr 1, 2, 4, 8 scan the 16-lane rows, row_bcast15 / row_bcast31 carry the row totals
        uint32_t p = s4;
        p += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p, 0x111, 0xf, 0xf, true);
        p += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p, 0x112, 0xf, 0xf, true);
        p += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p, 0x114, 0xf, 0xf, true);
        p += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p, 0x118, 0xf, 0xf, true);
        p += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p, 0x142, 0xa, 0xf, false);
        p += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p, 0x143, 0xc, 0xf, false);
        const uint32_t before = p - s4;                                   // the lanes in front of this one
        const uint32_t room = limit > before ? limit - before : 0u;       // what this lane's prefixes may reach
        // the lane's elements in front of its first stop (the prefixes are non-decreasing) and the prefix of the last of them
        int fk = 0;
        uint32_t last = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in_front = P[k] < room;
            fk += in_front ? 1 : 0;
            last = in_front ? P[k] : last;
        }
        const uint32_t reach = before + last;  // the sum's increment up to the lane's last element in front of its stop
        const unsigned long long mask = __ballot(fk < 4);
        int nvalid = cnt - j;
        nvalid = nvalid < 256 ? nvalid : 256;
        int c = 256;
        uint32_t pc;
        if (mask) {
            const int L = __builtin_ctzll(mask);
            c = 4 * L + __builtin_amdgcn_readlane(fk, L);
            pc = (uint32_t)__builtin_amdgcn_readlane((int)reach, L);
        } else {
            pc = (uint32_t)__builtin_amdgcn_readlane((int)p, 63);  // (the zeros behind the row add nothing)
        }
        if (c > nvalid) c = nvalid;  // (a stop never sits on a zero behind the row: pc is the row's increment then as well)
        if (c > 0) {  // elements j .. j + c - 1 advance acc inside its binade (c is wave-uniform)
            acc = __uint_as_float((aexp << 23) | ((m + pc) & 0x007fffffu));  // (m + pc) * 2^(E-23), 2^23 <= m + pc < 2^24
            j += c;
        }
        if (c < nvalid) {  // the stopping element: literal step (may change the binade); its value sits in lane c / 4
            const int ks = c & 3;
            const double es = readlane_f64(ks == 0 ? ev[0] : ks == 1 ? ev[1] : ks == 2 ? ev[2] : ev[3], c >> 2);
            acc = (float)((double)acc + es);
            ++j;
        }
    }
    return acc;
}

}  // namespace shl

// matmul_step.h -- the pieces of the matmul kernels (matmul.hip) that the fused attention kernel (attention.hip) runs as well:
// the mfma form's tile constants, the 16-byte slab pieces and their LDS image, and the store -- mm_value is the element the
// plain kernel stores for a float32 sum: the int8 byte under the output's record, the rounded half with the NaN rule.  One
// definition, so that a product computed inside another launch equals shl_mi355x_matmul's by construction.
#pragma once
#include <type_traits>

#include "add_step.h"
#include "igemm_common.h"

namespace shl {

constexpr int MM_T = 64;      // tile rows and columns
constexpr int MM_KB = 64;     // bytes of k per slab and row
constexpr int MM_PITCH = 80;  // bytes per LDS row

struct MmArgs {
    const void *a, *b;
    void *out;
    int32_t batches, M, N, K;
    int64_t abs, ars, aks, bbs, brs, bks;  // strides in elements
    int32_t a_kc, b_kc, a_vec, b_vec;
    int32_t iza, izb, div_fma, tiles_m, tiles_n;
    float sa, za, sb, zb, so, zo, inv_so, mult;  // so, zo: the record the product is stored under (BIAS: the intermediate's)
    // BIAS only: the bias (N elements), the add's records (a: the intermediate, b: the bias) and whether the bias is the add
    // layer's first input
    const void *bias;
    AddRec add;
    int32_t bias_first;
};

template <bool F16>
__device__ __forceinline__ uint32_t mm_load(const void *p, int64_t at)
{
    if constexpr (F16) return static_cast<const uint16_t *>(p)[at];
    else return static_cast<const uint8_t *>(p)[at];
}

// what the plain kernel stores for the sum f under the record (so, zo): binary16 the rounded half, a NaN as 0x7FFF with its
// sign; int8 sat8(rint(f / so) + zo) (float_to_int8_base), the division through div_by_scale where the plan admits it
template <bool F16>
__device__ __forceinline__ int mm_value(float f, float so, float zo, float inv_so, int div_fma)
{
    if constexpr (F16) {
        return f != f ? ((__float_as_uint(f) >> 31) ? 0xFFFF : 0x7FFF) : (int)float_to_f16_bits_ref(f);
    } else {
        const float d = div_fma ? div_by_scale(f, so, inv_so) : __fdiv_rn(f, so);
        return sat8_from_float(__fadd_rn(rintf(d), zo));
    }
}

// braw: the raw bias element of the output's column (BIAS only).  The kernels fetch it BEFORE their K loop: a lane's outputs
// share one column, and a load issued between the stores would have to wait for each of them (the pointers may alias)
template <bool F16, bool BIAS = false>
__device__ __forceinline__ void mm_store(const MmArgs &a, int64_t o, float f, uint32_t braw = 0)
{
    if constexpr (F16) {
        const uint16_t h = (uint16_t)mm_value<true>(f, a.so, a.zo, a.inv_so, a.div_fma);
        if constexpr (BIAS) {
            const uint16_t hb = (uint16_t)braw;
            static_cast<uint16_t *>(a.out)[o] = a.bias_first ? add_f16_step(hb, h) : add_f16_step(h, hb);
        } else {
            static_cast<uint16_t *>(a.out)[o] = h;
        }
    } else {
        const int q = mm_value<false>(f, a.so, a.zo, a.inv_so, a.div_fma);
        if constexpr (BIAS) static_cast<int8_t *>(a.out)[o] = (int8_t)add_i8_step(q, (int8_t)braw, a.add);
        else static_cast<int8_t *>(a.out)[o] = (int8_t)q;
    }
}

// ---- the mfma form ---------------------------------------------------------------------------------------------------------
// One thread's 16-byte piece of a slab.  base: the operand's first element of this batch; `os` the stride of the dimension the
// piece does not walk.  kc: the piece walks k (thread t: row t / 4, piece t % 4 of the row's 64 bytes); else it walks the
// tile's rows (k = t / PPK of the slab, rows 16 / ES (t % PPK) on).  Elements outside the operand come back as zeros
template <bool F16>
__device__ __forceinline__ uint4 mm_piece(const void *base, int64_t os, int row0, int rows, int k0, int K, int kc, int vec, int tid)
{
    using E = typename std::conditional<F16, uint16_t, uint8_t>::type;
    constexpr int ES = (int)sizeof(E), EPP = 16 / ES, PPK = MM_T / EPP;
    const E *p = static_cast<const E *>(base);
    const int outer = kc ? row0 + (tid >> 2) : k0 + tid / PPK;   // the coordinate the piece does not walk
    const int outer_end = kc ? rows : K;
    const int first = kc ? k0 + (tid & 3) * EPP : row0 + (tid % PPK) * EPP;  // the piece's first coordinate along its walk
    const int end = kc ? K : rows;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (outer >= outer_end || first >= end) return v;
    const E *src = p + (int64_t)outer * os + first;
    if (vec && first + EPP <= end) return *reinterpret_cast<const uint4 *>(src);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < EPP; ++e)
        if (first + e < end) w[e * ES / 4] |= (uint32_t)src[e] << (8 * (e * ES % 4));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// ... and its place in the LDS image [row][k]
template <bool F16>
__device__ __forceinline__ void mm_put(char *lds, const uint4 &v, int kc, int tid)
{
    using E = typename std::conditional<F16, uint16_t, uint8_t>::type;
    constexpr int ES = (int)sizeof(E), EPP = 16 / ES, PPK = MM_T / EPP;
    if (kc) {
        *reinterpret_cast<uint4 *>(lds + (tid >> 2) * MM_PITCH + (tid & 3) * 16) = v;
        return;
    }
    const int kk = tid / PPK, r0 = (tid % PPK) * EPP;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < EPP; ++e)
        *reinterpret_cast<E *>(lds + (r0 + e) * MM_PITCH + kk * ES) = (E)(w[e * ES / 4] >> (8 * (e * ES % 4)));
}

}  // namespace shl

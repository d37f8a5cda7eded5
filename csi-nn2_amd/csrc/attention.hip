// attention.hip -- the core of an attention block as ONE launch: scores = Q K^T, [scores * constant], softmax over the keys,
// P V (shl_mi355x_attention; a session's STEP_ATTENTION).  Unfused that is four launches, and three intermediates -- the
// [batches][S][T] scores twice, the probabilities once -- make a round trip through HBM.
//
// The launch equals shl_mi355x_matmul (mfma form) -> shl_mi355x_mul -> shl_mi355x_softmax -> shl_mi355x_matmul (mfma form) bit
// for bit, by construction: every intermediate is computed exactly as the unfused kernel would STORE it -- the int8 byte under
// its record, the rounded half with the NaN rule --, is kept in LDS and goes through the next layer's own element function:
//   products  matmul_mfma's instructions on its fragment layout (matmul_step.h: 16 bytes of k per lane, [row][k] images with
//             a zero-filled K tail, k ascending in 64-byte slabs into one accumulator), int8 on the raw bytes with the same
//             correction by row and column sums, then mm_value.  That fixes the float32 summation order of binary16 as well
//   multiply  mul_i8_one / mul_f16_one (mul_step.h) on the value the first product would have stored
//   add       (shl_mi355x_attention_bias, the BIAS instantiations: a bias or mask between the multiply and the softmax, which a
//             session's planner finds as a broadcasting add) add_i8_step / add_f16_step (add_step.h) on the value the multiply
//             -- or the first product -- would have stored and the bias element, read from global memory by the descriptor's
//             strides; the sum goes into the tile under its own record, which is the one the softmax then reads.  That launch
//             equals matmul -> [mul] -> shl_mi355x_add_bcast -> softmax -> matmul
//   softmax   a row per wave.  The max is order-free, every element's exp(double(x - max)) is the same operation on the same
//             operands (softmax_step.h), running_sum_exact is a one-wave routine over an LDS row padded with 256 zeros.  int8
//             rows longer than 256 take the exponential and the requantised quotient from a per-row table of 256, as
//             softmax_kernel does for every row: the same operations on the same operands, four f64 exp and divisions per lane
//             and row instead of T / 64
// A workgroup owns 32 query rows of one batch.  Its first four waves run the products; the softmax's f64 work is what a
// small grid waits for, so there a workgroup brings four or twelve more waves for it (attention_canon.h:att_waves: 16, 8 or
// 4 waves, as the grid and the LDS allow).  Q K^T: a pass covers 128 keys, a wave one 32 x 32 block of them;
// the 32 x T tile of scores is written to LDS through mm_value + the mul step.  The probabilities overwrite the scores in
// place, and P V reads them as its [row][k] operand directly; v goes through mm_put's transposing write, a pass covers 128
// output columns.  LDS (attention_canon.h:att_lds) caps T at SHL_MI355X_ATTENTION_MAX_KEYS; d and dv are looped over.
//
// The LAYOUT instantiations (shl_mi355x_attention_layout) take the operands where a model's projections left them -- q, k, v
// inside [B, S, H d], the output into one -- instead of behind a reshape and a transpose(0,2,1,3) each: per operand three
// element strides {outer, head, row} and `heads`, the batch index bi = i0 heads + i1, the base i0 outer + i1 head computed
// once per workgroup in scalar registers, mm_piece given the row stride where the dense form gives d / dv, the store's index
// base + row out_row + col.  The innermost dim keeps stride 1.  That launch equals the movers (shl_mi355x_move,
// shl_mi355x_transpose) around the dense launch bit for bit: int8 movers under one record copy bytes; binary16 movers turn an
// infinity into +-65504 and a NaN into 0x7FFF with its sign (requant_move.h:move_fix_f16x2), which the kernel applies to the
// pieces of an input whose `moved` bit is set.  The dense instantiations take their old argument blocks and keep their
// registers (profiles/attention_layout_notes.md); every combination of dtype, bias and layout compiles without a spill, so
// none is refused for its registers.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "add_step.h"
#include "attention_canon.h"  // the host side: validation, the form rule, the LDS layout (a stand-alone program compiles it too)
#include "matmul_step.h"
#include "mul_step.h"
#include "requant_move.h"
#include "softmax_step.h"

namespace shl {

struct AttArgs {
    const void *q, *k, *v;
    void *out;
    int32_t batches, S, T, D, DV, tiles;  // tiles: row tiles per batch
    int32_t q_vec, k_vec, v_vec;
    AttLds lds;
    // Q K^T: the raw-byte correction's zero points, mult = fl(q_scale k_scale), the record the scores are stored under
    int32_t izq, izk, s_div;
    float mult1, s_so, s_zo, s_inv;
    // the multiply by the constant craw (its raw element)
    int32_t has_scale, craw;
    MulRec mul;
    // softmax: the record it reads (the scaled scores', else the scores') and the probabilities'
    float x_si, x_zi, p_so, p_zo;
    // P V
    int32_t izp, izv, o_div;
    float mult2, o_so, o_zo, o_inv;
};

// the biased launch's further arguments (shl_mi355x_attention_bias).  A kernel without the bias takes AttArgs alone: its
// arguments, and with them its instructions, are what they were before the bias existed
struct AttBiasArgs : AttArgs {
    const void *bias;
    int32_t b_ext1, b_stride0, b_stride1, row_stride, key_stride;  // in elements; validated: every index fits 31 bits
    int32_t bias_first;                                            // the bias is the add layer's first input
    AddRec add;                                                    // a the (scaled) scores, b the bias, the sum's record
};

// the layout launch's further arguments (shl_mi355x_attention_layout), appended to either struct as AttBiasArgs' are to AttArgs:
// a kernel without them takes what it took before the layout form existed.  Strides in elements; validated: every index an
// operand forms fits 31 bits
struct AttLayoutPart {
    int32_t heads, moved;  // bi = i0 * heads + i1; moved: ATT_MOVED_* (binary16: the movers' rule for special values on what is loaded)
    int32_t q_outer, q_head, q_row, k_outer, k_head, k_row, v_outer, v_head, v_row, o_outer, o_head, o_row;
};
struct AttLayoutArgs : AttArgs {
    AttLayoutPart lay;
};
struct AttBiasLayoutArgs : AttBiasArgs {
    AttLayoutPart lay;
};
template <bool BIAS, bool LAYOUT>
using AttArgsOf = typename std::conditional<LAYOUT, typename std::conditional<BIAS, AttBiasLayoutArgs, AttLayoutArgs>::type,
                                            typename std::conditional<BIAS, AttBiasArgs, AttArgs>::type>::type;

// a piece as the movers would have delivered it (requant_move.h: an infinity as +-65504, a NaN as 0x7FFF with its sign; idempotent,
// so once stands for a reshape and a transpose; the zeros of a piece's tail stay zeros)
__device__ __forceinline__ uint4 att_moved(uint4 v)
{
    v.x = move_fix_f16x2(v.x), v.y = move_fix_f16x2(v.y), v.z = move_fix_f16x2(v.z), v.w = move_fix_f16x2(v.w);
    return v;
}

// a wave's LDS writes are visible to its own later reads (the LDS serves one wave's instructions in order); this keeps the
// compiler from moving either across the point
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The lane's sixteen bias elements for its block of scores.  C/D layout: a lane holds one key and sixteen rows; for a fixed r 32
// adjacent lanes read 32 adjacent keys of one row -- coalesced where key_stride is 1, one address where it is 0.  The batch's
// and the tile's part of the index is the same for the whole wave and stays in scalar registers; a lane adds 32-bit offsets
// (validated: every index fits 31 bits).  A key past the last one and a row past the last query load nothing
template <typename E>
__device__ __forceinline__ void att_bias_load(E (&bv)[16], const AttBiasArgs &a, uint32_t bi, int m0, int key, int fh, bool active)
{
    const uint32_t i0 = bi / (uint32_t)a.b_ext1, i1 = bi - i0 * (uint32_t)a.b_ext1;
    const E *const pb = static_cast<const E *>(a.bias) +
                        (i0 * (uint32_t)a.b_stride0 + i1 * (uint32_t)a.b_stride1 + (uint32_t)m0 * (uint32_t)a.row_stride);
    const bool in = active && key < a.T;
    const uint32_t lane_off = (uint32_t)(in ? key : 0) * (uint32_t)a.key_stride + (uint32_t)(4 * fh) * (uint32_t)a.row_stride;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2);
        bv[r] = in && m0 + row + 4 * fh < a.S ? pb[lane_off + (uint32_t)row * (uint32_t)a.row_stride] : (E)0;
    }
}

// Where the biased kernel asks for the bias (profiles/attention_bias_notes.md).  binary16: EARLY, in front of the K loop, so
// that the store behind the loop does not wait for it: measured 1 to 3 % faster than asking at the store (128 VGPRs, no
// spill).  int8: at the head of the store, in front of the row sums' exchange -- sixteen more values across the loop spill
// there (the kernel's scalar registers already overflow into vector ones).  -DATT_BIAS_EARLY=0 builds the late binary16 form
#ifndef ATT_BIAS_EARLY
#define ATT_BIAS_EARLY 1
#endif

template <bool F16, bool BIAS, bool LAYOUT>
__global__ __launch_bounds__(1024) void attention_mfma_kernel(AttArgsOf<BIAS, LAYOUT> a)
{
    using Acc = typename AccT<!F16>::type;
    using E = typename std::conditional<F16, uint16_t, uint8_t>::type;
    constexpr int ES = F16 ? 2 : 1, KS = MM_KB / ES;  // elements of k per slab
    [[maybe_unused]] constexpr bool BIAS_EARLY = F16 && ATT_BIAS_EARLY;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, fr = lane & 31, fh = lane >> 5;
    const int nw = (int)blockDim.x >> 6;  // 4, 8 or 16 waves: the first four run the products, all of them the softmax
    const bool mover = tid < 256;         // (wave-uniform) the threads that load slabs and hold fragments
    const int T = a.T, tp = a.lds.tile_pitch;
    double *const e = reinterpret_cast<double *>(smem + a.lds.e) + wave * (T + 256);  // the wave's row of terms, 256 zeros behind
    char *const tile = smem + a.lds.tile;
    char *const lds_q = smem + a.lds.slab_q;
    char *const lds_kv = smem + a.lds.slab_kv;
    int32_t(*const row_sum)[32] = reinterpret_cast<int32_t(*)[32]>(smem + a.lds.row_sum);
    const uint32_t bi = blockIdx.x / (uint32_t)a.tiles;
    const int m0 = (int)(blockIdx.x - bi * (uint32_t)a.tiles) * ATT_ROWS;
    // (every tensor holds fewer than 2^31 elements)
    const void *pq, *pk, *pv;
    int q_row, k_row, v_row;  // the stride of the dimension a piece does not walk
    [[maybe_unused]] bool fix_q = false, fix_k = false, fix_v = false;
    [[maybe_unused]] uint32_t o_base = 0;
    if constexpr (LAYOUT) {
        // (wave-uniform, in scalar registers; validated: every operand's largest index fits 31 bits)
        const uint32_t i0 = bi / (uint32_t)a.lay.heads, i1 = bi - i0 * (uint32_t)a.lay.heads;
        pq = static_cast<const E *>(a.q) + (i0 * (uint32_t)a.lay.q_outer + i1 * (uint32_t)a.lay.q_head);
        pk = static_cast<const E *>(a.k) + (i0 * (uint32_t)a.lay.k_outer + i1 * (uint32_t)a.lay.k_head);
        pv = static_cast<const E *>(a.v) + (i0 * (uint32_t)a.lay.v_outer + i1 * (uint32_t)a.lay.v_head);
        o_base = i0 * (uint32_t)a.lay.o_outer + i1 * (uint32_t)a.lay.o_head;
        q_row = a.lay.q_row, k_row = a.lay.k_row, v_row = a.lay.v_row;
        if constexpr (F16) {
            fix_q = a.lay.moved & ATT_MOVED_Q, fix_k = a.lay.moved & ATT_MOVED_K, fix_v = a.lay.moved & ATT_MOVED_V;
        }
    } else {
        pq = static_cast<const char *>(a.q) + (int64_t)bi * a.S * a.D * ES;
        pk = static_cast<const char *>(a.k) + (int64_t)bi * T * a.D * ES;
        pv = static_cast<const char *>(a.v) + (int64_t)bi * T * a.DV * ES;
        q_row = a.D, k_row = a.D, v_row = a.DV;
    }

    // ---- scores = Q K^T, stored as matmul_mfma stores them, then the multiply -------------------------------------------------
    for (int n0 = 0; n0 < T; n0 += ATT_KEYS) {
        const bool active = mover && n0 + wave * 32 < T;  // (wave-uniform) the wave's block holds keys
        Acc acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
        int32_t rs = 0, cs = 0;
        uint4 vq = make_uint4(0u, 0u, 0u, 0u), vk0 = vq, vk1 = vq;
        [[maybe_unused]] E bv[16];  // BIAS: the lane's sixteen bias elements
        if constexpr (BIAS && BIAS_EARLY) att_bias_load<E>(bv, a, bi, m0, n0 + wave * 32 + fr, fh, active);
        if (tid < 4 * ATT_ROWS) vq = mm_piece<F16>(pq, q_row, m0, a.S, 0, a.D, 1, a.q_vec, tid);
        if (mover) {
            vk0 = mm_piece<F16>(pk, k_row, n0, T, 0, a.D, 1, a.k_vec, tid);
            vk1 = mm_piece<F16>(pk, k_row, n0 + MM_T, T, 0, a.D, 1, a.k_vec, tid);
        }
        for (int k0 = 0; k0 < a.D; k0 += KS) {
            __syncthreads();  // the previous slab's fragments were read
            if constexpr (LAYOUT && F16) {  // (between mm_piece and mm_put: the operand as its movers would have left it)
                if (fix_q) vq = att_moved(vq);
                if (fix_k) vk0 = att_moved(vk0), vk1 = att_moved(vk1);
            }
            if (tid < 4 * ATT_ROWS) mm_put<F16>(lds_q, vq, 1, tid);
            if (mover) {
                mm_put<F16>(lds_kv, vk0, 1, tid);
                mm_put<F16>(lds_kv + MM_T * MM_PITCH, vk1, 1, tid);
            }
            __syncthreads();
            if (mover && k0 + KS < a.D) {  // the next slab's pieces travel while this slab's MFMAs run
                if (tid < 4 * ATT_ROWS) vq = mm_piece<F16>(pq, q_row, m0, a.S, k0 + KS, a.D, 1, a.q_vec, tid);
                vk0 = mm_piece<F16>(pk, k_row, n0, T, k0 + KS, a.D, 1, a.k_vec, tid);
                vk1 = mm_piece<F16>(pk, k_row, n0 + MM_T, T, k0 + KS, a.D, 1, a.k_vec, tid);
            }
            if (!active) continue;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const v4i fa = *reinterpret_cast<const v4i *>(lds_q + fr * MM_PITCH + s * 32 + fh * 16);
                const v4i fb = *reinterpret_cast<const v4i *>(lds_kv + (wave * 32 + fr) * MM_PITCH + s * 32 + fh * 16);
                acc = mfma<!F16>(fa, fb, acc);
                if constexpr (!F16) {
                    if (a.izk != 0) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) rs = __builtin_amdgcn_sdot4(fa[j], 0x01010101, rs, false);
                    }
                    if (a.izq != 0) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) cs = __builtin_amdgcn_sdot4(fb[j], 0x01010101, cs, false);
                    }
                }
            }
        }
        // (asked for in front of the row sums' exchange and its barrier, which the elements then travel behind)
        if constexpr (BIAS && !BIAS_EARLY) att_bias_load<E>(bv, a, bi, m0, n0 + wave * 32 + fr, fh, active);
        if constexpr (!F16) {
            // a lane holds half of its row's / column's k: the other half is 32 lanes away
            rs += __shfl_xor(rs, 32);
            cs += __shfl_xor(cs, 32);
            if (mover && fh == 0) row_sum[wave][fr] = rs;
            __syncthreads();
        }
        // C/D layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        const int key = n0 + wave * 32 + fr;
        const int32_t kzz = a.D * a.izq * a.izk;  // (D <= 32768, |zp| <= 128: below 2^30)
        if (mover && key < T) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * fh;
                E *const dst = reinterpret_cast<E *>(tile + row * tp) + key;
                if constexpr (F16) {
                    uint16_t h = (uint16_t)mm_value<true>(acc[r], a.s_so, a.s_zo, a.s_inv, a.s_div);
                    if (a.has_scale) h = mul_f16_one(h, (uint16_t)a.craw, a.mul);
                    if constexpr (BIAS) h = a.bias_first ? add_f16_step(bv[r], h) : add_f16_step(h, bv[r]);
                    *dst = h;
                } else {
                    // (every term and the true sum fit 32 bits; unsigned arithmetic, so that no intermediate wrap is undefined)
                    const uint32_t S = (uint32_t)acc[r] - (uint32_t)(a.izk * row_sum[wave][row]) - (uint32_t)(a.izq * cs) + (uint32_t)kzz;
                    int qv = mm_value<false>(__fmul_rn((float)(int32_t)S, a.mult1), a.s_so, a.s_zo, a.s_inv, a.s_div);
                    if (a.has_scale) qv = mul_i8_one(qv, a.craw, a.mul);
                    if constexpr (BIAS) qv = add_i8_step(qv, (int)(int8_t)bv[r], a.add);
                    *dst = (E)(int8_t)qv;
                }
            }
        }
    }
    __syncthreads();  // the tile is complete

    // ---- softmax along the keys, a row per wave; the probabilities overwrite the scores ---------------------------------------
    {
        const int tk = (T + KS - 1) / KS * KS;  // the keys of P V's whole slabs: those past T are zeros
        double *const lut_e = reinterpret_cast<double *>(smem + a.lds.lut_e) + wave * 256;  // (a table per wave)
        int8_t *const lut_q = reinterpret_cast<int8_t *>(smem + a.lds.lut_q) + wave * 256;
        const bool table = !F16 && T > ATT_TABLE_ABOVE;
#pragma unroll
        for (int j = 0; j < 4; ++j) e[T + 4 * lane + j] = 0.0;
        for (int row = wave; row < ATT_ROWS; row += nw) {
            E *const x = reinterpret_cast<E *>(tile + row * tp);
            for (int j = T + lane; j < tk; j += 64) x[j] = 0;
            if (m0 + row >= a.S) continue;  // (wave-uniform) a row past the last query: nothing of it is stored
            // max (fmax over floats: exact whatever the order)
            float m = -3.402823466e+38f;
            for (int j = lane; j < T; j += 64) {
                if constexpr (F16) m = fmaxf(m, f16_bits_to_float(x[j]));
                else m = fmaxf(m, dequant_i8((int8_t)x[j], a.x_zi, a.x_si));
            }
#pragma unroll
            for (int w = 32; w >= 1; w >>= 1) m = fmaxf(m, __shfl_xor(m, w));
            if (table) {
                // the row holds at most 256 distinct values: lane l evaluates the exponential (and, below, the quotient and its
                // requantisation) of the values l - 128, l - 64, l, l + 64 once, the elements look theirs up
                for (int v = lane; v < 256; v += 64) lut_e[v] = softmax_exp(dequant_i8(v - 128, a.x_zi, a.x_si), m);
                wave_lds_sync();
                for (int j = lane; j < T; j += 64) e[j] = lut_e[(int)(int8_t)x[j] + 128];
            } else {
                for (int j = lane; j < T; j += 64) {
                    if constexpr (F16) e[j] = softmax_exp(f16_bits_to_float(x[j]), m);
                    else e[j] = softmax_exp(dequant_i8((int8_t)x[j], a.x_zi, a.x_si), m);
                }
            }
            wave_lds_sync();
            const double acc = (double)running_sum_exact(e, T, lane);
            if (table) {
                for (int v = lane; v < 256; v += 64) lut_q[v] = (int8_t)requant_i8((float)(lut_e[v] / acc), a.p_so, a.p_zo);
                wave_lds_sync();
                for (int j = lane; j < T; j += 64) x[j] = (E)lut_q[(int)(int8_t)x[j] + 128];
            } else {
                for (int j = lane; j < T; j += 64) {
                    const float pj = (float)(e[j] / acc);
                    if constexpr (F16) x[j] = float_to_f16_bits_ref(pj);
                    else x[j] = (E)(int8_t)requant_i8(pj, a.p_so, a.p_zo);
                }
            }
            wave_lds_sync();  // the next row reuses e and the tables
        }
    }

    // ---- out = P V: p from the tile as the [row][k] operand, v through the transposing write ---------------------------------
    for (int c0 = 0; c0 < a.DV; c0 += ATT_KEYS) {
        const bool active = mover && c0 + wave * 32 < a.DV;
        Acc acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
        int32_t rs = 0, cs = 0;
        uint4 vv0 = make_uint4(0u, 0u, 0u, 0u), vv1 = vv0;
        if (mover) {
            vv0 = mm_piece<F16>(pv, v_row, c0, a.DV, 0, T, 0, a.v_vec, tid);
            vv1 = mm_piece<F16>(pv, v_row, c0 + MM_T, a.DV, 0, T, 0, a.v_vec, tid);
        }
        for (int k0 = 0; k0 < T; k0 += KS) {
            __syncthreads();  // the previous slab's fragments were read (first slab: every wave's probabilities are written)
            if constexpr (LAYOUT && F16) {
                if (fix_v) vv0 = att_moved(vv0), vv1 = att_moved(vv1);
            }
            if (mover) {
                mm_put<F16>(lds_kv, vv0, 0, tid);
                mm_put<F16>(lds_kv + MM_T * MM_PITCH, vv1, 0, tid);
            }
            __syncthreads();
            if (mover && k0 + KS < T) {
                vv0 = mm_piece<F16>(pv, v_row, c0, a.DV, k0 + KS, T, 0, a.v_vec, tid);
                vv1 = mm_piece<F16>(pv, v_row, c0 + MM_T, a.DV, k0 + KS, T, 0, a.v_vec, tid);
            }
            if (!active) continue;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const v4i fa = *reinterpret_cast<const v4i *>(tile + fr * tp + k0 * ES + s * 32 + fh * 16);
                const v4i fb = *reinterpret_cast<const v4i *>(lds_kv + (wave * 32 + fr) * MM_PITCH + s * 32 + fh * 16);
                acc = mfma<!F16>(fa, fb, acc);
                if constexpr (!F16) {
                    if (a.izv != 0) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) rs = __builtin_amdgcn_sdot4(fa[j], 0x01010101, rs, false);
                    }
                    if (a.izp != 0) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) cs = __builtin_amdgcn_sdot4(fb[j], 0x01010101, cs, false);
                    }
                }
            }
        }
        if constexpr (!F16) {
            rs += __shfl_xor(rs, 32);
            cs += __shfl_xor(cs, 32);
            if (mover && fh == 0) row_sum[wave][fr] = rs;
            __syncthreads();
        }
        const int n = c0 + wave * 32 + fr;
        const int32_t kzz = T * a.izp * a.izv;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * fh;
            const int m = m0 + row;
            if (!mover || m >= a.S || n >= a.DV) continue;
            // LAYOUT: the movers behind the core would change nothing of what is stored here -- mm_value<true> gives a NaN as
            // 0x7FFF / 0xFFFF and float_to_f16_bits_ref saturates everything else to at most 0x7BFF in magnitude, and
            // move_fix_f16x2 leaves exactly those halves alone --, so the output's moved bit needs no work
            int64_t o;
            if constexpr (LAYOUT) o = (int64_t)(o_base + (uint32_t)m * (uint32_t)a.lay.o_row + (uint32_t)n);
            else o = ((int64_t)bi * a.S + m) * a.DV + n;
            if constexpr (F16) {
                static_cast<uint16_t *>(a.out)[o] = (uint16_t)mm_value<true>(acc[r], a.o_so, a.o_zo, a.o_inv, a.o_div);
            } else {
                const uint32_t S = (uint32_t)acc[r] - (uint32_t)(a.izv * row_sum[wave][row]) - (uint32_t)(a.izp * cs) + (uint32_t)kzz;
                static_cast<int8_t *>(a.out)[o] =
                    (int8_t)mm_value<false>(__fmul_rn((float)(int32_t)S, a.mult2), a.o_so, a.o_zo, a.o_inv, a.o_div);
            }
        }
    }
}

// NULL, or why the call is refused; *code: the status that goes with it
static const char *attention_refusal(const void *q, const void *k, const void *v, const void *out, const shl_mi355x_attention_desc *d,
                                     int *code)
{
    *code = SHL_MI355X_EINVAL;
    const char *why = att_validate(q, k, v, out, d);
    if (why) return why;
    *code = SHL_MI355X_ENOTSUP;
    return att_unsupported(d);
}

}  // namespace shl

extern "C" const char *shl_mi355x_attention_kernel_name(const void *q_dev, const void *k_dev, const void *v_dev, const void *out_dev,
                                                        const struct shl_mi355x_attention_desc *d)
{
    int code;
    return shl::attention_refusal(q_dev, k_dev, v_dev, out_dev, d, &code) ? "" : SHL_MI355X_ATTENTION_MFMA;
}

extern "C" int shl_mi355x_attention_by_default(const void *q_dev, const void *k_dev, const void *v_dev, const void *out_dev,
                                               const struct shl_mi355x_attention_desc *d)
{
    int code;
    return !shl::attention_refusal(q_dev, k_dev, v_dev, out_dev, d, &code) && shl::att_default(d) ? 1 : 0;
}

namespace shl {

// the arguments both launches share, for a call attention_refusal has passed; *waves: the workgroup's
static void attention_args(const void *q_dev, const void *k_dev, const void *v_dev, void *out_dev, const shl_mi355x_attention_desc *d,
                           AttArgs &a, int *waves)
{
    const bool f16 = d->dtype == SHL_MI355X_F16;
    const int64_t es = f16 ? 2 : 1;
    shl_mi355x_matmul_desc qk, pv;
    att_qk_desc(d, &qk);
    att_pv_desc(d, &pv);
    a.q = q_dev, a.k = k_dev, a.v = v_dev, a.out = out_dev;
    a.batches = d->batches, a.S = d->s, a.T = d->t, a.D = d->d, a.DV = d->dv;
    a.tiles = (d->s + ATT_ROWS - 1) / ATT_ROWS;
    a.q_vec = att_vec(q_dev, d->d, es), a.k_vec = att_vec(k_dev, d->d, es), a.v_vec = att_vec(v_dev, d->dv, es);
    *waves = att_waves(d);
    a.lds = att_lds(d, *waves);
    // the products' constants as matmul_launch sets them
    a.izq = d->q_zp, a.izk = d->k_zp, a.mult1 = d->q_scale * d->k_scale;  // rounded once, here
    a.s_so = d->s_scale, a.s_zo = (float)d->s_zp, a.s_inv = 1.0f / d->s_scale, a.s_div = !f16 && mm_fma_ok(&qk);
    a.izp = d->p_zp, a.izv = d->v_zp, a.mult2 = d->p_scale * d->v_scale;
    a.o_so = d->out_scale, a.o_zo = (float)d->out_zp, a.o_inv = 1.0f / d->out_scale, a.o_div = !f16 && mm_fma_ok(&pv);
    // the multiply's as bcast_launch sets them: a the scores, b the constant
    a.has_scale = d->has_scale, a.craw = d->scale_raw;
    a.mul.sa = d->s_scale, a.mul.za = (float)d->s_zp, a.mul.sb = d->c_scale, a.mul.zb = (float)d->c_zp;
    a.mul.so = d->sc_scale, a.mul.zo = (float)d->sc_zp, a.mul.inv_so = 1.0f / d->sc_scale;
    a.mul.fma_div = mul_fma_ok(d->s_scale, d->s_zp, d->c_scale, d->c_zp, d->sc_scale);
    a.mul.a_second = d->scale_is_first ? 1 : 0;
    a.x_si = d->has_scale ? d->sc_scale : d->s_scale, a.x_zi = (float)(d->has_scale ? d->sc_zp : d->s_zp);
    a.p_so = d->p_scale, a.p_zo = (float)d->p_zp;
}

template <typename Args>
static int attention_enqueue(void (*kernel)(Args), LdsOptIn &opted_in, const Args &a, int waves, void *stream)
{
    const int64_t groups = (int64_t)a.batches * a.tiles;  // (at most the output's element count)
    if (a.lds.bytes > 48 * 1024) lds_opt_in(opted_in, reinterpret_cast<const void *>(kernel));
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(64 * (unsigned)waves), (size_t)a.lds.bytes, (hipStream_t)stream, a);
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

// the biased launches' further arguments, behind attention_args
static void attention_bias_args(const void *bias_dev, const shl_mi355x_attention_desc *d, const shl_mi355x_attention_bias_desc *bd,
                                AttBiasArgs &a)
{
    // the add's as bcast_launch sets them: a the (scaled) scores, b the bias; the softmax then reads the sum's record.  add_rec
    // is the one rule that picks the int8 division for shl_mi355x_add_bcast as well
    a.bias = bias_dev;
    a.add = add_rec(a.x_si, d->has_scale ? d->sc_zp : d->s_zp, bd->b_scale, bd->b_zp, bd->sb_scale, bd->sb_zp);
    a.x_si = bd->sb_scale, a.x_zi = (float)bd->sb_zp;
    a.bias_first = bd->bias_is_first;
    // (a stride along an extent of 1 is never used: att_bias_last has bounded the others)
    a.b_ext1 = bd->b_ext1;
    a.b_stride0 = d->batches / bd->b_ext1 > 1 ? (int32_t)bd->b_stride[0] : 0, a.b_stride1 = bd->b_ext1 > 1 ? (int32_t)bd->b_stride[1] : 0;
    a.row_stride = d->s > 1 ? (int32_t)bd->row_stride : 0, a.key_stride = d->t > 1 ? (int32_t)bd->key_stride : 0;
}

// NULL, or why the biased call is refused; *code: the status that goes with it
static const char *attention_bias_refusal(const void *q, const void *k, const void *v, const void *bias, const void *out,
                                          const shl_mi355x_attention_desc *d, const shl_mi355x_attention_bias_desc *bd, int *code)
{
    *code = SHL_MI355X_EINVAL;
    const char *why = att_bias_validate(q, k, v, bias, out, d, bd);
    if (why) return why;
    *code = SHL_MI355X_ENOTSUP;
    return att_unsupported(d);
}

}  // namespace shl

extern "C" int shl_mi355x_attention(const void *q_dev, const void *k_dev, const void *v_dev, void *out_dev,
                                    const struct shl_mi355x_attention_desc *d, void *stream)
{
    using namespace shl;
    int code;
    const char *why = attention_refusal(q_dev, k_dev, v_dev, out_dev, d, &code);
    if (why) {
        set_error("attention: %s", why);
        return code;
    }
    AttArgs a;
    memset(&a, 0, sizeof(a));
    int waves;
    attention_args(q_dev, k_dev, v_dev, out_dev, d, a, &waves);
    static LdsOptIn opted_in[2];
    const bool f16 = d->dtype == SHL_MI355X_F16;
    return attention_enqueue(f16 ? attention_mfma_kernel<true, false, false> : attention_mfma_kernel<false, false, false>, opted_in[f16], a, waves, stream);
}

extern "C" const char *shl_mi355x_attention_bias_kernel_name(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev,
                                                             const void *out_dev, const struct shl_mi355x_attention_desc *d,
                                                             const struct shl_mi355x_attention_bias_desc *bd)
{
    int code;
    return shl::attention_bias_refusal(q_dev, k_dev, v_dev, bias_dev, out_dev, d, bd, &code) ? "" : SHL_MI355X_ATTENTION_BIAS_MFMA;
}

extern "C" int shl_mi355x_attention_bias_by_default(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev,
                                                    const void *out_dev, const struct shl_mi355x_attention_desc *d,
                                                    const struct shl_mi355x_attention_bias_desc *bd)
{
    int code;
    return !shl::attention_bias_refusal(q_dev, k_dev, v_dev, bias_dev, out_dev, d, bd, &code) && shl::att_bias_default(d) ? 1 : 0;
}

extern "C" int shl_mi355x_attention_bias_geometry(const struct shl_mi355x_mul_desc *m, int32_t batches, int32_t s, int32_t t,
                                                  struct shl_mi355x_attention_bias_desc *bd)
{
    const int rc = shl::att_bias_geometry(m, batches, s, t, bd);
    if (rc == 1) shl::set_error("attention_bias_geometry: the groups are not those of [batches][s][t]");
    if (rc == 2) shl::set_error("attention_bias_geometry: a bias that i0, i1, row and key strides cannot express");
    return rc == 0 ? SHL_MI355X_OK : rc == 1 ? SHL_MI355X_EINVAL : SHL_MI355X_ENOTSUP;
}

extern "C" int shl_mi355x_attention_bias(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev, void *out_dev,
                                         const struct shl_mi355x_attention_desc *d, const struct shl_mi355x_attention_bias_desc *bd,
                                         void *stream)
{
    using namespace shl;
    int code;
    const char *why = attention_bias_refusal(q_dev, k_dev, v_dev, bias_dev, out_dev, d, bd, &code);
    if (why) {
        set_error("attention_bias: %s", why);
        return code;
    }
    AttBiasArgs a;
    memset(&a, 0, sizeof(a));
    int waves;
    attention_args(q_dev, k_dev, v_dev, out_dev, d, a, &waves);
    attention_bias_args(bias_dev, d, bd, a);
    static LdsOptIn opted_in[2];
    const bool f16 = d->dtype == SHL_MI355X_F16;
    return attention_enqueue(f16 ? attention_mfma_kernel<true, true, false> : attention_mfma_kernel<false, true, false>, opted_in[f16], a, waves, stream);
}

// ---- the layout form: the operands where the projections left them (shl_mi355x_attention_layout) ------------------------------
namespace shl {

// NULL, or why the layout call is refused; *code: the status that goes with it
static const char *attention_layout_refusal(const void *q, const void *k, const void *v, const void *bias, const void *out,
                                            const shl_mi355x_attention_desc *d, const shl_mi355x_attention_bias_desc *bd,
                                            const shl_mi355x_attention_layout_desc *ld, int *code)
{
    *code = SHL_MI355X_EINVAL;
    const char *why = att_layout_validate(q, k, v, bias, out, d, bd, ld);
    if (why) return why;
    *code = SHL_MI355X_ENOTSUP;
    return att_unsupported(d);
}

static void attention_layout_args(const void *q_dev, const void *k_dev, const void *v_dev, const shl_mi355x_attention_desc *d,
                                  const shl_mi355x_attention_layout_desc *ld, AttArgs &a, AttLayoutPart &lay)
{
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    const int64_t ext_q[3] = {d->batches / ld->heads, ld->heads, d->s}, ext_kv[3] = {d->batches / ld->heads, ld->heads, d->t};
    a.q_vec = att_vec_layout(q_dev, ld->q_stride, ext_q, d->d, es), a.k_vec = att_vec_layout(k_dev, ld->k_stride, ext_kv, d->d, es);
    a.v_vec = att_vec_layout(v_dev, ld->v_stride, ext_kv, d->dv, es);
    lay.heads = ld->heads, lay.moved = ld->moved;
    lay.q_outer = ld->q_stride[0], lay.q_head = ld->q_stride[1], lay.q_row = ld->q_stride[2];
    lay.k_outer = ld->k_stride[0], lay.k_head = ld->k_stride[1], lay.k_row = ld->k_stride[2];
    lay.v_outer = ld->v_stride[0], lay.v_head = ld->v_stride[1], lay.v_row = ld->v_stride[2];
    lay.o_outer = ld->out_stride[0], lay.o_head = ld->out_stride[1], lay.o_row = ld->out_stride[2];
}

}  // namespace shl

extern "C" const char *shl_mi355x_attention_layout_kernel_name(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev,
                                                               const void *out_dev, const struct shl_mi355x_attention_desc *d,
                                                               const struct shl_mi355x_attention_bias_desc *bd,
                                                               const struct shl_mi355x_attention_layout_desc *ld)
{
    int code;
    if (shl::attention_layout_refusal(q_dev, k_dev, v_dev, bias_dev, out_dev, d, bd, ld, &code)) return "";
    return bias_dev ? SHL_MI355X_ATTENTION_BIAS_LAYOUT_MFMA : SHL_MI355X_ATTENTION_LAYOUT_MFMA;
}

extern "C" int shl_mi355x_attention_layout_by_default(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev,
                                                      const void *out_dev, const struct shl_mi355x_attention_desc *d,
                                                      const struct shl_mi355x_attention_bias_desc *bd,
                                                      const struct shl_mi355x_attention_layout_desc *ld)
{
    int code;
    return !shl::attention_layout_refusal(q_dev, k_dev, v_dev, bias_dev, out_dev, d, bd, ld, &code) && shl::att_layout_default(d, ld) ? 1 : 0;
}

extern "C" int shl_mi355x_attention_layout_strides(const int32_t *src_dim, int32_t src_rank, int32_t nsteps, const int32_t *step_is_transpose,
                                                   const int32_t *step_rank, const int32_t *step_v, int32_t swap_last2, int32_t *batches,
                                                   int32_t *rows, int32_t *cols, int32_t *heads, int32_t stride[3])
{
    using namespace shl;
    constexpr int MAX_STEPS = 8;
    AttViewStep step[MAX_STEPS];
    int rc = 1;
    if (nsteps >= 0 && nsteps <= MAX_STEPS && (nsteps == 0 || (step_is_transpose && step_rank && step_v))) {
        for (int i = 0; i < nsteps; ++i) {
            step[i].is_transpose = step_is_transpose[i], step[i].rank = step_rank[i];
            for (int j = 0; j < SHL_MI355X_MAX_DIM; ++j) step[i].v[j] = j < step_rank[i] ? step_v[i * SHL_MI355X_MAX_DIM + j] : 0;
        }
        rc = att_layout_strides(src_dim, src_rank, step, nsteps, swap_last2, batches, rows, cols, heads, stride);
    }
    if (rc == 1) set_error("attention_layout_strides: the arguments describe no view of the source");
    if (rc == 2) set_error("attention_layout_strides: a view that outer, head and row strides cannot express");
    return rc == 0 ? SHL_MI355X_OK : rc == 1 ? SHL_MI355X_EINVAL : SHL_MI355X_ENOTSUP;
}

extern "C" int shl_mi355x_attention_layout(const void *q_dev, const void *k_dev, const void *v_dev, const void *bias_dev, void *out_dev,
                                           const struct shl_mi355x_attention_desc *d, const struct shl_mi355x_attention_bias_desc *bd,
                                           const struct shl_mi355x_attention_layout_desc *ld, void *stream)
{
    using namespace shl;
    int code;
    const char *why = attention_layout_refusal(q_dev, k_dev, v_dev, bias_dev, out_dev, d, bd, ld, &code);
    if (why) {
        set_error("attention_layout: %s", why);
        return code;
    }
    const bool f16 = d->dtype == SHL_MI355X_F16;
    int waves;
    static LdsOptIn opted_in[4];
    if (!bias_dev) {
        AttLayoutArgs a;
        memset(&a, 0, sizeof(a));
        attention_args(q_dev, k_dev, v_dev, out_dev, d, a, &waves);
        attention_layout_args(q_dev, k_dev, v_dev, d, ld, a, a.lay);
        return attention_enqueue(f16 ? attention_mfma_kernel<true, false, true> : attention_mfma_kernel<false, false, true>, opted_in[f16], a,
                                 waves, stream);
    }
    AttBiasLayoutArgs a;
    memset(&a, 0, sizeof(a));
    attention_args(q_dev, k_dev, v_dev, out_dev, d, a, &waves);
    attention_bias_args(bias_dev, d, bd, a);
    attention_layout_args(q_dev, k_dev, v_dev, d, ld, a, a.lay);
    return attention_enqueue(f16 ? attention_mfma_kernel<true, true, true> : attention_mfma_kernel<false, true, true>, opted_in[2 + f16], a,
                             waves, stream);
}

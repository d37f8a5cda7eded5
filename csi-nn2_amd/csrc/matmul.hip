// matmul.hip -- batched matrix product of two int8 / binary16 tensors, both transposes and the reference's "dense"
// broadcast: CSINN_OP_MATMUL.
//
// Restates shl_ref_matmul_f32 behind shl_ref_diso_callback_base (source/reference/matmul.c:21-132, utils.c:623-637): both
// operands converted to float32 with their records, per output `total = 0; for k: total += a * b` in float32 with k
// ascending, the result converted with the output's record.  The layer's nine loop nests differ in their offsets only; here
// they are strides of one descriptor (element (b, i, k) of A at b abs + i ars + k aks, element (b, k, j) of B at
// b bbs + j brs + k bks; the broadcast is bbs == 0).
//
// Two forms, chosen by mm_form (matmul_canon.h) for the launch and for shl_mi355x_matmul_kernel_name:
//   matmul_chain  one output per thread, the literal chain: one __fmaf_rn per step (the reference's build contracts
//                 `total += a * b`), k ascending, the loads of eight steps issued ahead of their additions.  Bit-identical to the reference for any records.
//                 A binary16 chain can meet NaNs, and float32_to_float16_base keeps a NaN's sign: the steps restate which
//                 NaN an x86 multiplication and addition hand on instead of trusting this machine's
//   matmul_mfma   a workgroup of four waves owns a 64 x 64 output tile of one batch, a wave a 32 x 32 quarter
//                 (v_mfma_i32_32x32x32_i8 / v_mfma_f32_32x32x16_f16: 16 bytes of k per lane and operand).  The K loop walks
//                 slabs of 64 bytes of k: every thread loads ONE 16-byte piece of A and one of B along the operand's
//                 contiguous dimension (one uint4 where the plan proved every piece aligned, else element loads), the
//                 next slab's pieces are in flight while this slab's MFMAs run, and the pieces are written to LDS as
//                 [row][k] for both operands -- a transposed operand is transposed by that write.  Rows past M / N and k
//                 past K are written as zeros.  LDS: 2 x 64 rows x 80 bytes (64 + 16: the 32 rows a fragment read walks
//                 fall on different banks) + 512 bytes of row sums = 10.5 KiB.
//                 int8 multiplies the RAW bytes and corrects afterwards: S = sum qa qb - zb sum_k qa - za sum_k qb +
//                 K za zb.  The row sums of A and the column sums of B come from the fragments the wave holds anyway
//                 (v_dot4 against ones), only when the other operand's zero point is not 0; the zero-filled K tail adds
//                 nothing to any of the three sums, the constant term uses the true K.  Then f = (float)S * mult,
//                 sat8(rint(f / s_out) + zp_out) with div_by_scale where mm_fma_ok admits the records.
//                 binary16: exact products, float32 accumulation on the matrix cores, the reference's conversion.
//
// matmul + add(constant bias[N]) as one launch (shl_mi355x_matmul_bias; a session's STEP_MATMUL_BIAS): both kernels have a
// second instantiation, BIAS, that differs in mm_store alone.  There the value the plain kernel would STORE -- the int8 byte
// under the intermediate record, the rounded half -- stays in a register and goes through the add's own element function
// (add_step.h) with bias[n], n the output's column: matmul followed by add, bit for bit, without the intermediate tensor's
// trip through HBM.  The plain instantiations do not contain the epilogue.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "matmul_canon.h"  // the host side: validation, the exactness proof, the form rule (a stand-alone program compiles it too)
#include "matmul_step.h"   // the store and the mfma form's slab pieces, shared with attention.hip

namespace shl {

// (MmArgs, mm_load, mm_store and the mfma form's mm_piece / mm_put: matmul_step.h, which attention.hip includes as well)

template <bool F16>
__device__ __forceinline__ float mm_cvt(uint32_t raw, float z, float s)
{
    if constexpr (F16) return f16_bits_to_float((uint16_t)raw);
    else return __fmul_rn(__fsub_rn((float)(int8_t)raw, z), s);  // int8_to_float_base
}

// total += x * y as the reference's build computes it: -O3 -mfma contracts the product and the sum into ONE fused
// multiply-add (the genuine library's outputs show it: with converter scales a rounded product followed by a rounded sum
// differs in about one output of two thousand).  binary16 only: a NaN result hands on the accumulator's NaN, else an
// operand's, else (inf * 0, inf - inf) the default NaN, whose sign bit is set on x86
template <bool F16>
__device__ __forceinline__ float mm_step(float acc, float x, float y)
{
    const float r = __fmaf_rn(x, y, acc);
    if constexpr (F16) return r == r ? r : (acc != acc ? acc : (x != x ? x : (y != y ? y : __uint_as_float(0xFFC00000u))));
    else return r;
}

template <bool F16, bool BIAS = false>
__global__ __launch_bounds__(256) void matmul_chain_kernel(MmArgs a)
{
    constexpr int B = 8;  // loads in flight ahead of the additions
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= (int64_t)a.batches * a.M * a.N) return;  // (the product is the output's element count: below 2^31)
    const uint32_t mn = (uint32_t)a.M * (uint32_t)a.N;
    const uint32_t bi = (uint32_t)o / mn, r = (uint32_t)o - bi * mn;
    const uint32_t m = r / (uint32_t)a.N, n = r - m * (uint32_t)a.N;
    const int64_t pa = (int64_t)bi * a.abs + (int64_t)m * a.ars, pb = (int64_t)bi * a.bbs + (int64_t)n * a.brs;
    uint32_t braw = 0;
    if constexpr (BIAS) braw = mm_load<F16>(a.bias, n);
    float acc = 0.0f;
    int32_t k = 0;
    for (; k + B <= a.K; k += B) {
        uint32_t ra[B], rb[B];
#pragma unroll
        for (int j = 0; j < B; ++j) {
            ra[j] = mm_load<F16>(a.a, pa + (int64_t)(k + j) * a.aks);
            rb[j] = mm_load<F16>(a.b, pb + (int64_t)(k + j) * a.bks);
        }
#pragma unroll
        for (int j = 0; j < B; ++j) acc = mm_step<F16>(acc, mm_cvt<F16>(ra[j], a.za, a.sa), mm_cvt<F16>(rb[j], a.zb, a.sb));
    }
    for (; k < a.K; ++k)
        acc = mm_step<F16>(acc, mm_cvt<F16>(mm_load<F16>(a.a, pa + (int64_t)k * a.aks), a.za, a.sa),
                           mm_cvt<F16>(mm_load<F16>(a.b, pb + (int64_t)k * a.bks), a.zb, a.sb));
    mm_store<F16, BIAS>(a, o, acc, braw);
}

// ---- the mfma form (its slab pieces and their LDS image: matmul_step.h) ------------------------------------------------------
template <bool F16, bool BIAS = false>
__global__ __launch_bounds__(256) void matmul_mfma_kernel(MmArgs a)
{
    using Acc = typename AccT<!F16>::type;
    constexpr int ES = F16 ? 2 : 1, KS = MM_KB / ES;  // elements of k per slab
    __shared__ __attribute__((aligned(16))) char lds_a[MM_T * MM_PITCH];
    __shared__ __attribute__((aligned(16))) char lds_b[MM_T * MM_PITCH];
    __shared__ int32_t row_sum[4][32];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1, fr = lane & 31, fh = lane >> 5;
    const uint32_t tiles = (uint32_t)a.tiles_m * (uint32_t)a.tiles_n;
    const uint32_t bi = blockIdx.x / tiles, t = blockIdx.x - bi * tiles;
    const int m0 = (int)(t / (uint32_t)a.tiles_n) * MM_T, n0 = (int)(t % (uint32_t)a.tiles_n) * MM_T;
    const void *pa = static_cast<const char *>(a.a) + (int64_t)bi * a.abs * ES;
    const void *pb = static_cast<const char *>(a.b) + (int64_t)bi * a.bbs * ES;
    const int64_t a_os = a.a_kc ? a.ars : a.aks, b_os = a.b_kc ? a.brs : a.bks;

    uint32_t braw = 0;  // the lane's column of the output is one for all its sixteen outputs
    if constexpr (BIAS) {
        const int col = n0 + wn * 32 + fr;
        if (col < a.N) braw = mm_load<F16>(a.bias, col);
    }
    Acc acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
    int32_t rs = 0, cs = 0;
    uint4 va = mm_piece<F16>(pa, a_os, m0, a.M, 0, a.K, a.a_kc, a.a_vec, tid);
    uint4 vb = mm_piece<F16>(pb, b_os, n0, a.N, 0, a.K, a.b_kc, a.b_vec, tid);
    for (int k0 = 0; k0 < a.K; k0 += KS) {
        __syncthreads();  // the previous slab's fragments were read
        mm_put<F16>(lds_a, va, a.a_kc, tid);
        mm_put<F16>(lds_b, vb, a.b_kc, tid);
        __syncthreads();
        if (k0 + KS < a.K) {  // the next slab's pieces travel while this slab's MFMAs run
            va = mm_piece<F16>(pa, a_os, m0, a.M, k0 + KS, a.K, a.a_kc, a.a_vec, tid);
            vb = mm_piece<F16>(pb, b_os, n0, a.N, k0 + KS, a.K, a.b_kc, a.b_vec, tid);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const v4i fa = *reinterpret_cast<const v4i *>(lds_a + (wm * 32 + fr) * MM_PITCH + s * 32 + fh * 16);
            const v4i fb = *reinterpret_cast<const v4i *>(lds_b + (wn * 32 + fr) * MM_PITCH + s * 32 + fh * 16);
            acc = mfma<!F16>(fa, fb, acc);
            if constexpr (!F16) {
                if (a.izb != 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) rs = __builtin_amdgcn_sdot4(fa[j], 0x01010101, rs, false);
                }
                if (a.iza != 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) cs = __builtin_amdgcn_sdot4(fb[j], 0x01010101, cs, false);
                }
            }
        }
    }
    if constexpr (!F16) {
        // a lane holds half of its row's / column's k: the other half is 32 lanes away
        rs += __shfl_xor(rs, 32);
        cs += __shfl_xor(cs, 32);
        if (fh == 0) row_sum[wave][fr] = rs;
        __syncthreads();
    }
    // C/D layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int n = n0 + wn * 32 + fr;
    const int32_t kzz = a.K * a.iza * a.izb;  // (K <= 32768, |zp| <= 128: below 2^30)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * fh;
        const int m = m0 + wm * 32 + row;
        if (m >= a.M || n >= a.N) continue;
        const int64_t o = ((int64_t)bi * a.M + m) * a.N + n;
        if constexpr (F16) {
            mm_store<true, BIAS>(a, o, acc[r], braw);
        } else {
            // (every term and the true sum fit 32 bits; unsigned arithmetic, so that no intermediate wrap is undefined)
            const uint32_t S = (uint32_t)acc[r] - (uint32_t)(a.izb * row_sum[wave][row]) - (uint32_t)(a.iza * cs) + (uint32_t)kzz;
            mm_store<false, BIAS>(a, o, __fmul_rn((float)(int32_t)S, a.mult), braw);
        }
    }
}

// ---- host side (validation, the proof and the form rule are in matmul_canon.h) -----------------------------------------
// the fused bias of shl_mi355x_matmul_bias: NULL for the plain product
struct MmBias {
    const void *dev;
    float scale, mid_scale;
    int32_t zp, mid_zp, first;
};

static int matmul_launch(const void *a_dev, const void *b_dev, void *out_dev, const shl_mi355x_matmul_desc *d, const MmBias *bias,
                         hipStream_t s)
{
    const bool f16 = d->dtype == SHL_MI355X_F16;
    MmPlan p;
    mm_plan(a_dev, b_dev, d, &p);
    const int form = mm_form(d, &p);
    MmArgs a;
    memset(&a, 0, sizeof(a));
    a.a = a_dev, a.b = b_dev, a.out = out_dev;
    a.batches = d->batches, a.M = d->m, a.N = d->n, a.K = d->k;
    a.abs = d->a_batch_stride, a.ars = d->a_row_stride, a.aks = d->a_k_stride;
    a.bbs = d->b_batch_stride, a.brs = d->b_col_stride, a.bks = d->b_k_stride;
    a.a_kc = p.a_kcontig, a.b_kc = p.b_kcontig, a.a_vec = p.a_vec, a.b_vec = p.b_vec;
    a.sa = d->a_scale, a.za = (float)d->a_zp, a.sb = d->b_scale, a.zb = (float)d->b_zp;
    a.so = d->out_scale, a.zo = (float)d->out_zp, a.inv_so = 1.0f / d->out_scale;
    a.iza = d->a_zp, a.izb = d->b_zp;
    a.mult = d->a_scale * d->b_scale;  // rounded once, here
    a.div_fma = !f16 && mm_fma_ok(d);
    if (bias) {
        // the product is stored under the intermediate's record, the descriptor's output record is the add's
        shl_mi355x_matmul_desc mid = *d;
        mid.out_scale = bias->mid_scale, mid.out_zp = bias->mid_zp;
        a.so = mid.out_scale, a.zo = (float)mid.out_zp, a.inv_so = 1.0f / mid.out_scale;
        a.div_fma = !f16 && mm_fma_ok(&mid);
        a.bias = bias->dev, a.bias_first = bias->first ? 1 : 0;
        a.add = add_rec(bias->mid_scale, bias->mid_zp, bias->scale, bias->zp, d->out_scale, d->out_zp);
    }
    a.tiles_m = (d->m + MM_T - 1) / MM_T, a.tiles_n = (d->n + MM_T - 1) / MM_T;
    if (form == MM_MFMA) {
        const int64_t groups = (int64_t)d->batches * a.tiles_m * a.tiles_n;  // (at most the output's element count)
        const dim3 grid((unsigned)groups), block(256);
        if (bias) hipLaunchKernelGGL((f16 ? matmul_mfma_kernel<true, true> : matmul_mfma_kernel<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL(f16 ? matmul_mfma_kernel<true> : matmul_mfma_kernel<false>, grid, block, 0, s, a);
    } else {
        const dim3 grid((unsigned)((d->out_elems + 255) / 256)), block(256);
        if (bias) hipLaunchKernelGGL((f16 ? matmul_chain_kernel<true, true> : matmul_chain_kernel<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL(f16 ? matmul_chain_kernel<true> : matmul_chain_kernel<false>, grid, block, 0, s, a);
    }
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

}  // namespace shl

extern "C" const char *shl_mi355x_matmul_kernel_name(const void *a_dev, const void *b_dev, const void *out_dev,
                                                     const struct shl_mi355x_matmul_desc *d)
{
    using namespace shl;
    if (mm_validate(a_dev, b_dev, out_dev, d)) return "";
    MmPlan p;
    mm_plan(a_dev, b_dev, d, &p);
    return mm_form_name(mm_form(d, &p));
}

extern "C" int shl_mi355x_matmul_is_exact(const struct shl_mi355x_matmul_desc *d) { return shl::mm_is_exact(d) ? 1 : 0; }

extern "C" int shl_mi355x_matmul(const void *a_dev, const void *b_dev, void *out_dev, const struct shl_mi355x_matmul_desc *d,
                                 void *stream)
{
    using namespace shl;
    const char *why = mm_validate(a_dev, b_dev, out_dev, d);
    if (why) {
        set_error("matmul: %s", why);
        return SHL_MI355X_EINVAL;
    }
    return matmul_launch(a_dev, b_dev, out_dev, d, NULL, (hipStream_t)stream);
}

extern "C" const char *shl_mi355x_matmul_bias_kernel_name(const void *a_dev, const void *b_dev, const void *bias_dev,
                                                          const void *out_dev, const struct shl_mi355x_matmul_desc *d)
{
    using namespace shl;
    if (mm_validate(a_dev, b_dev, out_dev, d) || mm_validate_bias(bias_dev, out_dev, d)) return "";
    MmPlan p;
    mm_plan(a_dev, b_dev, d, &p);
    return mm_form(d, &p) == MM_MFMA ? SHL_MI355X_MATMUL_MFMA_BIAS : SHL_MI355X_MATMUL_CHAIN_BIAS;
}

extern "C" int shl_mi355x_matmul_bias(const void *a_dev, const void *b_dev, const void *bias_dev, void *out_dev,
                                      const struct shl_mi355x_matmul_desc *d, float bias_scale, int32_t bias_zp, float mid_scale,
                                      int32_t mid_zp, int32_t bias_is_first, void *stream)
{
    using namespace shl;
    const char *why = mm_validate(a_dev, b_dev, out_dev, d);
    if (!why) why = mm_validate_bias(bias_dev, out_dev, d);
    if (why) {
        set_error("matmul_bias: %s", why);
        return SHL_MI355X_EINVAL;
    }
    const MmBias bias = {bias_dev, bias_scale, mid_scale, bias_zp, mid_zp, bias_is_first};
    return matmul_launch(a_dev, b_dev, out_dev, d, &bias, (hipStream_t)stream);
}

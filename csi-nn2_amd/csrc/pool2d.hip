// pool2d.hip -- windowed max / average pooling on quantised int8 / binary16 tensors
// (CSINN_OP_MAXPOOL2D, CSINN_OP_AVGPOOL2D).
//
// Restates shl_ref_maxpool2d_quant / shl_ref_avgpool2d_quant (source/reference/maxpool.c:21-124,
// averagepool.c:21-138), which run inside shl_ref_siso_callback_base like global_avgpool2d
// (pool_softmax.hip): dequantise -> fp32 op -> requantise.
//   geometry  window origin = out * stride - pad_top / pad_left, clamped to the image; the OUTPUT size is the
//             output tensor's (ceil_mode, pad_down and pad_right act through it only)
//   max       m = -FLT_MAX, then m = fmax(m, x) over the in-image taps in (y, x) order.  The reference's fmax is the
//             x86-64 C library's (an unordered test, then maxsd, which hands back its SECOND operand unless the
//             first compares greater): a NaN never wins, and of -0 / +0 the LAST one stays -- `x >= m ? x : m`
//             here, not v_max_f32 (which orders the zeros); tests/golden/pool_cases.npz pins it
//   avg       total += x in (y, x) order in fp32, count = in-image taps (count_include_pad: Kh * Kw),
//             total / count by IEEE division
// Nothing has a summation-order freedom: results are bit-identical to the reference for any scales.
//
// HBM-bound (ResNet-50's 3x3 stride-2 pool at batch 128: 103 MB in, 25.7 MB out).  Three forms, chosen by
// pool_form() below, which also names them:
//   nhwc_vec   NHWC with C * esize % 16 == 0: a thread owns one output pixel x one 16-byte piece of channels;
//              consecutive lanes run along the pieces, then the pixels (a wave's loads are whole lines); for
//              3x3 and 2x2 windows every in-image tap is requested before the first is used
//   nchw_row   NCHW: a thread finishes four consecutive outputs of one plane row (dwconv_channel.hip's shape),
//              flat 1-D grid over (plane, row, group of four); for the common windows a window row is fetched
//              as one span of whole dwords
//   generic    one output per thread, any C, either layout: the literal restatement
// int8 max in the first two forms is taken on the stored INTEGERS: q -> fl(fl((float)q - zp) * s) is monotone
// non-decreasing for a finite s > 0 (a correctly rounded subtraction of a constant, then a correctly rounded
// multiplication by a positive number: both monotone), so max commutes with it and one dequantise -> requantise of the
// winner finishes the output.  When the in and out records are equal and that round trip was checked to be
// the identity on all 256 values (host, per call) it is skipped.  The generic form stays literal;
// tests/test_pool2d.py runs every case through both.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"

namespace shl {

struct PoolArgs {
    const void *in;
    void *out;
    int32_t N, C, H, W, Ho, Wo;
    int32_t Kh, Kw, sh, sw, pt, pl;
    int32_t cip;       // avg: count_include_pad
    int32_t nhwc;      // generic form only
    int32_t identity;  // int8 max: requantising the winner is the identity
    float si, zi, so, zo;
};

enum { POOL_VEC = 0, POOL_ROW = 1, POOL_GENERIC = 2 };

constexpr float POOL_LOWEST = -3.402823466e+38f;  // -FLT_MAX

__device__ __forceinline__ float pool_dq(int q, const PoolArgs &a)
{
    return __fmul_rn(__fsub_rn((float)q, a.zi), a.si);  // int8_to_float_base (source/nn2/utils.c:499-502)
}

__device__ __forceinline__ int pool_rq(float v, const PoolArgs &a)
{
    return sat8_from_float(__fadd_rn(rintf(__fdiv_rn(v, a.so)), a.zo));  // float_to_int8_base (:550-560)
}

// the reference's fmax step (see the header comment)
__device__ __forceinline__ float pool_fmax(float m, float x) { return x >= m ? x : m; }

typedef short v2s __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_max_i16(uint32_t x, uint32_t y)
{
    const v2s r = __builtin_elementwise_max(__builtin_bit_cast(v2s, x), __builtin_bit_cast(v2s, y));
    return __builtin_bit_cast(uint32_t, r);
}

// the in-image part [s, e) of a window of k taps whose first tap sits at `origin` on an axis of `size`
__device__ __forceinline__ void clamp_window(int origin, int k, int size, int &s, int &e)
{
    s = origin < 0 ? -origin : 0;
    e = size - origin < k ? size - origin : k;
}

// ---- NHWC, 16 bytes of channels per thread -----------------------------------------------------------------
// Running state of one thread: int8 max keeps the sixteen bytes as 8 + 8 signed 16-bit lanes (byte << 8 keeps
// the order; v_pk_max_i16 folds two per instruction); everything else keeps one float per channel.
template <bool AVG, bool F16>
struct VecState {
    static constexpr int NF = F16 ? 8 : 16;
    float f[NF];
    uint32_t lo[4], hi[4];

    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int k = 0; k < NF; ++k) f[k] = AVG ? 0.f : POOL_LOWEST;
#pragma unroll
        for (int d = 0; d < 4; ++d) lo[d] = hi[d] = 0x80008000u;
    }

    __device__ __forceinline__ void fold(const uint4 &v, const PoolArgs &a)
    {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        if constexpr (F16) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float x = f16_bits_to_float((uint16_t)(w[k >> 1] >> (16 * (k & 1))));
                f[k] = AVG ? __fadd_rn(f[k], x) : pool_fmax(f[k], x);
            }
        } else if constexpr (AVG) {
#pragma unroll
            for (int k = 0; k < 16; ++k) f[k] = __fadd_rn(f[k], pool_dq((int8_t)(w[k >> 2] >> (8 * (k & 3))), a));
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                lo[d] = pk_max_i16(lo[d], (w[d] << 8) & 0xFF00FF00u);  // bytes 0 and 2
                hi[d] = pk_max_i16(hi[d], w[d] & 0xFF00FF00u);         // bytes 1 and 3
            }
        }
    }

    __device__ __forceinline__ uint4 finish(float count, const PoolArgs &a) const
    {
        uint32_t r[4];
        if constexpr (F16) {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const float x0 = AVG ? __fdiv_rn(f[2 * d], count) : f[2 * d];
                const float x1 = AVG ? __fdiv_rn(f[2 * d + 1], count) : f[2 * d + 1];
                r[d] = (uint32_t)float_to_f16_bits_ref(x0) | (uint32_t)float_to_f16_bits_ref(x1) << 16;
            }
        } else if constexpr (AVG) {
#pragma unroll
            for (int d = 0; d < 4; ++d)
                r[d] = pack4_i8(pool_rq(__fdiv_rn(f[4 * d], count), a), pool_rq(__fdiv_rn(f[4 * d + 1], count), a),
                                pool_rq(__fdiv_rn(f[4 * d + 2], count), a), pool_rq(__fdiv_rn(f[4 * d + 3], count), a));
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const uint32_t q = ((lo[d] >> 8) & 0x00FF00FFu) | (hi[d] & 0xFF00FF00u);  // the winners, in place
                if (a.identity) {
                    r[d] = q;
                } else {
                    r[d] = pack4_i8(pool_rq(pool_dq((int8_t)q, a), a), pool_rq(pool_dq((int8_t)(q >> 8), a), a),
                                    pool_rq(pool_dq((int8_t)(q >> 16), a), a), pool_rq(pool_dq((int8_t)(q >> 24), a), a));
                }
            }
        }
        return make_uint4(r[0], r[1], r[2], r[3]);
    }
};

// KH, KW > 0: the window's size, taps unrolled and all requested up front; KH == 0: any window, a loop
template <int KH, int KW, bool AVG, bool F16>
__global__ __launch_bounds__(256) void pool2d_nhwc_vec_kernel(PoolArgs a, int pieces, int64_t items)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (n, oy, ox, piece), piece fastest
    if (i >= items) return;
    const int64_t pix = i / pieces;
    const int piece = (int)(i - pix * pieces);
    const int64_t t = pix / a.Wo;
    const int ox = (int)(pix - t * a.Wo);
    const int64_t n = t / a.Ho;
    const int oy = (int)(t - n * a.Ho);
    const int y0 = oy * a.sh - a.pt, x0 = ox * a.sw - a.pl;
    int ys, ye, xs, xe;
    clamp_window(y0, KH ? KH : a.Kh, a.H, ys, ye);
    clamp_window(x0, KW ? KW : a.Kw, a.W, xs, xe);
    const uint4 *in = static_cast<const uint4 *>(a.in);
    const int64_t base = (n * a.H * a.W) * pieces + piece;  // pixel (n, 0, 0)
    VecState<AVG, F16> st;
    st.init();
    if constexpr (KH > 0) {
        uint4 v[KH * KW];
#pragma unroll
        for (int ky = 0; ky < KH; ++ky)
#pragma unroll
            for (int kx = 0; kx < KW; ++kx)
                if (ky >= ys && ky < ye && kx >= xs && kx < xe)
                    v[ky * KW + kx] = in[base + ((int64_t)(y0 + ky) * a.W + (x0 + kx)) * pieces];
#pragma unroll
        for (int ky = 0; ky < KH; ++ky)
#pragma unroll
            for (int kx = 0; kx < KW; ++kx)
                if (ky >= ys && ky < ye && kx >= xs && kx < xe) st.fold(v[ky * KW + kx], a);
    } else {
        for (int ky = ys; ky < ye; ++ky)
            for (int kx = xs; kx < xe; ++kx) st.fold(in[base + ((int64_t)(y0 + ky) * a.W + (x0 + kx)) * pieces], a);
    }
    const float count = a.cip ? (float)(a.Kh * a.Kw) : (float)((ye - ys) * (xe - xs));
    static_cast<uint4 *>(a.out)[i] = st.finish(count, a);
}

// ---- one output, literally ---------------------------------------------------------------------------------
// `in` points at the window's plane (NCHW) or at the image's channel (NHWC); xstep / ystep in elements
// Q_DOMAIN: the int8 max is taken on the stored integers (header comment); v: the stored element (f16 bits / int8)
template <bool AVG, bool F16, bool Q_DOMAIN>
struct OneState {
    float acc = AVG ? 0.f : POOL_LOWEST;
    int qmax = -128;

    __device__ __forceinline__ void fold(uint32_t v, const PoolArgs &a)
    {
        if constexpr (F16) {
            const float x = f16_bits_to_float((uint16_t)v);
            acc = AVG ? __fadd_rn(acc, x) : pool_fmax(acc, x);
        } else {
            const int q = (int8_t)v;
            if constexpr (AVG) acc = __fadd_rn(acc, pool_dq(q, a));
            else if constexpr (Q_DOMAIN) qmax = q > qmax ? q : qmax;
            else acc = pool_fmax(acc, pool_dq(q, a));
        }
    }

    // in_image: the window's taps inside the image
    __device__ __forceinline__ uint32_t finish(int in_image, const PoolArgs &a) const
    {
        float r = acc;
        if constexpr (AVG) r = __fdiv_rn(r, a.cip ? (float)(a.Kh * a.Kw) : (float)in_image);
        if constexpr (F16) return float_to_f16_bits_ref(r);
        if constexpr (!AVG && Q_DOMAIN) {
            if (a.identity) return (uint32_t)qmax & 0xFFu;
            r = pool_dq(qmax, a);
        }
        return (uint32_t)pool_rq(r, a) & 0xFFu;
    }
};

template <bool AVG, bool F16, bool Q_DOMAIN>
__device__ __forceinline__ uint32_t pool_one(const void *in, int64_t ystep, int64_t xstep, int y0, int x0, int ys, int ye,
                                             int xs, int xe, const PoolArgs &a)
{
    OneState<AVG, F16, Q_DOMAIN> st;
    for (int ky = ys; ky < ye; ++ky) {
        for (int kx = xs; kx < xe; ++kx) {
            const int64_t off = (y0 + ky) * ystep + (x0 + kx) * xstep;
            if constexpr (F16) st.fold(static_cast<const uint16_t *>(in)[off], a);
            else st.fold((uint32_t)static_cast<const int8_t *>(in)[off], a);
        }
    }
    return st.finish((ye - ys) * (xe - xs), a);
}

// ---- NCHW, four consecutive outputs of a plane row per thread ----------------------------------------------
// KW, SW > 0 (the window's width and the column stride, known at compile time): a window row is fetched as the span of
// 3 SW + KW input columns under the four windows, in whole dwords at whatever byte address (3 loads instead of 12 byte
// loads for int8 3x3 stride 2; 5 instead of 12 for binary16), and the taps are picked from registers.  EVERY group of a
// row takes this path, the first and the last one too -- a wave that ran a tap-by-tap path for its edge groups beside
// the span path paid for both (measured, profiles/pool2d_notes.md).  A span that sticks out of the image row reads the
// neighbouring row's bytes (never used: each tap is predicated on its column); only a dword that would leave the
// TENSOR -- in front of its first row, behind its last -- is assembled from the bytes that exist.
// KW == 0: any other window, tap by tap.
template <int KW, int SW, bool AVG, bool F16>
__global__ __launch_bounds__(256) void pool2d_nchw_row_kernel(PoolArgs a, int groups_per_row, int64_t items)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (plane, oy, group of four), group fastest
    if (i >= items) return;
    const int64_t row = i / groups_per_row;
    const int ox0 = (int)(i - row * groups_per_row) * 4;
    const int64_t plane = row / a.Ho;  // n * C + c
    const int oy = (int)(row - plane * a.Ho);
    const int y0 = oy * a.sh - a.pt;
    int ys, ye;
    clamp_window(y0, a.Kh, a.H, ys, ye);
    constexpr int ES = F16 ? 2 : 1;
    uint32_t r[4] = {0, 0, 0, 0};
    if constexpr (KW > 0) {
        constexpr int SPAN = 3 * SW + KW;  // input columns under the four windows
        constexpr int EPD = 4 / ES;        // elements per dword
        constexpr int NDW = (SPAN + EPD - 1) / EPD;
        constexpr int BITS = 8 * ES;
        const int xl = ox0 * SW - a.pl;    // first column of the span
        const int64_t total = (int64_t)a.N * a.C * a.H * a.W * ES;  // the tensor's bytes
        const char *base = static_cast<const char *>(a.in);
        int xs[4], xe[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            clamp_window(xl + e * SW, KW, a.W, xs[e], xe[e]);
            if (ox0 + e >= a.Wo) xe[e] = xs[e] = 0;  // no such output
        }
        OneState<AVG, F16, true> st[4];
        for (int ky = ys; ky < ye; ++ky) {
            const int64_t boff = ((plane * a.H + (y0 + ky)) * a.W + xl) * ES;  // the span's first byte in the tensor
            uint32_t dw[NDW];
#pragma unroll
            for (int d = 0; d < NDW; ++d) {
                const int64_t b0 = boff + 4 * d;
                if (b0 >= 0 && b0 + 4 <= total) {
                    typedef uint32_t u1_a1 __attribute__((aligned(1)));
                    dw[d] = *reinterpret_cast<const u1_a1 *>(base + b0);
                } else {
                    dw[d] = 0;
                    for (int j = 0; j < 4; ++j)
                        if (b0 + j >= 0 && b0 + j < total) dw[d] |= (uint32_t)(uint8_t)base[b0 + j] << (8 * j);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int kx = 0; kx < KW; ++kx) {
                    const int idx = e * SW + kx;
                    if (kx >= xs[e] && kx < xe[e]) st[e].fold(dw[idx / EPD] >> (BITS * (idx % EPD)), a);
                }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = st[e].finish((ye - ys) * (xe[e] - xs[e]), a);
    } else {
        const char *in = static_cast<const char *>(a.in) + plane * a.H * a.W * ES;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (ox0 + e < a.Wo) {
                const int x0 = (ox0 + e) * a.sw - a.pl;
                int xs, xe;
                clamp_window(x0, a.Kw, a.W, xs, xe);
                r[e] = pool_one<AVG, F16, true>(in, a.W, 1, y0, x0, ys, ye, xs, xe, a);
            }
        }
    }
    const int64_t o = row * a.Wo + ox0;  // element index of the first output
    const int left = a.Wo - ox0;
    if constexpr (F16) {
        uint16_t *dst = static_cast<uint16_t *>(a.out) + o;
        if (left >= 4 && ((uintptr_t)dst & 3) == 0) {
            reinterpret_cast<uint32_t *>(dst)[0] = r[0] | r[1] << 16;
            reinterpret_cast<uint32_t *>(dst)[1] = r[2] | r[3] << 16;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < left) dst[e] = (uint16_t)r[e];
        }
    } else {
        int8_t *dst = static_cast<int8_t *>(a.out) + o;
        if (left >= 4) {
            typedef uint32_t u1_a1 __attribute__((aligned(1)));  // one packed store at whatever byte address
            *reinterpret_cast<u1_a1 *>(dst) = r[0] | r[1] << 8 | r[2] << 16 | r[3] << 24;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < left) dst[e] = (int8_t)r[e];
        }
    }
}

// ---- any C, either layout, one output per thread -----------------------------------------------------------
template <bool AVG, bool F16>
__global__ __launch_bounds__(256) void pool2d_generic_kernel(PoolArgs a, int64_t items)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // the output element, in the tensor's own order
    if (i >= items) return;
    int64_t n, t;
    int c, oy, ox;
    if (a.nhwc) {
        t = i / a.C, c = (int)(i - t * a.C);
        n = t / a.Wo, ox = (int)(t - n * a.Wo);
        t = n, n = t / a.Ho, oy = (int)(t - n * a.Ho);
    } else {
        t = i / a.Wo, ox = (int)(i - t * a.Wo);
        n = t / a.Ho, oy = (int)(t - n * a.Ho);
        t = n, n = t / a.C, c = (int)(t - n * a.C);
    }
    const int y0 = oy * a.sh - a.pt, x0 = ox * a.sw - a.pl;
    int ys, ye, xs, xe;
    clamp_window(y0, a.Kh, a.H, ys, ye);
    clamp_window(x0, a.Kw, a.W, xs, xe);
    constexpr int ES = F16 ? 2 : 1;
    const int64_t first = a.nhwc ? n * a.H * a.W * a.C + c : (n * a.C + c) * a.H * a.W;
    const int64_t xstep = a.nhwc ? a.C : 1;
    const uint32_t r = pool_one<AVG, F16, false>(static_cast<const char *>(a.in) + first * ES, xstep * a.W, xstep, y0, x0, ys,
                                                 ye, xs, xe, a);
    if constexpr (F16) static_cast<uint16_t *>(a.out)[i] = (uint16_t)r;
    else static_cast<int8_t *>(a.out)[i] = (int8_t)r;
}

// ---- host side ---------------------------------------------------------------------------------------------
static bool pool_desc_ok(const shl_mi355x_pool_desc *d)
{
    return d && (d->kind == SHL_MI355X_POOL_MAX || d->kind == SHL_MI355X_POOL_AVG) &&
           (d->dtype == SHL_MI355X_I8 || d->dtype == SHL_MI355X_F16) &&
           (d->layout == SHL_MI355X_NHWC || d->layout == SHL_MI355X_NCHW) && d->batch >= 0 && d->c > 0 && d->in_h > 0 &&
           d->in_w > 0 && d->out_h > 0 && d->out_w > 0 && d->kernel_h > 0 && d->kernel_w > 0 && d->stride_h > 0 &&
           d->stride_w > 0;
}

// The one place that chooses the form (launch and name).  SHL_MI355X_POOL_FORM=generic forces the literal
// form (A/B runs, tests); read per call.
static int pool_form(const shl_mi355x_pool_desc *d)
{
    const char *force = getenv("SHL_MI355X_POOL_FORM");
    if (force && strcmp(force, "generic") == 0) return POOL_GENERIC;
    // the integer-domain max needs a monotone dequantisation: a finite scale > 0
    if (d->kind == SHL_MI355X_POOL_MAX && d->dtype == SHL_MI355X_I8 && !(d->in_scale > 0.f && d->in_scale < INFINITY))
        return POOL_GENERIC;
    if (d->layout == SHL_MI355X_NCHW) return POOL_ROW;
    const int esize = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    return ((int64_t)d->c * esize) % 16 == 0 ? POOL_VEC : POOL_GENERIC;
}

// is requantising a dequantised value the identity for every int8 value?  (only asked for equal records; the movers
// ask too: requant_move.h:move_rec)
bool requant_is_identity(float s, int32_t zp)
{
    const float z = (float)zp;
    for (int q = -128; q < 128; ++q) {
        const float x = ((float)q - z) * s;  // (this file is compiled without contraction)
        float r = rintf(x / s) + z;
        r = r > 127.0f ? 127.0f : r;
        r = r < -128.0f ? -128.0f : r;
        if (!(r == r) || (int)r != q) return false;
    }
    return true;
}

// every output's window must hold at least one input element: the reference yields -FLT_MAX / 0 / 0 there
static bool axis_covered(int out, int stride, int pad, int k, int size, int *bad)
{
    for (int o = 0; o < out; ++o) {
        const int64_t origin = (int64_t)o * stride - pad;
        const int64_t s = origin < 0 ? -origin : 0, e = size - origin < k ? size - origin : k;
        if (e <= s) {
            *bad = o;
            return false;
        }
    }
    return true;
}

template <bool AVG, bool F16>
static void (*pick_row(int kw, int sw))(PoolArgs, int, int64_t)
{
    if (kw == 3 && sw == 2) return pool2d_nchw_row_kernel<3, 2, AVG, F16>;
    if (kw == 2 && sw == 2) return pool2d_nchw_row_kernel<2, 2, AVG, F16>;
    if (kw == 3 && sw == 1) return pool2d_nchw_row_kernel<3, 1, AVG, F16>;
    return pool2d_nchw_row_kernel<0, 0, AVG, F16>;
}

template <bool AVG, bool F16>
static void (*pick_vec(int kh, int kw))(PoolArgs, int, int64_t)
{
    if (kh == 3 && kw == 3) return pool2d_nhwc_vec_kernel<3, 3, AVG, F16>;
    if (kh == 2 && kw == 2) return pool2d_nhwc_vec_kernel<2, 2, AVG, F16>;
    return pool2d_nhwc_vec_kernel<0, 0, AVG, F16>;
}

}  // namespace shl

extern "C" const char *shl_mi355x_pool2d_kernel_name(const struct shl_mi355x_pool_desc *d)
{
    if (!shl::pool_desc_ok(d)) return "";
    switch (shl::pool_form(d)) {
        case shl::POOL_VEC: return "pool2d_nhwc_vec";
        case shl::POOL_ROW: return "pool2d_nchw_row";
        default: return "pool2d_generic";
    }
}

extern "C" int shl_mi355x_pool2d(const void *in_dev, void *out_dev, const struct shl_mi355x_pool_desc *d, void *stream)
{
    using namespace shl;
    if (!in_dev || !out_dev || !pool_desc_ok(d)) {
        set_error("pool2d: invalid argument");
        return SHL_MI355X_EINVAL;
    }
    int bad = 0;
    if (!axis_covered(d->out_h, d->stride_h, d->pad_top, d->kernel_h, d->in_h, &bad)) {
        set_error("pool2d: the window of output row %d holds no input element", bad);
        return SHL_MI355X_EINVAL;
    }
    if (!axis_covered(d->out_w, d->stride_w, d->pad_left, d->kernel_w, d->in_w, &bad)) {
        set_error("pool2d: the window of output column %d holds no input element", bad);
        return SHL_MI355X_EINVAL;
    }
    if ((int64_t)d->kernel_h * d->kernel_w > (1 << 24)) {
        set_error("pool2d: window too large");
        return SHL_MI355X_ENOTSUP;
    }
    if (d->batch == 0) return SHL_MI355X_OK;
    const bool avg = d->kind == SHL_MI355X_POOL_AVG, f16 = d->dtype == SHL_MI355X_F16;
    PoolArgs a;
    a.in = in_dev, a.out = out_dev;
    a.N = d->batch, a.C = d->c, a.H = d->in_h, a.W = d->in_w, a.Ho = d->out_h, a.Wo = d->out_w;
    a.Kh = d->kernel_h, a.Kw = d->kernel_w, a.sh = d->stride_h, a.sw = d->stride_w, a.pt = d->pad_top, a.pl = d->pad_left;
    a.cip = d->count_include_pad ? 1 : 0;
    a.nhwc = d->layout == SHL_MI355X_NHWC ? 1 : 0;
    a.si = d->in_scale, a.zi = (float)d->in_zp, a.so = d->out_scale, a.zo = (float)d->out_zp;
    const int form = pool_form(d);
    a.identity = !avg && !f16 && form != POOL_GENERIC && d->in_zp == d->out_zp &&
                 memcmp(&d->in_scale, &d->out_scale, sizeof(float)) == 0 && requant_is_identity(d->in_scale, d->in_zp);
    const int64_t outputs = (int64_t)d->batch * d->c * d->out_h * d->out_w;
    int64_t items;
    if (form == POOL_VEC) {
        if ((((uintptr_t)in_dev | (uintptr_t)out_dev) & 15) != 0) {
            set_error("pool2d: NHWC buffers must be 16-byte aligned");
            return SHL_MI355X_EINVAL;
        }
        items = outputs / (f16 ? 8 : 16);
    } else if (form == POOL_ROW) {
        items = (int64_t)d->batch * d->c * d->out_h * ((d->out_w + 3) / 4);
    } else {
        items = outputs;
    }
    const int64_t blocks = (items + 255) / 256;
    if (blocks > 0x7FFFFFFFll) {
        set_error("pool2d: %lld workgroups exceed the grid", (long long)blocks);
        return SHL_MI355X_ENOTSUP;
    }
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (form == POOL_VEC) {
        const int pieces = (int)((int64_t)d->c * (f16 ? 2 : 1) / 16);
        auto k = avg ? (f16 ? pick_vec<true, true>(a.Kh, a.Kw) : pick_vec<true, false>(a.Kh, a.Kw))
                     : (f16 ? pick_vec<false, true>(a.Kh, a.Kw) : pick_vec<false, false>(a.Kh, a.Kw));
        hipLaunchKernelGGL(k, grid, block, 0, s, a, pieces, items);
    } else if (form == POOL_ROW) {
        auto k = avg ? (f16 ? pick_row<true, true>(a.Kw, a.sw) : pick_row<true, false>(a.Kw, a.sw))
                     : (f16 ? pick_row<false, true>(a.Kw, a.sw) : pick_row<false, false>(a.Kw, a.sw));
        hipLaunchKernelGGL(k, grid, block, 0, s, a, (d->out_w + 3) / 4, items);
    } else {
        auto k = avg ? (f16 ? pool2d_generic_kernel<true, true> : pool2d_generic_kernel<true, false>)
                     : (f16 ? pool2d_generic_kernel<false, true> : pool2d_generic_kernel<false, false>);
        hipLaunchKernelGGL(k, grid, block, 0, s, a, items);
    }
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

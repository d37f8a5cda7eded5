// resize.hip -- nearest-neighbour and bilinear resize of 4-d int8 / binary16 tensors (CSINN_OP_RESIZE), NHWC and NCHW.
//
// Restates shl_ref_resize_quant (source/reference/resize.c:464-468 inside shl_ref_siso_callback_base): the input is
// converted to float32 with its record, resized in float32, and converted to the output's dtype with the output's record.
//   scale     height_scale = (float)in_h / out_h, with align_corners (float)(in_h - 1) / (out_h - 1); the same for the
//             width.  ONE float division each, made on the host and handed over in the descriptor.
//   source    input_y = y * height_scale: one float product (__fmul_rn: nothing may contract it into a neighbour)
//   nearest   in_y = min((int)floor(input_y), in_h - 1); with align_corners (int)round(input_y), halves away from zero.
//             A pure gather: out = requantise(dequantise(in)).  int8: a 256-entry table built on the host
//             (shl_mi355x_resize_table_i8), by value in the kernel arguments, held in LDS; a byte copy when the records
//             are equal and the round trip was checked on all 256 values.  binary16: the two rules of
//             float16 -> float32 -> float32_to_float16_base (+-inf -> +-65504, NaN -> 0x7FFF / 0xFFFF), as concat's.
//   bilinear  y0 = floor(input_y), y1 = min(y0 + 1, in_h - 1), dy = input_y - y0, the same along x;
//             out = v00 (1-dy) (1-dx) + v10 dy (1-dx) + v01 (1-dy) dx + v11 dy dx, every product (v w_y) w_x, summed in
//             that order in float32.  The reference's build (-O3 -mfma) fuses all three additions, the first one with the
//             second multiplication of the FIRST term: t = (v10 dy) (1-dx); t = fma(v00 (1-dy), 1-dx, t);
//             t = fma(v01 (1-dy), dx, t); t = fma(v11 dy, dx, t) -- settled by the genuine library's float32 outputs
//             (the only one of the twelve candidates that matches them on every element), spelled out here
//             with __fmaf_rn.  No tap is skipped at weight zero: an infinity under a zero weight gives a NaN, as it does
//             there.  A NaN reaches binary16 as 0x7FFF with a sign: an operand NaN keeps its sign through the x86
//             operations, a NaN the arithmetic makes itself (inf * 0, inf - inf) is x86's default one, sign bit set, and
//             of several the fused multiply-adds hand on their product operand's before their addend's (bilinear_f16).
// The reference's NCHW nearest routines advance the output by the INPUT's batch size per image (resize.c:179, :397); here
// every image is computed on its own.
//
// Three forms, chosen by resize_form() below, which also names them:
//   nhwc_vec  16 bytes of one output pixel's channel vector per thread (16 int8 / 8 binary16 channels), in output
//             order.  Lanes run along the pieces of a pixel (blockDim.x, a power of two) then along the pixels of a row
//             (blockDim.y); the row and the image are blockIdx.y / .z: no thread divides by a run-time value.  Nearest:
//             one 16-byte load, a copy / sixteen table look-ups / the binary16 fix-up, one 16-byte store; bilinear: four
//             16-byte loads, 16 or 8 results, one store.  Needs C * element size % 16 == 0 and both pointers on the
//             16-byte grid.
//   nchw_row  a workgroup walks output rows of one (n, c) plane, lanes along x; a thread owns the outputs that share one
//             aligned dword of the output (4 int8 / 2 binary16) and stores them as that dword; only a row's first and last
//             group, when the row does not start or end on a dword, fall back to single stores.  Needs the output
//             pointer on the 4-byte grid; the input may lie anywhere (it is gathered element by element).
//   generic   one output per thread, any layout, channel count and alignment: the literal formula
//             (SHL_MI355X_RESIZE_FORM=generic forces it) -- tests/test_resize.py runs the geometry cases through it too.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "common.h"

namespace shl {

bool requant_is_identity(float s, int32_t zp);  // pool2d.hip

enum { RESIZE_VEC = 0, RESIZE_ROW = 1, RESIZE_GENERIC = 2 };
enum { OP_COPY = 0, OP_LUT = 1, OP_BILINEAR = 2 };  // nearest without / with the int8 table, bilinear

struct ResizeArgs {
    uint32_t tab[64];  // FIRST: the int8 nearest table, entry of byte b = byte b & 3 of tab[b >> 2] (see lut_load)
    const void *in;
    void *out;
    int32_t n, c, ih, iw, oh, ow;
    float hs, ws;       // height_scale, width_scale
    int32_t align;      // align_corners
    int32_t nchw;       // generic form: the layout
    int32_t pieces;     // vec form: 16-byte pieces per pixel
    int32_t piece_blocks;  // vec form: workgroups along the pieces (1 unless a pixel has more than 256 pieces)
    int32_t rows_per_wg;   // row form: output rows one workgroup walks
    float si, zi, so, zo, inv_so;
    int32_t fma_div;    // div_by_scale is exact for every value these records can give
};

// the table is the first kernel argument: thread t < 64 copies dword t of the argument block to LDS (indexing the by-value
// struct with a lane id would send it through scratch)
__device__ __forceinline__ void lut_load(uint32_t *lds)
{
    typedef const __attribute__((address_space(4))) uint32_t *kernarg_words;
    const unsigned t = threadIdx.y * blockDim.x + threadIdx.x;
    if (t < 64) lds[t] = ((kernarg_words)__builtin_amdgcn_kernarg_segment_ptr())[t];
    __syncthreads();
}

__device__ __forceinline__ uint32_t lut_word(const uint8_t *lut, uint32_t v)
{
    const uint32_t b0 = lut[v & 0xFFu], b1 = lut[(v >> 8) & 0xFFu], b2 = lut[(v >> 16) & 0xFFu], b3 = lut[v >> 24];
    return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

// one binary16 value through float16 -> float32 -> float32_to_float16_base: +-inf -> +-65504, a NaN -> 0x7FFF with its sign
__device__ __forceinline__ uint32_t fix_f16(uint32_t h)
{
    const uint32_t m = h & 0x7FFFu;
    return m < 0x7C00u ? h : ((h & 0x8000u) | (m == 0x7C00u ? 0x7BFFu : 0x7FFFu));
}

__device__ __forceinline__ uint32_t fix_f16x2(uint32_t w)
{
    if ((((w & 0x7FFF7FFFu) + 0x04000400u) & 0x80008000u) == 0u) return w;  // neither half reaches 0x7C00
    return fix_f16(w & 0xFFFFu) | (fix_f16(w >> 16) << 16);
}

// the source row / column of output row / column `o` for the nearest mode
__device__ __forceinline__ int nearest_index(int o, float scale, int align, int in)
{
    const float s = __fmul_rn((float)o, scale);
    const int i = (int)fminf(align ? roundf(s) : floorf(s), 0x1p30f);  // round(): halves away from zero
    return max(0, min(i, in - 1));
}

// the two source rows / columns and the weight of the second for the bilinear mode
struct Tap {
    int i0, i1;
    float w0, w1;
};

__device__ __forceinline__ Tap bilinear_tap(int o, float scale, int in)
{
    const float s = __fmul_rn((float)o, scale);
    const int f = (int)fminf(floorf(s), 0x1p30f);
    Tap t;
    t.w1 = __fsub_rn(s, (float)f);
    t.w0 = __fsub_rn(1.0f, t.w1);
    t.i0 = max(0, min(f, in - 1));  // (f is inside the image for every scale the host computes)
    t.i1 = max(0, min(f + 1, in - 1));
    return t;
}

// v00 = (y0, x0), v10 = (y1, x0), v01 = (y0, x1), v11 = (y1, x1): the reference's order of terms and its build's fusion
__device__ __forceinline__ float bilinear_f32(float v00, float v10, float v01, float v11, const Tap &ty, const Tap &tx)
{
    float t = __fmul_rn(__fmul_rn(v10, ty.w1), tx.w0);
    t = __fmaf_rn(__fmul_rn(v00, ty.w0), tx.w0, t);
    t = __fmaf_rn(__fmul_rn(v01, ty.w0), tx.w1, t);
    return __fmaf_rn(__fmul_rn(v11, ty.w1), tx.w1, t);
}

__device__ __forceinline__ int bilinear_i8(int q00, int q10, int q01, int q11, const Tap &ty, const Tap &tx, const ResizeArgs &a)
{
    // int8_to_float_base (source/nn2/utils.c:499-502), float_to_int8_base (:550-560)
    const float r = bilinear_f32(__fmul_rn(__fsub_rn((float)q00, a.zi), a.si), __fmul_rn(__fsub_rn((float)q10, a.zi), a.si),
                                 __fmul_rn(__fsub_rn((float)q01, a.zi), a.si), __fmul_rn(__fsub_rn((float)q11, a.zi), a.si), ty, tx);
    const float d = a.fma_div ? div_by_scale(r, a.so, a.inv_so) : __fdiv_rn(r, a.so);
    return sat8_from_float(__fadd_rn(rintf(d), a.zo));
}

// is the operand a term hands to its fused multiply-add -- v w_y, for the (y1, x0) term (v w_y) w_x, pass wx = 1 otherwise --
// a NaN, and with which sign?  0: no NaN; 1: a positive NaN; 2: a negative one.  An operand NaN keeps its sign; inf * 0
// makes x86's default NaN, whose sign bit is set
__device__ __forceinline__ int term_nan(uint32_t h, float v, float wy, float wx)
{
    if ((h & 0x7FFFu) > 0x7C00u) return (h & 0x8000u) ? 2 : 1;
    const float p = __fmul_rn(__fmul_rn(v, wy), wx);
    return p != p ? 2 : 0;
}

__device__ __forceinline__ uint32_t bilinear_f16(uint32_t h00, uint32_t h10, uint32_t h01, uint32_t h11, const Tap &ty, const Tap &tx)
{
    const float v00 = f16_bits_to_float((uint16_t)h00), v10 = f16_bits_to_float((uint16_t)h10);
    const float v01 = f16_bits_to_float((uint16_t)h01), v11 = f16_bits_to_float((uint16_t)h11);
    const float r = bilinear_f32(v00, v10, v01, v11, ty, tx);
    if (r != r) {
        // float32_to_float16_base keeps a NaN's sign only.  An x86 fused multiply-add hands on the NaN of its product
        // operand (v w_y, computed by a multiplication of its own) before its addend's, so the LAST such operand in
        // the chain wins, and the (y1, x0) term, the first addend, comes last; a NaN that only a fused operation makes
        // (inf * 0 inside it, inf - inf) is the default one, and yields to any operand NaN
        int s = term_nan(h11, v11, ty.w1, 1.0f);
        if (!s) s = term_nan(h01, v01, ty.w0, 1.0f);
        if (!s) s = term_nan(h00, v00, ty.w0, 1.0f);
        if (!s) s = term_nan(h10, v10, ty.w1, tx.w0);
        return s == 1 ? 0x7FFFu : 0xFFFFu;
    }
    return float_to_f16_bits_ref(r);
}

// ------------------------------------------------------------------------------------------ NHWC, 16 bytes per thread
template <bool F16>
__device__ __forceinline__ uint32_t bilinear_word(uint32_t w00, uint32_t w10, uint32_t w01, uint32_t w11, const Tap &ty, const Tap &tx,
                                                  const ResizeArgs &a)
{
    if constexpr (F16) {
        return bilinear_f16(w00 & 0xFFFFu, w10 & 0xFFFFu, w01 & 0xFFFFu, w11 & 0xFFFFu, ty, tx) |
               (bilinear_f16(w00 >> 16, w10 >> 16, w01 >> 16, w11 >> 16, ty, tx) << 16);
    } else {
        return pack4_i8(bilinear_i8((int8_t)w00, (int8_t)w10, (int8_t)w01, (int8_t)w11, ty, tx, a),
                        bilinear_i8((int8_t)(w00 >> 8), (int8_t)(w10 >> 8), (int8_t)(w01 >> 8), (int8_t)(w11 >> 8), ty, tx, a),
                        bilinear_i8((int8_t)(w00 >> 16), (int8_t)(w10 >> 16), (int8_t)(w01 >> 16), (int8_t)(w11 >> 16), ty, tx, a),
                        bilinear_i8((int8_t)(w00 >> 24), (int8_t)(w10 >> 24), (int8_t)(w01 >> 24), (int8_t)(w11 >> 24), ty, tx, a));
    }
}

template <bool F16, int OP>
__global__ __launch_bounds__(256) void resize_nhwc_vec_kernel(ResizeArgs a)
{
    __shared__ uint32_t lds[64];
    if constexpr (OP == OP_LUT) lut_load(lds);
    // blockIdx.x = (block of pixels of the row, block of pieces of a pixel); the second is 0 unless C is huge
    const unsigned pb = a.piece_blocks == 1 ? 0u : blockIdx.x % (unsigned)a.piece_blocks;
    const unsigned xb = a.piece_blocks == 1 ? blockIdx.x : blockIdx.x / (unsigned)a.piece_blocks;
    const int p = (int)(pb * blockDim.x + threadIdx.x);
    const int ox = (int)(xb * blockDim.y + threadIdx.y);
    if (p >= a.pieces || ox >= a.ow) return;
    const int oy = blockIdx.y, n = blockIdx.z;
    const int64_t P = a.pieces;
    const uint4 *in = static_cast<const uint4 *>(a.in) + (int64_t)n * a.ih * a.iw * P + p;
    uint4 *out = static_cast<uint4 *>(a.out) + (((int64_t)n * a.oh + oy) * a.ow + ox) * P + p;
    if constexpr (OP == OP_BILINEAR) {
        const Tap ty = bilinear_tap(oy, a.hs, a.ih), tx = bilinear_tap(ox, a.ws, a.iw);
        const uint4 v00 = in[((int64_t)ty.i0 * a.iw + tx.i0) * P], v10 = in[((int64_t)ty.i1 * a.iw + tx.i0) * P];
        const uint4 v01 = in[((int64_t)ty.i0 * a.iw + tx.i1) * P], v11 = in[((int64_t)ty.i1 * a.iw + tx.i1) * P];
        uint4 r;
        r.x = bilinear_word<F16>(v00.x, v10.x, v01.x, v11.x, ty, tx, a);
        r.y = bilinear_word<F16>(v00.y, v10.y, v01.y, v11.y, ty, tx, a);
        r.z = bilinear_word<F16>(v00.z, v10.z, v01.z, v11.z, ty, tx, a);
        r.w = bilinear_word<F16>(v00.w, v10.w, v01.w, v11.w, ty, tx, a);
        *out = r;
    } else {
        const int iy = nearest_index(oy, a.hs, a.align, a.ih), ix = nearest_index(ox, a.ws, a.align, a.iw);
        uint4 v = in[((int64_t)iy * a.iw + ix) * P];
        if constexpr (F16) {
            v.x = fix_f16x2(v.x), v.y = fix_f16x2(v.y), v.z = fix_f16x2(v.z), v.w = fix_f16x2(v.w);
        } else if constexpr (OP == OP_LUT) {
            const uint8_t *lut = reinterpret_cast<const uint8_t *>(lds);
            v.x = lut_word(lut, v.x), v.y = lut_word(lut, v.y), v.z = lut_word(lut, v.z), v.w = lut_word(lut, v.w);
        }
        *out = v;
    }
}

// ------------------------------------------------------------------------------------------ one output, any layout
// the output element at (oy, ox) of a plane whose elements are `stride` apart (NHWC: C, NCHW: 1), as bits
template <bool F16, int OP, typename T>
__device__ __forceinline__ uint32_t resize_one(const T *in, int64_t stride, int oy, int ox, const ResizeArgs &a, const uint8_t *lut)
{
    if constexpr (OP == OP_BILINEAR) {
        const Tap ty = bilinear_tap(oy, a.hs, a.ih), tx = bilinear_tap(ox, a.ws, a.iw);
        const T v00 = in[((int64_t)ty.i0 * a.iw + tx.i0) * stride], v10 = in[((int64_t)ty.i1 * a.iw + tx.i0) * stride];
        const T v01 = in[((int64_t)ty.i0 * a.iw + tx.i1) * stride], v11 = in[((int64_t)ty.i1 * a.iw + tx.i1) * stride];
        if constexpr (F16) return bilinear_f16(v00, v10, v01, v11, ty, tx);
        else return (uint32_t)(uint8_t)bilinear_i8(v00, v10, v01, v11, ty, tx, a);
    } else {
        const int iy = nearest_index(oy, a.hs, a.align, a.ih), ix = nearest_index(ox, a.ws, a.align, a.iw);
        const T v = in[((int64_t)iy * a.iw + ix) * stride];
        if constexpr (F16) return fix_f16(v);
        else if constexpr (OP == OP_LUT) return lut[(uint8_t)v];
        else return (uint32_t)(uint8_t)v;
    }
}

template <bool F16, int OP>
__global__ __launch_bounds__(256) void resize_generic_kernel(ResizeArgs a)
{
    typedef typename std::conditional<F16, uint16_t, int8_t>::type T;
    __shared__ uint32_t lds[64];
    if constexpr (OP == OP_LUT) lut_load(lds);
    const int64_t total = (int64_t)a.n * a.c * a.oh * a.ow;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    int n, c, oy, ox;
    int64_t r = e;
    if (a.nchw) {
        ox = (int)(r % a.ow), r /= a.ow;
        oy = (int)(r % a.oh), r /= a.oh;
        c = (int)(r % a.c), n = (int)(r / a.c);
    } else {
        c = (int)(r % a.c), r /= a.c;
        ox = (int)(r % a.ow), r /= a.ow;
        oy = (int)(r % a.oh), n = (int)(r / a.oh);
    }
    const int64_t image = (int64_t)a.ih * a.iw * a.c;
    const T *in = static_cast<const T *>(a.in) + n * image + (a.nchw ? (int64_t)c * a.ih * a.iw : (int64_t)c);
    static_cast<T *>(a.out)[e] = (T)resize_one<F16, OP, T>(in, a.nchw ? 1 : a.c, oy, ox, a, reinterpret_cast<const uint8_t *>(lds));
}

// ------------------------------------------------------------------------------------------ NCHW, rows of one plane
template <bool F16, int OP>
__global__ __launch_bounds__(256) void resize_nchw_row_kernel(ResizeArgs a)
{
    typedef typename std::conditional<F16, uint16_t, int8_t>::type T;
    constexpr int G = F16 ? 2 : 4;  // outputs per dword
    __shared__ uint32_t lds[64];
    if constexpr (OP == OP_LUT) lut_load(lds);
    const uint8_t *lut = reinterpret_cast<const uint8_t *>(lds);
    const int64_t plane = blockIdx.x;  // n * C + c
    const T *in = static_cast<const T *>(a.in) + plane * a.ih * a.iw;
    T *out = static_cast<T *>(a.out) + plane * a.oh * a.ow;
    const int r0 = blockIdx.y * a.rows_per_wg, r1 = min(a.oh, r0 + a.rows_per_wg);
    for (int oy = r0 + (int)threadIdx.y; oy < r1; oy += blockDim.y) {
        T *orow = out + (int64_t)oy * a.ow;
        // group g holds the outputs of the g-th aligned dword the row touches: columns g G - lead .. g G - lead + G - 1
        const int lead = (int)(((uintptr_t)orow & 3u) / sizeof(T));
        const int groups = (a.ow + lead + G - 1) / G;
        for (int g = threadIdx.x; g < groups; g += blockDim.x) {
            const int x0 = g * G - lead;
            if (x0 >= 0 && x0 + G <= a.ow) {
                uint32_t w = 0;
#pragma unroll
                for (int k = 0; k < G; ++k) w |= resize_one<F16, OP, T>(in, 1, oy, x0 + k, a, lut) << (k * 8 * (int)sizeof(T));
                *reinterpret_cast<uint32_t *>(orow + x0) = w;
            } else {
                for (int k = 0; k < G; ++k)
                    if (x0 + k >= 0 && x0 + k < a.ow) orow[x0 + k] = (T)resize_one<F16, OP, T>(in, 1, oy, x0 + k, a, lut);
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------
static int64_t esize(const shl_mi355x_resize_desc *d) { return d->dtype == SHL_MI355X_F16 ? 2 : 1; }

// NULL when the arguments describe a resize, else what is wrong with them
static const char *resize_invalid(const void *in_dev, const void *out_dev, const shl_mi355x_resize_desc *d)
{
    if (!d || !in_dev || !out_dev) return "NULL argument";
    if (d->dtype != SHL_MI355X_I8 && d->dtype != SHL_MI355X_F16) return "dtype is neither int8 nor binary16";
    if (d->layout != SHL_MI355X_NHWC && d->layout != SHL_MI355X_NCHW) return "layout is neither NHWC nor NCHW";
    if (d->mode == SHL_MI355X_RESIZE_BICUBIC) return "bicubic is not supported";
    if (d->mode != SHL_MI355X_RESIZE_NEAREST && d->mode != SHL_MI355X_RESIZE_BILINEAR) return "unknown mode";
    if (d->align_corners != 0 && d->align_corners != 1) return "align_corners is neither 0 nor 1";
    if (d->n < 0 || d->c < 0 || d->out_h < 0 || d->out_w < 0) return "negative size";
    if (d->in_h < 1 || d->in_w < 1) return "an input without pixels";
    if (d->align_corners && (d->out_h == 1 || d->out_w == 1)) return "align_corners with an output extent of 1 (the reference divides by zero)";
    // the scales index memory: they must be what a division of two extents can give
    if (!(d->height_scale >= 0.0f && d->height_scale <= (float)d->in_h) || !(d->width_scale >= 0.0f && d->width_scale <= (float)d->in_w))
        return "a scale that is negative, larger than the input or not a number";
    for (int i = 0; i < 4; ++i)
        if (d->reserved[i] != 0) return "reserved fields must be zero";
    int64_t in_bytes, out_bytes;
    if (__builtin_mul_overflow((int64_t)d->n * d->c, (int64_t)d->in_h * d->in_w, &in_bytes) ||
        __builtin_mul_overflow((int64_t)d->n * d->c, (int64_t)d->out_h * d->out_w, &out_bytes) || in_bytes > INT64_MAX / 2 ||
        out_bytes > INT64_MAX / 2)
        return "tensor too large";
    in_bytes *= esize(d), out_bytes *= esize(d);
    const uintptr_t i0 = (uintptr_t)in_dev, i1 = i0 + (uintptr_t)in_bytes, o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)out_bytes;
    if (i0 < i1 && o0 < o1 && i0 < o1 && o0 < i1) return "the output overlaps the input";
    return NULL;
}

// The one place that chooses the form (launch and name).  SHL_MI355X_RESIZE_FORM=generic forces the literal form (A/B
// runs, tests); read per call.
static int resize_form(const void *in_dev, const void *out_dev, const shl_mi355x_resize_desc *d)
{
    const char *force = getenv("SHL_MI355X_RESIZE_FORM");
    if (force && strcmp(force, "generic") == 0) return RESIZE_GENERIC;
    if (d->layout == SHL_MI355X_NHWC) {
        // the grid carries the output row and the image in y / z
        if (((int64_t)d->c * esize(d)) % 16 != 0 || (((uintptr_t)in_dev | (uintptr_t)out_dev) & 15) != 0) return RESIZE_GENERIC;
        return d->out_h <= 65535 && d->n <= 65535 ? RESIZE_VEC : RESIZE_GENERIC;
    }
    if (((uintptr_t)out_dev & 3) != 0) return RESIZE_GENERIC;
    return (int64_t)d->n * d->c <= 0x7FFFFFFFll ? RESIZE_ROW : RESIZE_GENERIC;
}

static const char *const g_form_name[] = {"resize_nhwc_vec", "resize_nchw_row", "resize_generic"};

// div_by_scale(x, so, RN(1 / so)) == x / so for every x a bilinear sum of dequantised values can be (common.h; the range
// conv_plan.hip:fma_division_ok admits: 2^-40 <= so <= 2^40, |x| <= 2^60, x finite)
static bool resize_fma_ok(float s, int32_t zp, float so)
{
    return fma_div_ok((128.0 + fabs((double)zp)) * fabs((double)s) * 4.0, so);  // four terms, weights in [0, 1]
}

template <bool F16, int OP>
static void resize_launch(int form, const ResizeArgs &a, dim3 grid, dim3 block, hipStream_t s)
{
    if (form == RESIZE_VEC) hipLaunchKernelGGL((resize_nhwc_vec_kernel<F16, OP>), grid, block, 0, s, a);
    else if (form == RESIZE_ROW) hipLaunchKernelGGL((resize_nchw_row_kernel<F16, OP>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((resize_generic_kernel<F16, OP>), grid, block, 0, s, a);
}

static int pow2_at_least(int64_t v, int cap)
{
    int p = 1;
    while (p < cap && p < v) p <<= 1;
    return p;
}

}  // namespace shl

extern "C" const char *shl_mi355x_resize_kernel_name(const struct shl_mi355x_resize_desc *d, const void *in_dev, const void *out_dev)
{
    if (shl::resize_invalid(in_dev, out_dev, d)) return "";
    return shl::g_form_name[shl::resize_form(in_dev, out_dev, d)];
}

extern "C" int shl_mi355x_resize(const void *in_dev, void *out_dev, const struct shl_mi355x_resize_desc *d, void *stream)
{
    using namespace shl;
    const char *why = resize_invalid(in_dev, out_dev, d);
    if (why) {
        set_error("resize: %s", why);
        return SHL_MI355X_EINVAL;
    }
    const int64_t total = (int64_t)d->n * d->c * d->out_h * d->out_w;
    if (total == 0) return SHL_MI355X_OK;
    const bool f16 = d->dtype == SHL_MI355X_F16;
    const int form = resize_form(in_dev, out_dev, d);
    ResizeArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in_dev, a.out = out_dev;
    a.n = d->n, a.c = d->c, a.ih = d->in_h, a.iw = d->in_w, a.oh = d->out_h, a.ow = d->out_w;
    a.hs = d->height_scale, a.ws = d->width_scale;
    a.align = d->align_corners;
    a.nchw = d->layout == SHL_MI355X_NCHW;
    a.si = d->in_scale, a.zi = (float)d->in_zp, a.so = d->out_scale, a.zo = (float)d->out_zp, a.inv_so = 1.0f / d->out_scale;
    a.fma_div = resize_fma_ok(d->in_scale, d->in_zp, d->out_scale) ? 1 : 0;
    int op = OP_BILINEAR;
    if (d->mode == SHL_MI355X_RESIZE_NEAREST) {
        // int8: equal records whose round trip is the identity on all 256 values make the gather a byte copy
        const bool raw = f16 || (d->in_zp == d->out_zp && memcmp(&d->in_scale, &d->out_scale, sizeof(float)) == 0 &&
                                 requant_is_identity(d->out_scale, d->out_zp));
        op = raw ? OP_COPY : OP_LUT;
        if (!raw) memcpy(a.tab, d->table, 256);
    }
    dim3 grid, block;
    if (form == RESIZE_VEC) {
        a.pieces = (int32_t)((int64_t)d->c * esize(d) / 16);
        const int bx = pow2_at_least(a.pieces, 256), by = 256 / bx;
        a.piece_blocks = (a.pieces + bx - 1) / bx;
        const int64_t gx = (int64_t)a.piece_blocks * ((d->out_w + by - 1) / by);
        if (gx > 0x7FFFFFFFll) {
            set_error("resize: %lld workgroups per row exceed the grid", (long long)gx);
            return SHL_MI355X_ENOTSUP;
        }
        block = dim3(bx, by), grid = dim3((unsigned)gx, d->out_h, d->n);
    } else if (form == RESIZE_ROW) {
        const int per = f16 ? 2 : 4;
        const int bx = pow2_at_least(((int64_t)d->out_w + 2 * per - 2) / per, 256), by = 256 / bx;
        // one workgroup per plane when there are planes enough to fill the device, else the rows are shared out
        const int64_t planes = (int64_t)d->n * d->c;
        int64_t chunks = planes >= 2048 ? 1 : (2048 + planes - 1) / planes;
        const int64_t most = ((int64_t)d->out_h + by - 1) / by;
        if (chunks > most) chunks = most;
        if (chunks > 65535) chunks = 65535;
        a.rows_per_wg = (int32_t)(((int64_t)d->out_h + chunks - 1) / chunks);
        block = dim3(bx, by), grid = dim3((unsigned)planes, (unsigned)(((int64_t)d->out_h + a.rows_per_wg - 1) / a.rows_per_wg));
    } else {
        const int64_t blocks = (total + 255) / 256;
        if (blocks > 0x7FFFFFFFll) {
            set_error("resize: %lld workgroups exceed the grid", (long long)blocks);
            return SHL_MI355X_ENOTSUP;
        }
        block = dim3(256), grid = dim3((unsigned)blocks);
    }
    hipStream_t s = (hipStream_t)stream;
    if (f16) {
        if (op == OP_BILINEAR) resize_launch<true, OP_BILINEAR>(form, a, grid, block, s);
        else resize_launch<true, OP_COPY>(form, a, grid, block, s);
    } else {
        if (op == OP_BILINEAR) resize_launch<false, OP_BILINEAR>(form, a, grid, block, s);
        else if (op == OP_LUT) resize_launch<false, OP_LUT>(form, a, grid, block, s);
        else resize_launch<false, OP_COPY>(form, a, grid, block, s);
    }
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

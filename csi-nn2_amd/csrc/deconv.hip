// deconv.hip -- transposed convolution (deconv2d, depthwise_deconv2d) for gfx950: the learned upsampling of a U-Net / FCN
// decoder, pix2pix, DCGAN, FSRCNN.  Restates shl_ref_deconv2d_quant / shl_ref_depthwise_deconv2d_quant
// (source/reference/deconvolution.c:21-175, 334-369 through shl_ref_conv_callback_base, utils.c:639-655): the reference
// SCATTERS every input element into out[n, iy sh - pt + ky, ix sw - pl + kx, oc]; both kernels here GATHER, so every output
// element is written once, by one thread, with the epilogue of DESIGN 2.
//
//   S = sum (q - zp_in) w  over the (iy, ix, ky, kx, ic) that reach the output element, exact int32
//   binary16: fp32 sum of exact products
// ConvArgs: H, W, C are the deconvolution's INPUT, Ho, Wo, Co its OUTPUT.  The output extents are whatever the output tensor
// says (output_padding is a larger output; an element no tap reaches gets the epilogue of S = 0); dilation is not read.
//
// Two forms, chosen and named by ONE function (deconv_form):
//   gather  one output element per thread (conv_direct.hip's shape and coalescing rule): tap ky contributes when
//           (oy + pt - ky) % sh == 0 and iy = (oy + pt - ky) / sh lies in [0, H); loops ky DESCENDING, kx descending, ic
//           ascending -- the order in which the reference's scatter reaches one output element, so the binary16 sum is the
//           reference's bit for bit.  int8 / binary16, NHWC / NCHW, group 1 / depthwise, any kernel, stride and padding.
//   phase   MFMA; NHWC, group 1, Cin * esize a multiple of 32.  With stride s the operator is sh sw small ordinary
//           convolutions: phase (py, px) owns the outputs with (oy + pt) % sh == py, (ox + pl) % sw == px, its taps are
//           ky = py + j sh < Kh, kx = px + i sw < Kw, and with qy = (oy + pt) / sh tap j reads iy = qy - j.  One wave computes
//           32 consecutive pixels of ONE phase (flattened over n, qy, qx) x 32 output channels; a workgroup is four waves on
//           four tiles.  No LDS, no barrier: the activation fragment comes straight from global memory (the pad page when the
//           position is outside the image), the weight fragment from the plan's copy in fragment order.
#include <stdlib.h>
#include <string.h>

#include "igemm_common.h"

namespace shl {

// ---- the decomposition of one axis (host and device) ----------------------------------------------------------------------
// taps of phase p: k = p, p + s, ... < K
__host__ __device__ inline int dc_taps(int K, int s, int p) { return p < K ? (K - p + s - 1) / s : 0; }
// taps of the phases in front of p
__host__ __device__ inline int dc_taps_before(int K, int s, int p)
{
    int n = 0;
    for (int q = 0; q < p; ++q) n += dc_taps(K, s, q);
    return n;
}
// first output position o >= 0 with (o + pad) % s == p
__host__ __device__ inline int dc_first(int pad, int s, int p)
{
    const int r = (p - pad) % s;
    return r < 0 ? r + s : r;
}
// output positions o0, o0 + s, ... < O
__host__ __device__ inline int dc_count(int O, int s, int o0) { return o0 < O ? (O - o0 + s - 1) / s : 0; }

// ---- gather form ----------------------------------------------------------------------------------------------------------
// weights: NHWC group 1 [O, Kh, Kw, I]; NCHW group 1 [I, O, Kh, Kw]; depthwise NHWC [1, Kh, Kw, C]; depthwise NCHW [C, 1, Kh, Kw]
template <bool kNHWC, bool kDW>
__device__ __forceinline__ int64_t deconv_weight_index(const ConvArgs &a, int oc, int ky, int kx, int ic)
{
    if (kDW) return kNHWC ? ((int64_t)ky * a.Kw + kx) * a.C + oc : ((int64_t)oc * a.Kh + ky) * a.Kw + kx;
    if (kNHWC) return (((int64_t)oc * a.Kh + ky) * a.Kw + kx) * a.C + ic;
    return (((int64_t)ic * a.Co + oc) * a.Kh + ky) * a.Kw + kx;
}

template <typename T, bool kNHWC, bool kDW>
__global__ __launch_bounds__(256) void deconv_gather_kernel(ConvArgs a)
{
    const int64_t total = (int64_t)a.M * a.Co;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        int n, oy, ox, oc;
        if (kNHWC) {
            oc = (int)(idx % a.Co);
            int64_t p = idx / a.Co;
            ox = (int)(p % a.Wo);
            p /= a.Wo;
            oy = (int)(p % a.Ho);
            n = (int)(p / a.Ho);
        } else {
            ox = (int)(idx % a.Wo);
            int64_t p = idx / a.Wo;
            oy = (int)(p % a.Ho);
            p /= a.Ho;
            oc = (int)(p % a.Co);
            n = (int)(p / a.Co);
        }
        const T *in = static_cast<const T *>(a.in);
        const T *w = static_cast<const T *>(a.w);
        const int ic0 = kDW ? oc : 0, ic1 = kDW ? oc + 1 : a.C;
        int32_t acc_i = 0;
        float acc_f = 0.0f;
        for (int ky = a.Kh - 1; ky >= 0; --ky) {
            const int ty = oy + a.pt - ky;
            if (ty < 0 || ty % a.sh != 0) continue;
            const int y = ty / a.sh;
            if (y >= a.H) continue;
            for (int kx = a.Kw - 1; kx >= 0; --kx) {
                const int tx = ox + a.pl - kx;
                if (tx < 0 || tx % a.sw != 0) continue;
                const int x = tx / a.sw;
                if (x >= a.W) continue;
                for (int ic = ic0; ic < ic1; ++ic) {
                    const int64_t ii = kNHWC ? (((int64_t)n * a.H + y) * a.W + x) * a.C + ic
                                             : (((int64_t)n * a.C + ic) * a.H + y) * a.W + x;
                    const int64_t wi = deconv_weight_index<kNHWC, kDW>(a, oc, ky, kx, ic);
                    if constexpr (sizeof(T) == 1) acc_i += ((int32_t)in[ii] - a.in_zp) * (int32_t)w[wi];
                    else acc_f = __fadd_rn(acc_f, __fmul_rn((float)in[ii], (float)w[wi]));
                }
            }
        }
        if constexpr (sizeof(T) == 1)
            static_cast<int8_t *>(a.out)[idx] = (int8_t)requant_i8_fast<true>(acc_i, a.mult[oc], a.bias[oc], a);
        else
            static_cast<uint16_t *>(a.out)[idx] = finish_f16(acc_f, a.bias[oc], a);
    }
}

// ---- phase form -----------------------------------------------------------------------------------------------------------
struct DeconvPhaseArgs {
    const void *w_frag;      // [phase][tap][K step][channel tile][64 lanes][16 B], zero padded to whole channel tiles
    const int32_t *acc_tab;  // int8: [phase][co_pad] = -zp_in * sum over the phase's taps and ic of w
    int32_t ctiles;          // channel tiles of 32
    int32_t ksteps;          // MFMA steps per tap = Cin * esize / 32
    int32_t co_pad;          // ctiles * 32
};

template <bool kI8, int EPI>
__global__ __launch_bounds__(256) void deconv_phase_kernel(ConvArgs a, DeconvPhaseArgs g)
{
    using Acc = typename AccT<kI8>::type;
    constexpr int ESIZE = kI8 ? 1 : 2;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int frow = lane & 31, fhalf = lane >> 5;
    const int phase = blockIdx.y;
    const int py = phase / a.sw, px = phase - py * a.sw;
    const int ty = dc_taps(a.Kh, a.sh, py), tx = dc_taps(a.Kw, a.sw, px);
    const int oy0 = dc_first(a.pt, a.sh, py), ox0 = dc_first(a.pl, a.sw, px);
    const int rows = dc_count(a.Ho, a.sh, oy0), cols = dc_count(a.Wo, a.sw, ox0);
    const int64_t P = (int64_t)a.N * rows * cols;  // the phase's pixels (at most M)
    const int64_t ptiles = (P + 31) >> 5;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;  // channel tile fastest: the four waves share their pixels' lines
    if (tile >= ptiles * g.ctiles) return;  // (an empty phase included; no barrier below)
    const int ct = (int)(tile % g.ctiles);
    const int64_t m_raw = (tile / g.ctiles) * 32 + frow;
    const bool live = m_raw < P;
    const int64_t m = live ? m_raw : P - 1;  // rows past the end of the list read a valid pixel; their stores are guarded
    const int rc = rows * cols;
    const int n = (int)(m / rc);
    const int rem = (int)(m - (int64_t)n * rc);
    const int r = rem / cols, c = rem - r * cols;
    const int qy = (oy0 + a.pt) / a.sh + r, qx = (ox0 + a.pl) / a.sw + c;

    const int pixb = a.C * ESIZE;
    const char *img = static_cast<const char *>(a.in) + (int64_t)n * a.H * a.W * pixb + fhalf * 16;
    const char *pad = static_cast<const char *>(a.pad_page) + (lane << 4);
    const int64_t tap0 = (int64_t)dc_taps_before(a.Kh, a.sh, py) * a.Kw + (int64_t)ty * dc_taps_before(a.Kw, a.sw, px);
    const int64_t wstep = (int64_t)g.ctiles * 1024;
    const char *wp = static_cast<const char *>(g.w_frag) + (tap0 * g.ksteps * g.ctiles + ct) * 1024 + lane * 16;

    Acc acc;
    if constexpr (kI8) {
        Acc t[1];
        igemm_acc_from_table(t, g.acc_tab + (int64_t)phase * g.co_pad + ct * 32, fhalf);
        acc = t[0];
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    }
    for (int j = 0; j < ty; ++j) {
        const int iy = qy - j;
        for (int i = 0; i < tx; ++i) {
            const int ix = qx - i;
            const bool ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const char *src = ok ? img + ((int64_t)iy * a.W + ix) * pixb : pad;
            const int step = ok ? 32 : 0;
            for (int ks = 0; ks < g.ksteps; ++ks) {
                const v4i fw = *reinterpret_cast<const v4i *>(wp);
                const v4i fx = *reinterpret_cast<const v4i *>(src);
                wp += wstep;
                src += step;
                acc = mfma<kI8>(fw, fx, acc);
            }
        }
    }

    // C/D layout: column (pixel) = lane & 31, register 4 g + e = channel 8 g + 4 (lane >> 5) + e of the tile
    if (!live) return;
    const int oy = oy0 + r * a.sh, ox = ox0 + c * a.sw;
    char *outp = static_cast<char *>(a.out) + (((int64_t)n * a.Ho + oy) * a.Wo + ox) * a.Co * ESIZE;
    const bool whole = (a.Co & 3) == 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c0 = ct * 32 + 8 * q + 4 * fhalf;
        if (c0 >= a.Co) continue;
        const float4 bi = *reinterpret_cast<const float4 *>(a.bias + c0);  // (the tables are padded to 128 channels)
        if constexpr (kI8) {
            const float4 mu = *reinterpret_cast<const float4 *>(a.mult + c0);
            const uint32_t pk = requant4_i8_sel<EPI>(acc[4 * q + 0], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3], mu, bi, a);
            if (whole) {
                *reinterpret_cast<uint32_t *>(outp + c0) = pk;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c0 + e < a.Co) outp[c0 + e] = (char)(pk >> (8 * e));
            }
        } else {
            const uint2 hp = finish4_f16(acc[4 * q + 0], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3], bi, a);
            if (whole) {
                *reinterpret_cast<uint2 *>(outp + c0 * 2) = hp;
            } else {
                const uint16_t h[4] = {(uint16_t)hp.x, (uint16_t)(hp.x >> 16), (uint16_t)hp.y, (uint16_t)(hp.y >> 16)};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c0 + e < a.Co) reinterpret_cast<uint16_t *>(outp)[c0 + e] = h[e];
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
static int dc_esize(const shl_mi355x_conv_desc &d) { return d.dtype == SHL_MI355X_I8 ? 1 : 2; }

// NULL when the descriptor is a deconvolution this library runs, else why not (*status: EINVAL / ENOTSUP)
const char *deconv_invalid(const shl_mi355x_conv_desc *dp, int *status)
{
    *status = SHL_MI355X_EINVAL;
    if (!dp) return "NULL descriptor";
    const shl_mi355x_conv_desc &d = *dp;
    if (d.layout != SHL_MI355X_NHWC && d.layout != SHL_MI355X_NCHW) return "unknown layout";
    if (d.dtype != SHL_MI355X_I8 && d.dtype != SHL_MI355X_F16) return "unknown dtype";
    if (d.act < SHL_MI355X_ACT_NONE || d.act > SHL_MI355X_ACT_RELU6) return "unknown activation";
    if (d.batch < 0 || d.in_h <= 0 || d.in_w <= 0 || d.in_c <= 0 || d.out_h <= 0 || d.out_w <= 0 || d.out_c <= 0)
        return "non-positive extent";
    if (d.kernel_h <= 0 || d.kernel_w <= 0 || d.stride_h <= 0 || d.stride_w <= 0) return "non-positive kernel size or stride";
    if (d.pad_top < 0 || d.pad_left < 0) return "negative padding";
    if (d.dtype == SHL_MI355X_I8 && !(d.out_scale > 0.0f)) return "the output scale must be positive";
    // no padding can make the scatter reach further than (in - 1) s + K; one more stride is room for output_padding
    if ((int64_t)d.out_h > ((int64_t)d.in_h - 1) * d.stride_h + d.kernel_h + d.stride_h ||
        (int64_t)d.out_w > ((int64_t)d.in_w - 1) * d.stride_w + d.kernel_w + d.stride_w)
        return "the output is larger than (in - 1) * stride + kernel + stride";
    if ((int64_t)d.batch * d.out_h * d.out_w > 0x7FFFFFFFll) return "N*Ho*Wo exceeds 2^31-1";
    *status = SHL_MI355X_ENOTSUP;
    if (d.dilation_h != 1 || d.dilation_w != 1) return "dilated deconvolution is not supported (the reference never reads dilation)";
    if (d.group != 1 && d.group != d.in_c) return "group must be 1 or in_c (group_deconv2d is not supported)";
    if (d.group != 1 && d.out_c != d.in_c) return "depthwise deconvolution needs out_c == in_c";
    return nullptr;
}

static bool deconv_phase_eligible(const shl_mi355x_conv_desc &d)
{
    return d.layout == SHL_MI355X_NHWC && d.group == 1 && ((int64_t)d.in_c * dc_esize(d)) % 32 == 0 &&
           (int64_t)d.stride_h * d.stride_w <= 65535;
}

// The one place that chooses the form (plan, launch, name, geometry).  epilogue_ok: the plan's tables admit the MFMA kernels'
// epilogue (conv_plan.hip; true when asked without tables).  SHL_MI355X_DECONV_FORM=gather|phase forces a form (read per
// call); a forced `phase` on a layer that is not eligible is refused: -1 and *why.
// The rule: eligible -> phase.  NOT MEASURED (profiles/deconv_notes.md).
int deconv_form(const shl_mi355x_conv_desc &d, bool epilogue_ok, const char **why)
{
    const bool eligible = deconv_phase_eligible(d) && epilogue_ok;
    const char *force = getenv("SHL_MI355X_DECONV_FORM");
    if (force && !strcmp(force, "gather")) return DECONV_GATHER;
    if (force && !strcmp(force, "phase")) {
        if (!eligible) {
            if (why) *why = "SHL_MI355X_DECONV_FORM=phase: the phase form needs NHWC, group 1, Cin * element size a multiple of 32 and "
                            "an output scale in 2^-40 .. 2^40";
            return -1;
        }
        return DECONV_PHASE;
    }
    return eligible ? DECONV_PHASE : DECONV_GATHER;
}

const char *deconv_form_name(int form, int dtype)
{
    const bool i8 = dtype == SHL_MI355X_I8;
    if (form == DECONV_PHASE) return i8 ? "deconv_phase_i8_mfma32x32x32" : "deconv_phase_f16_mfma32x32x16";
    return i8 ? "deconv_gather_i8" : "deconv_gather_f16";
}

static int dc_ctiles(const shl_mi355x_conv_desc &d) { return (d.out_c + 31) / 32; }
static int dc_ksteps(const shl_mi355x_conv_desc &d) { return d.in_c * dc_esize(d) / 32; }
int deconv_phases(const shl_mi355x_conv_desc &d) { return d.stride_h * d.stride_w; }

size_t deconv_phase_weight_bytes(const shl_mi355x_conv_desc &d)
{
    return (size_t)d.kernel_h * d.kernel_w * dc_ksteps(d) * dc_ctiles(d) * 1024;  // every tap belongs to exactly one phase
}

size_t deconv_phase_acc_bytes(const shl_mi355x_conv_desc &d) { return (size_t)deconv_phases(d) * dc_ctiles(d) * 32 * 4; }

// src: [O, Kh, Kw, I] (NHWC group 1).  dst: fragment order; acc: [phase][co_pad], int8 only (else untouched)
void deconv_pack_phase(const shl_mi355x_conv_desc &d, const char *src, char *dst, int32_t *acc)
{
    const int es = dc_esize(d), ctiles = dc_ctiles(d), ksteps = dc_ksteps(d), co_pad = ctiles * 32;
    const size_t pixb = (size_t)d.in_c * es;
    memset(dst, 0, deconv_phase_weight_bytes(d));
    for (int py = 0; py < d.stride_h; ++py)
        for (int px = 0; px < d.stride_w; ++px) {
            const int phase = py * d.stride_w + px;
            const int ty = dc_taps(d.kernel_h, d.stride_h, py), tx = dc_taps(d.kernel_w, d.stride_w, px);
            if (d.dtype == SHL_MI355X_I8)
                for (int oc = 0; oc < co_pad; ++oc) {
                    int64_t s = 0;
                    if (oc < d.out_c)
                        for (int j = 0; j < ty; ++j)
                            for (int i = 0; i < tx; ++i) {
                                const int8_t *row = reinterpret_cast<const int8_t *>(src) +
                                                    (((size_t)oc * d.kernel_h + py + j * d.stride_h) * d.kernel_w + px + i * d.stride_w) * pixb;
                                for (int ic = 0; ic < d.in_c; ++ic) s += row[ic];
                            }
                    acc[(size_t)phase * co_pad + oc] = (int32_t)(-(int64_t)d.in_zp * s);
                }
            for (int j = 0; j < ty; ++j)
                for (int i = 0; i < tx; ++i) {
                    const int ky = py + j * d.stride_h, kx = px + i * d.stride_w;
                    for (int ks = 0; ks < ksteps; ++ks)
                        for (int ct = 0; ct < ctiles; ++ct)
                            for (int lane = 0; lane < 64; ++lane, dst += 16) {
                                const int oc = ct * 32 + (lane & 31);
                                if (oc >= d.out_c) continue;
                                memcpy(dst, src + (((size_t)oc * d.kernel_h + ky) * d.kernel_w + kx) * pixb + ks * 32 + (lane >> 5) * 16, 16);
                            }
                }
        }
}

// tiles of 32 pixels x 32 channels over all phases, the largest phase's, for `batch` images
static void deconv_tiles(const shl_mi355x_conv_desc &d, int64_t batch, int64_t *total, int64_t *most)
{
    *total = *most = 0;
    for (int py = 0; py < d.stride_h; ++py)
        for (int px = 0; px < d.stride_w; ++px) {
            const int rows = dc_count(d.out_h, d.stride_h, dc_first(d.pad_top, d.stride_h, py));
            const int cols = dc_count(d.out_w, d.stride_w, dc_first(d.pad_left, d.stride_w, px));
            const int64_t t = ((batch * rows * cols + 31) / 32) * dc_ctiles(d);
            *total += t;
            if (t > *most) *most = t;
        }
}

int launch_deconv_gather(const ConvArgs &a, int dtype, int layout, hipStream_t s)
{
    const int64_t total = (int64_t)a.M * a.Co;
    if (total == 0) return SHL_MI355X_OK;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;  // grid-stride beyond 32 blocks per CU
    const dim3 grid((unsigned)blocks), block(256);
    const bool nhwc = layout == SHL_MI355X_NHWC, dw = a.group != 1;
#define SHL_DC(T)                                                                                      \
    do {                                                                                               \
        if (nhwc && dw) hipLaunchKernelGGL((deconv_gather_kernel<T, true, true>), grid, block, 0, s, a);   \
        else if (nhwc) hipLaunchKernelGGL((deconv_gather_kernel<T, true, false>), grid, block, 0, s, a);   \
        else if (dw) hipLaunchKernelGGL((deconv_gather_kernel<T, false, true>), grid, block, 0, s, a);     \
        else hipLaunchKernelGGL((deconv_gather_kernel<T, false, false>), grid, block, 0, s, a);            \
    } while (0)
    if (dtype == SHL_MI355X_I8) SHL_DC(int8_t);
    else SHL_DC(_Float16);
#undef SHL_DC
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

// a.w_frag: the fragment-ordered weights, a.acc_init: the [phase][co_pad] table
int launch_deconv_phase(const ConvArgs &a, const shl_mi355x_conv_desc &d, hipStream_t s)
{
    if (a.M == 0) return SHL_MI355X_OK;
    if (!deconv_phase_eligible(d) || !a.w_frag) {
        set_error("deconv_phase: the layer does not qualify");
        return SHL_MI355X_ENOTSUP;
    }
    DeconvPhaseArgs g;
    g.w_frag = a.w_frag, g.acc_tab = a.acc_init;
    g.ctiles = dc_ctiles(d), g.ksteps = dc_ksteps(d), g.co_pad = g.ctiles * 32;
    int64_t total, most;
    deconv_tiles(d, a.N, &total, &most);
    const int64_t gx = (most + 3) / 4;
    if (gx > 0x7FFFFFFFll) {
        set_error("deconv_phase: %lld workgroups per phase exceed the grid", (long long)gx);
        return SHL_MI355X_ENOTSUP;
    }
    const dim3 grid((unsigned)gx, (unsigned)deconv_phases(d)), block(256);
    if (d.dtype == SHL_MI355X_F16) {
        hipLaunchKernelGGL((deconv_phase_kernel<false, 0>), grid, block, 0, s, a, g);
    } else {
        // the flavours the other MFMA kernels instantiate: the clamp epilogues at compile time, the literal activation at run time
        const int epi = (a.act != SHL_MI355X_ACT_NONE && !a.act_clamp) ? -1 : (a.div_exact ? 3 : 0);
        if (epi == 3) hipLaunchKernelGGL((deconv_phase_kernel<true, 3>), grid, block, 0, s, a, g);
        else if (epi == 0) hipLaunchKernelGGL((deconv_phase_kernel<true, 0>), grid, block, 0, s, a, g);
        else hipLaunchKernelGGL((deconv_phase_kernel<true, -1>), grid, block, 0, s, a, g);
    }
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

}  // namespace shl

extern "C" const char *shl_mi355x_deconv_kernel_name(const struct shl_mi355x_conv_desc *d)
{
    int st;
    if (shl::deconv_invalid(d, &st)) return "";
    const int form = shl::deconv_form(*d, true, nullptr);
    return form < 0 ? "" : shl::deconv_form_name(form, d->dtype);
}

extern "C" int shl_mi355x_deconv_geometry(const struct shl_mi355x_conv_desc *d, int32_t *out, int32_t count)
{
    using namespace shl;
    int st;
    const char *why = deconv_invalid(d, &st);
    if (why) {
        set_error("deconv_geometry: %s", why);
        return st;
    }
    const int form = deconv_form(*d, true, &why);
    if (form < 0) {
        set_error("deconv_geometry: %s", why);
        return SHL_MI355X_ENOTSUP;
    }
    const int64_t phases = (int64_t)d->stride_h * d->stride_w;
    if (!out || count < 4 + 6 * phases) {
        set_error("deconv_geometry: room for 4 + 6 * %lld values is needed", (long long)phases);
        return SHL_MI355X_EINVAL;
    }
    int32_t *o = out;
    *o++ = form;
    *o++ = (int32_t)phases;
    for (int py = 0; py < d->stride_h; ++py)
        for (int px = 0; px < d->stride_w; ++px) {
            *o++ = py;
            *o++ = px;
            *o++ = dc_taps(d->kernel_h, d->stride_h, py);
            *o++ = dc_taps(d->kernel_w, d->stride_w, px);
            *o++ = dc_count(d->out_h, d->stride_h, dc_first(d->pad_top, d->stride_h, py));
            *o++ = dc_count(d->out_w, d->stride_w, dc_first(d->pad_left, d->stride_w, px));
        }
    int64_t total, most;
    deconv_tiles(*d, d->batch, &total, &most);
    *o++ = (int32_t)(total > 0x7FFFFFFFll ? 0x7FFFFFFF : total);
    const int64_t wgs = ((most + 3) / 4) * phases;
    *o++ = (int32_t)(wgs > 0x7FFFFFFFll ? 0x7FFFFFFF : wgs);
    return SHL_MI355X_OK;
}

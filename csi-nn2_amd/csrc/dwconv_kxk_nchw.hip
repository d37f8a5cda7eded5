// dwconv_kxk_nchw.hip -- depthwise NCHW convolution with a kernel that is not 3x3 (1..7 taps per axis, strides 1 / 2), int8 and
// binary16, for gfx950: the second form of an ALGO_DIRECT plan for these layers (the 5x5 layers of MobileNetV3 / EfficientNet /
// MnasNet, ConvNeXt's 7x7).  Scope, geometry, LDS budget, packing and the default rule: dw_nchw_kxk.h.
//
// An NCHW depthwise layer is N C independent single-plane convolutions.  A 256-thread workgroup owns a rectangle of rw output
// rows by 4 cg output columns of one plane -- or, where that rectangle is the whole plane (7x7, 14x14 maps), the whole planes of
// pl consecutive (n, c) pairs, so that its waves are full.  grid = (plane groups, rectangles per plane), sized from the call's
// batch.
//
// Staging.  The input patch ((rw - 1) sh + Kh) x ((4 cg - 1) sw + Kw) of every owned plane goes to LDS once, one LDS dword per
// item; positions outside the image hold the zp_in byte (int8) or 0 (binary16).  Plane bases are (n C + c) H W elements -- odd
// byte offsets with a 7x7 map -- so an item whose four bytes lie inside the image is fetched as the two ALIGNED dwords that
// enclose it and cut out with v_alignbyte_b32 (binary16: one dword where the pair is aligned); items that cross an image edge,
// and the last bytes of the tensor, where the second aligned dword would end beyond it, are fetched element by element.  (The
// element-only staging was not measured against this one: kept as the form that issues a quarter of the loads.)
// Row pitch: an ODD number of dwords (dw_nchw_kxk.h:dn_patch says why) -- reasoning, not a counter.
//
// int8.  A thread produces four consecutive outputs of a row.  Per filter row it reads the 2..4 aligned dwords under its span,
// forms each output's unaligned 4-byte windows with v_alignbyte_b32 (stride 2 steps the window by two bytes) and accumulates
// v_dot4_i32_i8 against the filter row the plan packed as two dwords (taps 0..3; taps 4..6 and a zero): a 7-tap row is two dot4s
// in place of seven dependent multiply-adds.  Padding bytes equal zp_in, so sum(q w) - zp_in sum(w) over ALL taps is the
// reference's sum of (q - zp_in) w over the in-image taps; the constant is the plan's acc_init[c].  requant_i8_fast as
// dwconv3x3_nchw_kernel.  Bytes of a window beyond Kw (never staged, or a neighbour's) meet zero weights.
//
// binary16.  conv_direct.hip's contract: fp32 accumulation in ky -> kx order over in-image taps only, __fmul_rn then __fadd_rn;
// a tap outside the image is skipped by a select, not multiplied by zero (0 * inf, -0).  A thread keeps the 3 sw + 7 values of a
// patch row under its four outputs in registers, so each LDS value is read once per thread and filter row; the filters of the
// owned planes sit in LDS behind the patches, widened to fp32 (exact) as [7][8], a row two 16-byte broadcast reads.  The
// validity of a value is a lane mask held in scalar registers (one per value of the row, and-ed with the row's), so a tap costs
// a multiply, an add and a v_cndmask.  finish_f16 is the epilogue.  Results equal the direct kernel's bit for bit.
//
// Stores: one packed store per thread (int8: a dword, binary16: two dwords) where the address is aligned and all its outputs
// exist, element stores otherwise; nothing outside [out, out + N C Ho Wo).
//
// No matrix instructions, by design: weights differ per plane, so a plane's convolution as a GEMM is a banded Toeplitz operand
// with Kw useful values per 32 of K; and for binary16 the MFMA's internal summation order cannot reproduce the reference's chain.
#include "common.h"
#include "dw_nchw_kxk.h"

namespace shl {

// output at byte B of the thread's span: one or two dot4s on its unaligned windows
template <int B, bool KW2, int ND>
__device__ __forceinline__ int dn_dot(const uint32_t (&d)[ND], const uint2 &w, int acc)
{
    constexpr int q = B >> 2, sft = B & 3;
    uint32_t w0, w1 = 0;
    if constexpr (sft == 0) {
        w0 = d[q];
        if constexpr (KW2) w1 = d[q + 1];
    } else {
        w0 = __builtin_amdgcn_alignbyte(d[q + 1], d[q], (uint32_t)sft);
        if constexpr (KW2) w1 = __builtin_amdgcn_alignbyte(d[q + 2], d[q + 1], (uint32_t)sft);
    }
    acc = __builtin_amdgcn_sdot4((int)w0, (int)w.x, acc, false);
    if constexpr (KW2) acc = __builtin_amdgcn_sdot4((int)w1, (int)w.y, acc, false);
    return acc;
}

// what both kernels derive from the block and the thread
struct DnWhere {
    int64_t plane0, planes;  // first owned plane, planes of the call
    int oy0, ox0;            // first output of the rectangle
    int yb, xb;              // image position of patch element (0, 0)
};

__device__ __forceinline__ DnWhere dn_where(const ConvArgs &a, const DnGeom &g)
{
    DnWhere p;
    const int ty = (int)blockIdx.y / g.tiles_x, tx = (int)blockIdx.y - ty * g.tiles_x;
    p.plane0 = (int64_t)blockIdx.x * g.pl;
    p.planes = (int64_t)a.N * a.C;
    p.oy0 = ty * g.rw, p.ox0 = tx * g.cg * DN_TX;
    p.yb = p.oy0 * a.sh - a.pt, p.xb = p.ox0 * a.sw - a.pl;
    return p;
}

template <int SW, bool KW2>
__global__ __launch_bounds__(256) void dwconv_kxk_nchw_i8_kernel(ConvArgs a, DnGeom g)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t dn_lds[];
    const DnWhere p = dn_where(a, g);
    const int tid = threadIdx.x, hw = a.H * a.W;
    {
        const uint8_t *in8 = static_cast<const uint8_t *>(a.in);
        const int64_t total = p.planes * hw;
        const bool wide = ((uintptr_t)a.in & 3) == 0;
        const uint32_t zp4 = (uint32_t)(a.in_zp & 0xff) * 0x01010101u;
        const int per_plane = g.ph * g.row_dw, items = g.pl * per_plane;
        for (int i = tid; i < items; i += DN_THREADS) {
            const int pi = i / per_plane, j = i - pi * per_plane, r = j / g.row_dw, q = j - r * g.row_dw;
            if (p.plane0 + pi >= p.planes) continue;
            const int y = p.yb + r, x = p.xb + 4 * q;
            uint32_t v = zp4;
            if ((unsigned)y < (unsigned)a.H && x > -4 && x < a.W) {
                const int64_t go = (p.plane0 + pi) * hw + (int64_t)y * a.W + x, ga = go & ~(int64_t)3;
                if (x >= 0 && x + 3 < a.W && wide && ga + 8 <= total) {
                    const uint32_t lo = *reinterpret_cast<const uint32_t *>(in8 + ga), hi = *reinterpret_cast<const uint32_t *>(in8 + ga + 4);
                    v = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)go & 3u);
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if ((unsigned)(x + b) < (unsigned)a.W) v = (v & ~(0xffu << (8 * b))) | ((uint32_t)in8[go + b] << (8 * b));
                }
            }
            dn_lds[pi * g.plane_dw + r * g.pitch_dw + q] = v;
        }
    }
    __syncthreads();
    const int per = g.cg * g.rw, pi = tid / per, rest = tid - pi * per, rr = rest / g.cg, t = rest - rr * g.cg;
    const int64_t plane = p.plane0 + pi;
    const int oy = p.oy0 + rr, ox = p.ox0 + t * DN_TX;
    if (pi >= g.pl || plane >= p.planes || oy >= a.Ho || ox >= a.Wo) return;
    const int c = (int)(plane % a.C);
    constexpr int ND = (3 * SW + (KW2 ? 8 : 4) + 3) / 4;
    const uint32_t *row = dn_lds + pi * g.plane_dw + rr * a.sh * g.pitch_dw + t * SW;
    const uint2 *wr = static_cast<const uint2 *>(a.w) + (int64_t)c * a.Kh;
    const int init = a.acc_init[c];
    int acc[DN_TX] = {init, init, init, init};
    for (int ky = 0; ky < a.Kh; ++ky, row += g.pitch_dw) {
        const uint2 w = wr[ky];
        uint32_t d[ND];
#pragma unroll
        for (int q = 0; q < ND; ++q) d[q] = row[q];
        acc[0] = dn_dot<0, KW2, ND>(d, w, acc[0]);
        acc[1] = dn_dot<SW, KW2, ND>(d, w, acc[1]);
        acc[2] = dn_dot<2 * SW, KW2, ND>(d, w, acc[2]);
        acc[3] = dn_dot<3 * SW, KW2, ND>(d, w, acc[3]);
    }
    const float m = a.mult[c], b = a.bias[c];
    int qv[DN_TX];
#pragma unroll
    for (int j = 0; j < DN_TX; ++j) qv[j] = requant_i8_fast(acc[j], m, b, a);
    int8_t *out = static_cast<int8_t *>(a.out) + plane * a.Ho * a.Wo + (int64_t)oy * a.Wo + ox;
    if (ox + DN_TX <= a.Wo && ((uintptr_t)out & 3) == 0) {
        *reinterpret_cast<uint32_t *>(out) = pack4_i8(qv[0], qv[1], qv[2], qv[3]);
    } else {
#pragma unroll
        for (int j = 0; j < DN_TX; ++j)
            if (ox + j < a.Wo) out[j] = (int8_t)qv[j];
    }
}

template <int SW>
__global__ __launch_bounds__(256) void dwconv_kxk_nchw_f16_kernel(ConvArgs a, DnGeom g)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t dn_lds[];
    const DnWhere p = dn_where(a, g);
    const int tid = threadIdx.x, hw = a.H * a.W, taps = a.Kh * a.Kw;
    float *wl = reinterpret_cast<float *>(dn_lds + g.w_dw);  // [owned plane][ky][8]: fp32 (the widening is exact), a row is two 16-byte reads
    {
        const uint16_t *in16 = static_cast<const uint16_t *>(a.in);
        const bool wide = ((uintptr_t)a.in & 3) == 0;
        const int per_plane = g.ph * g.row_dw, items = g.pl * per_plane;
        for (int i = tid; i < items; i += DN_THREADS) {
            const int pi = i / per_plane, j = i - pi * per_plane, r = j / g.row_dw, q = j - r * g.row_dw;
            if (p.plane0 + pi >= p.planes) continue;
            const int y = p.yb + r, x = p.xb + 2 * q;
            uint32_t v = 0;
            if ((unsigned)y < (unsigned)a.H && x > -2 && x < a.W) {
                const int64_t go = (p.plane0 + pi) * hw + (int64_t)y * a.W + x;  // elements
                if (x >= 0 && x + 1 < a.W && wide && !(go & 1)) {
                    v = *reinterpret_cast<const uint32_t *>(in16 + go);
                } else {
                    if (x >= 0) v = in16[go];
                    if (x + 1 < a.W) v |= (uint32_t)in16[go + 1] << 16;
                }
            }
            dn_lds[pi * g.plane_dw + r * g.pitch_dw + q] = v;
        }
        const uint16_t *w16 = static_cast<const uint16_t *>(a.w);  // O1HW
        for (int i = tid; i < g.pl * taps; i += DN_THREADS) {
            const int pi = i / taps, k = i - pi * taps;
            if (p.plane0 + pi < p.planes) wl[pi * DN_W_SLOT + k / a.Kw * 8 + k % a.Kw] = f16_bits_to_float(w16[(int64_t)((p.plane0 + pi) % a.C) * taps + k]);
        }
    }
    __syncthreads();
    const int per = g.cg * g.rw, pi = tid / per, rest = tid - pi * per, rr = rest / g.cg, t = rest - rr * g.cg;
    const int64_t plane = p.plane0 + pi;
    const int oy = p.oy0 + rr, ox = p.ox0 + t * DN_TX;
    if (pi >= g.pl || plane >= p.planes || oy >= a.Ho || ox >= a.Wo) return;
    const int c = (int)(plane % a.C);
    constexpr int NV = 3 * SW + DN_MAX_K, ND = (NV + 1) / 2;  // values / dwords of a patch row under the thread's four outputs
    const uint32_t *row = dn_lds + pi * g.plane_dw + rr * a.sh * g.pitch_dw + t * 2 * SW;
    const float *wf = wl + pi * DN_W_SLOT;
    const int y0 = oy * a.sh - a.pt, x0 = ox * SW - a.pl;
    bool xok[NV];  // value v of the row lies inside the image: lane masks in scalar registers, one s_and per value and filter row
#pragma unroll
    for (int v = 0; v < NV; ++v) xok[v] = (unsigned)(x0 + v) < (unsigned)a.W;
    float acc[DN_TX] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ky = 0; ky < a.Kh; ++ky, row += g.pitch_dw, wf += 8) {
        const bool yok = (unsigned)(y0 + ky) < (unsigned)a.H;
        const float4 wa = *reinterpret_cast<const float4 *>(wf), wb = *reinterpret_cast<const float4 *>(wf + 4);
        const float wrow[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
        float xv[2 * ND];
#pragma unroll
        for (int q = 0; q < ND; ++q) {
            const uint32_t d = row[q];
            xv[2 * q] = f16_bits_to_float((uint16_t)(d & 0xffffu));
            xv[2 * q + 1] = f16_bits_to_float((uint16_t)(d >> 16));
        }
#pragma unroll
        for (int kx = 0; kx < DN_MAX_K; ++kx) {
            if (kx < a.Kw) {
                const float wv = wrow[kx];
#pragma unroll
                for (int j = 0; j < DN_TX; ++j) {
                    const float s = __fadd_rn(acc[j], __fmul_rn(xv[j * SW + kx], wv));
                    acc[j] = yok && xok[j * SW + kx] ? s : acc[j];
                }
            }
        }
    }
    const float b = a.bias[c];
    uint32_t h[DN_TX];
#pragma unroll
    for (int j = 0; j < DN_TX; ++j) h[j] = finish_f16(acc[j], b, a);
    uint16_t *out = static_cast<uint16_t *>(a.out) + plane * a.Ho * a.Wo + (int64_t)oy * a.Wo + ox;
    if (ox + DN_TX <= a.Wo && ((uintptr_t)out & 3) == 0) {
        reinterpret_cast<uint32_t *>(out)[0] = h[0] | (h[1] << 16);
        reinterpret_cast<uint32_t *>(out)[1] = h[2] | (h[3] << 16);
    } else {
#pragma unroll
        for (int j = 0; j < DN_TX; ++j)
            if (ox + j < a.Wo) out[j] = (uint16_t)h[j];
    }
}

// symmetric weights and the fast epilogue (int8) are the caller's business (conv_plan.hip:dw_nchw_kxk_takes); this is the scope,
// the geometry and, with by_rule, the measured default rule (dw_nchw_kxk.h).  N: the plan's batch.
bool dwconv_kxk_nchw_pick(bool i8, int N, int C, int Co, int group, int H, int W, int Ho, int Wo, int Kh, int Kw, int sh, int sw, int dh, int dw,
                          int in_zp, bool by_rule)
{
    DnGeom g;
    N = N > 0 ? N : 1;
    if (!dn_scope(i8, C, Co, group, Kh, Kw, sh, sw, dh, dw, in_zp) || !dn_geometry(i8, N, C, H, W, Ho, Wo, Kh, Kw, sh, sw, g)) return false;
    return !by_rule || dn_default(i8, (int64_t)N * C, Ho, Wo, Kh, Kw, sh, sw);
}

size_t dwconv_kxk_nchw_weight_bytes(int C, int Kh) { return (size_t)dn_weight_bytes(C, Kh); }

void dwconv_kxk_nchw_pack(const int8_t *o1hw, int C, int Kh, int Kw, int in_zp, uint32_t *dst, int32_t *acc_init)
{
    dn_pack(o1hw, C, Kh, Kw, in_zp, dst, acc_init);
}

// a.w: int8 the packed filter rows, binary16 the O1HW weights as they came
int launch_dwconv_kxk_nchw(const ConvArgs &a, int dtype, hipStream_t s)
{
    const bool i8 = dtype == SHL_MI355X_I8;
    DnGeom g;
    if (!dn_scope(i8, a.C, a.Co, a.group, a.Kh, a.Kw, a.sh, a.sw, a.dh, a.dw, a.in_zp) ||
        !dn_geometry(i8, a.N, a.C, a.H, a.W, a.Ho, a.Wo, a.Kh, a.Kw, a.sh, a.sw, g)) {
        set_error("dwconv_kxk_nchw: kernel size, stride, plane sizes, LDS patch or grid out of range");
        return SHL_MI355X_ENOTSUP;
    }
    if (!i8 && (((uintptr_t)a.in | (uintptr_t)a.out) & 1)) {
        set_error("dwconv_kxk_nchw: binary16 tensors must be 2-byte aligned");
        return SHL_MI355X_EINVAL;
    }
    const dim3 grid((unsigned)g.groups, (unsigned)(g.tiles_x * g.tiles_y));
    const size_t lds = (size_t)g.lds_bytes;
    if (i8) {
        const bool kw2 = a.Kw > 4;
        if (a.sw == 1 && kw2) hipLaunchKernelGGL((dwconv_kxk_nchw_i8_kernel<1, true>), grid, dim3(DN_THREADS), lds, s, a, g);
        else if (a.sw == 1) hipLaunchKernelGGL((dwconv_kxk_nchw_i8_kernel<1, false>), grid, dim3(DN_THREADS), lds, s, a, g);
        else if (kw2) hipLaunchKernelGGL((dwconv_kxk_nchw_i8_kernel<2, true>), grid, dim3(DN_THREADS), lds, s, a, g);
        else hipLaunchKernelGGL((dwconv_kxk_nchw_i8_kernel<2, false>), grid, dim3(DN_THREADS), lds, s, a, g);
    } else {
        if (a.sw == 1) hipLaunchKernelGGL((dwconv_kxk_nchw_f16_kernel<1>), grid, dim3(DN_THREADS), lds, s, a, g);
        else hipLaunchKernelGGL((dwconv_kxk_nchw_f16_kernel<2>), grid, dim3(DN_THREADS), lds, s, a, g);
    }
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

}  // namespace shl

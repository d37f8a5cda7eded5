// conv_group_mfma.hip -- grouped (not depthwise) int8 convolution on the matrix cores, over an LDS patch, on the NHWC view.
//
// conv_group_direct_kernel (conv_direct.hip) runs every grouped layer one output per thread: a scalar loop over the taps and the
// group's channels and several 64-bit divisions per output.  The dense implicit-GEMM kernels cannot take such a layer by
// zero-filling its weights to [Cout][Kh Kw C] -- that is G times the K loop and the weight bytes.  Here the zero fill stops at
// the 32 channels an MFMA consumes anyway, and the kernel itself knows nothing about groups:
//
//   unit       (plan time, group_mfma.h) 1, 2 or 4 blocks of 32 output channels that read ONE window of kc input channels.
//              C/G = 4 / 8 / 16: 32 output channels over the 32 input channels of their 8 / 4 / 2 groups, the 32 x 32 weight
//              matrix of a tap block-diagonal (dwconv_kxk.hip's diagonal fragment with blocks for bytes; the zeros are exact
//              in int32).  C/G a multiple of 32: up to four of a group's output blocks over the group's own channels, dense.
//   weights    packed once as A fragments [unit][block][K slab of 32 channels][tap][lane][16 B]: a wave fetches a tap's
//              fragment with one coalesced 1 KiB load, one tap ahead of its use.  They never touch LDS.
//   workgroup  four waves: one unit x one rectangle of output pixels (btx x bty tiles of 8 x 4) of one image.  Per K slab the
//              rectangle's input patch with its halo is staged once, [patch pixel][32 B + 16], pixels outside the image as the
//              input zero point (folded into acc_init by the plan): every one of the Kh Kw taps is a constant LDS offset, a
//              stride of 2 reads the patch at pixel stride 2.  The NEXT slab's patch is requested into registers before this
//              slab's MFMAs and stored behind them, between two barriers.
//   wave       one block x up to FOUR pixel tiles (4 / nblk waves deal a block's tiles out), one v16i accumulator per tile
//              live across the slab and tap loops; per tap and tile one ds_read_b128 (lane & 31 = pixel, lane >> 5 = half) and
//              one v_mfma_i32_32x32x32_i8
//   store      requant4_i8_t<EPI>, tile_channels_16 (v_permlane32_swap), one uint4 per lane, masked at the map's edge
//
// The layer arrives NCHW (the reference computes no channel-interleaved grouped convolution in NHWC); conv_plan.hip runs the
// re-layout pass of the implicit-GEMM families in front and behind.
// Cost, by dwconv_mfma.hip's cycle count (32 cycles per MFMA on one of four matrix pipes) and NOT by measurement: a 3x3 tap loop
// of four tiles is 36 MFMAs per 128 pixels x 32 channels against 9 KiB of weight fragments from L2 / L1; with one tile per
// wave the fragment loads (1 KiB per MFMA and wave) are the bound.  Measured: profiles/group_mfma_notes.md.
// LDS: at most 40 KiB (group_mfma.h) -- four workgroups per CU beside 128 registers; the pitch argument is in group_mfma.h.
// Registers (tools/dev/kregs.py): see profiles/group_mfma_notes.md; build.py's NO_SPILL_SOURCES holds the kernel free of spills.
// Restates shl_ref_group_conv2d_quant (source/reference/convolution.c:271-354, 476-508) + relu variants for NCHW.
#include <stdlib.h>

#include <type_traits>

#include "dw_mfma.h"
#include "group_mfma.h"

namespace shl {

// kMulti: more than one K slab -- the next slab's patch waits in GM_PREFETCH registers per thread under the MFMAs; a single
// slab (every narrow group) stages through GM_STAGE registers that are dead before the first MFMA, and affords a larger patch
template <int EPI, bool kMulti>
__global__ __launch_bounds__(256, 4) void conv_group_mfma_i8_kernel(ConvArgs a, GmGeom g)
{
    constexpr int NPF = kMulti ? GM_PREFETCH : GM_STAGE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = lane & 31, half = lane >> 5;
    const int u = blockIdx.x;  // unit
    const int tx = blockIdx.y;
    int ty = blockIdx.z, n = 0;
    if (a.N > 1) {
        n = ty / g.tiles_y;
        ty -= n * g.tiles_y;
    }
    const int ox0 = tx * g.btx * 8, oy0 = ty * g.bty * 4;
    const int ix0 = ox0 * a.sw - a.pl, iy0 = oy0 * a.sh - a.pt;  // patch origin in the image
    const char *img = static_cast<const char *>(a.in) + (int64_t)n * a.H * a.W * a.C + (u / g.upg) * g.kc;
    const uint32_t zp4 = (uint32_t)(a.in_zp & 0xff) * 0x01010101u;
    const int npix = g.pw * g.ph;

    // ---- a slab's patch: HBM -> registers (fetch), registers -> LDS (commit); piece = (patch pixel, 16-byte half)
    uint4 pf[NPF];
    auto fetch = [&](int s) {
#pragma unroll
        for (int k = 0; k < NPF; ++k) {
            if (k * 256 >= g.nslots) break;  // uniform
            const int slot = k * 256 + tid;
            const int pix = slot >> 1;
            const int pr = (int)__umulhi((uint32_t)pix, g.pw_magic);
            const int pc = pix - pr * g.pw;
            const int y = iy0 + pr, x = ix0 + pc;
            pf[k] = make_uint4(zp4, zp4, zp4, zp4);
            if (pix < npix && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W)  // (an image is below 2^31 bytes: the pick)
                pf[k] = *reinterpret_cast<const uint4 *>(img + (y * a.W + x) * a.C + s * 32 + (slot & 1) * 16);
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int k = 0; k < NPF; ++k) {
            if (k * 256 >= g.nslots) break;
            const int slot = k * 256 + tid;
            const int pix = slot >> 1;
            const int pr = (int)__umulhi((uint32_t)pix, g.pw_magic);
            const int pc = pix - pr * g.pw;
            if (pix < npix) *reinterpret_cast<uint4 *>(smem + pr * g.row_pitch + pc * GM_PIX_BYTES + (slot & 1) * 16) = pf[k];
        }
    };
    fetch(0);
    commit();
    __syncthreads();

    // ---- this wave's block and its tiles
    const int blk = wave & (g.nblk - 1);
    const int stream = g.nblk == 4 ? 0 : (g.nblk == 2 ? wave >> 1 : wave);
    const int nstream = 4 / g.nblk;
    const int ntile = g.btx * g.bty;
    const int nmine = stream < ntile ? (ntile - stream + nstream - 1) / nstream : 0;  // <= GM_TILES_PER_WAVE (group_mfma.h)
    const int oc0 = (u * g.nblk + blk) * 32;  // first output channel of the block
    const char *wf = static_cast<const char *>(a.w) + (int64_t)(u * g.nblk + blk) * g.nslab * g.ntaps * 1024 + lane * 16;
    const int tab_l = oc0 + 4 * half;  // this lane's first channel in each table (C layout: dw_mfma.h)
    char *outp = static_cast<char *>(a.out) + oc0 + half * 16;
    const int px = row & 7, py = row >> 3;
    const int lane_p0 = (py * a.sh) * g.row_pitch + (px * a.sw) * GM_PIX_BYTES + half * 16;  // tap (0, 0) of tile 0

    // every wave runs the slab loop with its barriers, also one without a tile (NT = 0)
    auto run = [&](auto nt_c) {
        constexpr int NT = decltype(nt_c)::value;
        constexpr int NA = NT ? NT : 1;
        int p0[NA];
        v16i acc[NA];
        if constexpr (NT > 0) {
            v16i ainit;  // acc_init: the folded input zero point
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int4 ai = *reinterpret_cast<const int4 *>(a.acc_init + tab_l + q * 8);
                ainit[4 * q] = ai.x, ainit[4 * q + 1] = ai.y, ainit[4 * q + 2] = ai.z, ainit[4 * q + 3] = ai.w;
            }
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int t = stream + i * nstream;
                const int tby = g.btx == 2 ? t >> 1 : t, tbx = g.btx == 2 ? t & 1 : 0;
                p0[i] = lane_p0 + (tby * 4 * a.sh) * g.row_pitch + (tbx * 8 * a.sw) * GM_PIX_BYTES;
                acc[i] = ainit;
            }
        }
        for (int s = 0; s < (kMulti ? g.nslab : 1); ++s) {
            const bool more = kMulti && s + 1 < g.nslab;
            if (more) fetch(s + 1);  // in flight under this slab's MFMAs
            if constexpr (NT > 0) {
                const char *wp = wf + (int64_t)s * g.ntaps * 1024;
                v4i fa = *reinterpret_cast<const v4i *>(wp);
                for (int tp = 0, ky = 0, kx = 0; tp < g.ntaps; ++tp, ++kx) {
                    if (kx == g.kw) kx = 0, ++ky;
                    v4i fan = fa;  // the next tap's fragment, requested in front of this tap's MFMAs
                    if (tp + 1 < g.ntaps) fan = *reinterpret_cast<const v4i *>(wp + (tp + 1) * 1024);
                    const int off = ky * g.row_pitch + kx * GM_PIX_BYTES;
                    v4i fb[NT];
#pragma unroll
                    for (int i = 0; i < NT; ++i) fb[i] = *reinterpret_cast<const v4i *>(smem + p0[i] + off);
#pragma unroll
                    for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb[i], acc[i], 0, 0, 0);
                    fa = fan;
                }
            }
            if (more) {
                __syncthreads();  // every wave is done with this slab's patch
                commit();
                __syncthreads();
            }
        }
        if constexpr (NT > 0) {
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int t = stream + i * nstream;
                const int tby = g.btx == 2 ? t >> 1 : t, tbx = g.btx == 2 ? t & 1 : 0;
                uint32_t pk[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 mu = *reinterpret_cast<const float4 *>(a.mult + tab_l + q * 8);
                    const float4 bi = *reinterpret_cast<const float4 *>(a.bias + tab_l + q * 8);
                    pk[q] = requant4_i8_t<EPI>(acc[i][4 * q], acc[i][4 * q + 1], acc[i][4 * q + 2], acc[i][4 * q + 3], mu, bi, a);
                }
                const uint4 v = tile_channels_16(pk);  // 16 consecutive channels per lane (dw_mfma.h)
                const int oy = oy0 + tby * 4 + py, ox = ox0 + tbx * 8 + px;
                if (oy < a.Ho && ox < a.Wo) *reinterpret_cast<uint4 *>(outp + (((int64_t)n * a.Ho + oy) * a.Wo + ox) * a.Co) = v;
            }
        }
    };
    switch (nmine) {  // wave-uniform
        case 1: run(std::integral_constant<int, 1>{}); break;
        case 2: run(std::integral_constant<int, 2>{}); break;
        case 3: run(std::integral_constant<int, 3>{}); break;
        case 4: run(std::integral_constant<int, 4>{}); break;
        default: run(std::integral_constant<int, 0>{}); break;
    }
}

// int8, NCHW, symmetric weights and the fast epilogue are the caller's business (conv_plan.hip:group_mfma_takes); this is the
// scope of the geometry, the switch and the measured default rule (group_mfma.h).  N: the plan's batch.
bool conv_group_mfma_pick(int N, int C, int Co, int G, int H, int W, int Ho, int Wo, int Kh, int Kw, int sh, int sw, int dh, int dw)
{
    static const char *env = getenv("SHL_MI355X_GROUPMFMA");  // "0" never, "1" wherever the geometry fits (A/B), default: the measured rule
    if (env && env[0] == '0') return false;
    if (dh != 1 || dw != 1 || N < 1 || H < 1 || W < 1) return false;
    const int64_t M = (int64_t)N * Ho * Wo;
    if (M <= 0 || M >= ((int64_t)1 << 31) || (int64_t)H * W * C >= ((int64_t)1 << 31)) return false;
    GmGeom g;
    if (!gm_geometry(C, Co, G, Kh, Kw, sh, sw, Ho, Wo, N, g)) return false;
    if (env && env[0] == '1') return true;
    return gm_default(M, C, Co, G, Kh * Kw, sh > 1 || sw > 1);
}

size_t conv_group_mfma_weight_bytes(int C, int Co, int G, int Kh, int Kw)
{
    GmGeom g;
    return gm_units(C, Co, G, g) ? (size_t)g.nunits * g.nblk * g.nslab * Kh * Kw * 1024 : 0;
}

void conv_group_mfma_pack(const int8_t *oihw, int C, int Co, int G, int Kh, int Kw, int in_zp, int8_t *dst, int32_t *acc_init)
{
    GmGeom g;
    if (gm_units(C, Co, G, g)) gm_pack(oihw, C, Co, G, Kh, Kw, in_zp, g, dst, acc_init);
}

// a: the NHWC view (conv_plan.hip's re-layout scratch on both sides), a.w the fragment-ordered weights
int launch_conv_group_mfma(const ConvArgs &a, hipStream_t s)
{
    GmGeom g;
    if (a.dh != 1 || a.dw != 1 || !gm_geometry(a.C, a.Co, a.group, a.Kh, a.Kw, a.sh, a.sw, a.Ho, a.Wo, a.N, g)) {
        set_error("conv_group_mfma: group widths, kernel size, stride or grid out of range");
        return SHL_MI355X_ENOTSUP;
    }
    const dim3 grid((unsigned)g.nunits, (unsigned)g.tiles_x, (unsigned)(g.tiles_y * a.N));
    const size_t lds = (size_t)gm_lds_bytes(g);
#define GM_LAUNCH(E)                                                                                             \
    do {                                                                                                         \
        if (g.nslab > 1) hipLaunchKernelGGL((conv_group_mfma_i8_kernel<E, true>), grid, dim3(256), lds, s, a, g); \
        else hipLaunchKernelGGL((conv_group_mfma_i8_kernel<E, false>), grid, dim3(256), lds, s, a, g);           \
    } while (0)
    switch (epi_code(a)) {
        case 0: GM_LAUNCH(0); break;
        case 1: GM_LAUNCH(1); break;
        case 2: GM_LAUNCH(2); break;
        case 3: GM_LAUNCH(3); break;
        case 4: GM_LAUNCH(4); break;
        default: GM_LAUNCH(5); break;
    }
#undef GM_LAUNCH
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

}  // namespace shl

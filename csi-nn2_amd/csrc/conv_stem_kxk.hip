// conv_stem_kxk.hip -- Kh x Kw convolutions with 1..4 input channels (image stems: 7x7 stride 2, 4x4 / 16x16 patchify, 5x5,
// grayscale) for int8 on the matrix cores, on the NHWC view.  The second form of SHL_MI355X_ALGO_STEM.
//
// Such a layer fails igemm_supports (a pixel is fewer than 16 bytes) and ran on conv_direct_kernel, one output per thread.
// conv_stem_i8_mfma_kernel (conv_stem.hip) builds the im2col row of a 3x3 / 3-channel pixel in registers, from the observation
// that ONE FILTER ROW IS ONE CONTIGUOUS RUN of the NHWC input (Kw in_c bytes).  Here the same observation is carried to an LDS
// patch, so that it holds for any Kh x Kw:
//
//   GEMM view  M = output pixels, N = output channels, K = Kh filter rows x (Kw in_c bytes zero-padded to 32 or 64): a filter
//              row is one or two K steps of v_mfma_i32_32x32x32_i8.  7x7x3 is 7 steps, 4x4x3 is 4, 16x16x3 is 32.
//   weights    packed once (stem_kxk.h) as A fragments [block of 32 channels][ky][step][lane][16 B], zeros in the padding: a
//              wave fetches a step's fragment with one coalesced 1 KiB load, one step ahead of its use.  They never touch LDS.
//   workgroup  four waves: a rectangle of btx x bty pixel tiles (8 x 4) of one image x one or two blocks of 32 output channels.
//              The rectangle's input patch with its halo is staged ONCE as plain NHWC bytes [row][x in_c], pixels outside the
//              image as the input zero point (folded into acc_init by the plan), 48 bytes of tail behind the last row.
//   wave       deals the (tile, channel block) pairs out: pair p = wave + 4 i, i < 4 -- one channel block per wave (4 is a
//              multiple of the one or two blocks), up to four tiles, one v16i accumulator each live across the K loop.
//   B operand  for (pixel, ky, step, half) the 16 bytes at row(y sh + ky) + x sw in_c + 32 step + 16 half.  That address is NOT
//              aligned (6 x + 16 half at stride 2 with three channels): the five aligned dwords that cover it are read
//              (ds_read_b32 / ds_read2_b32) and shifted into place with four v_alignbyte_b32; the shift (address & 3) is the
//              lane's own and the same for every step.  What a fragment reads behind its row's last tap -- the next pixels, the
//              next row, the tail -- meets zero weights, and in int32 that is exact.
//   store      requant4_i8_t<EPI>, tile_channels_16 (v_permlane32_swap), one uint4 per lane, masked at the map's edge; where
//              Cout is no multiple of 16 the pieces are unaligned or ragged and go out as dwords or bytes.
//
// An NCHW layer goes through the plan's re-layout scratch in front and behind (conv_plan.hip), as the grouped kernels do.
// Cost, by dwconv_mfma.hip's cycle count (32 cycles per MFMA on one of four matrix pipes) and NOT by measurement: per MFMA a wave
// reads 64 x 20 bytes of LDS (10 cycles of the CU's 128 bytes per cycle), so four waves ask 40 cycles of LDS per 32 of MFMA: the
// K loop is LDS-bound by a quarter when all four waves hold four tiles.  The lanes of a tile row are Cin sw <= 64 bytes apart and
// the rows an odd number of dwords (stem_kxk.h), so a read's lanes fall on a handful of neighbouring dwords per row, many of
// them shared -- argued, not counted.  Measured: profiles/stem_kxk_notes.md.
// Restates shl_ref_conv2d_nhwc_f32 / nchw (source/reference/convolution.c) + relu variants for these shapes.
#include <stdlib.h>

#include <type_traits>

#include "dw_mfma.h"
#include "stem_kxk.h"

namespace shl {

typedef uint32_t sk_u32_a1 __attribute__((aligned(1)));  // a dword at any byte address of the image

template <int EPI>
__global__ __launch_bounds__(256, 2) void conv_stem_kxk_i8_kernel(ConvArgs a, SkGeom g)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = lane & 31, half = lane >> 5;
    const int tx = blockIdx.y;
    int ty = blockIdx.z, n = 0;
    if (a.N > 1) {
        n = ty / g.tiles_y;
        ty -= n * g.tiles_y;
    }
    const int ox0 = tx * g.btx * 8, oy0 = ty * g.bty * 4;
    const int iy0 = oy0 * a.sh - a.pt;
    const int bx0 = (ox0 * a.sw - a.pl) * a.C;  // byte coordinate of the patch's first column in an image row (may be negative)
    const int rowlen = a.W * a.C;
    const char *img = static_cast<const char *>(a.in) + (int64_t)n * a.H * rowlen;  // (an image is below 2^31 bytes: the pick)
    const uint32_t zp4 = (uint32_t)(a.in_zp & 0xff) * 0x01010101u;

    // ---- the patch: dword j = (patch row, dword of the row); whole dwords inside the image row at whatever address, the ones
    // across its ends byte by byte
    {
        const int rdw = g.pitch >> 2;
        for (int j = tid; j < g.ndw; j += 256) {
            const int r = (int)__umulhi((uint32_t)j, g.rdw_magic);
            const int b = bx0 + 4 * (j - r * rdw);
            const int y = iy0 + r;
            uint32_t v = zp4;
            if ((unsigned)y < (unsigned)a.H && b > -4 && b < rowlen) {
                const char *p = img + y * rowlen + b;
                if (b >= 0 && b + 4 <= rowlen) {
                    v = *reinterpret_cast<const sk_u32_a1 *>(p);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (b + k >= 0 && b + k < rowlen) v = (v & ~(0xffu << (8 * k))) | ((uint32_t)(uint8_t)p[k] << (8 * k));
                }
            }
            *reinterpret_cast<uint32_t *>(smem + 4 * j) = v;
        }
    }
    __syncthreads();

    // ---- this wave's channel block and its tiles
    const int cb0 = blockIdx.x * g.ncb;
    const int ncb = g.nblk - cb0 < g.ncb ? g.nblk - cb0 : g.ncb;  // the last workgroup of an odd block count holds one
    const int blk = cb0 + (wave & (ncb - 1));
    const int stream = ncb == 2 ? wave >> 1 : wave;
    const int nstream = 4 / ncb;
    const int ntile = g.btx * g.bty;
    const int nmine = stream < ntile ? (ntile - stream + nstream - 1) / nstream : 0;  // <= SK_PAIRS_PER_WAVE (stem_kxk.h)
    const int oc0 = blk * 32;
    const int nsteps = g.kh * g.spr;
    const char *wf = static_cast<const char *>(a.w) + (int64_t)blk * nsteps * 1024 + lane * 16;
    const int tab_l = oc0 + 4 * half;  // this lane's first channel in each table (C layout: dw_mfma.h)
    const int px = row & 7, py = row >> 3;
    const int lane_a0 = (py * a.sh) * g.pitch + (px * a.sw) * a.C + half * 16;  // byte address of (ky 0, step 0) of tile 0

    auto run = [&](auto nt_c) {
        constexpr int NT = decltype(nt_c)::value;
        int p0[NT];
        uint32_t shift[NT];
        v16i acc[NT];
        {
            v16i ainit;  // acc_init: the folded input zero point (tables are padded to a multiple of 128 entries)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int4 ai = *reinterpret_cast<const int4 *>(a.acc_init + tab_l + q * 8);
                ainit[4 * q] = ai.x, ainit[4 * q + 1] = ai.y, ainit[4 * q + 2] = ai.z, ainit[4 * q + 3] = ai.w;
            }
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int t = stream + i * nstream;
                const int tby = t / g.btx, tbx = t - tby * g.btx;
                const int addr = lane_a0 + (tby * 4 * a.sh) * g.pitch + (tbx * 8 * a.sw) * a.C;
                p0[i] = addr & ~3, shift[i] = (uint32_t)addr & 3u;  // the pitch and the step offsets are multiples of 4
                acc[i] = ainit;
            }
        }
        v4i fa = *reinterpret_cast<const v4i *>(wf);
        for (int st = 0, ky = 0, s = 0; st < nsteps; ++st, ++s) {
            if (s == g.spr) s = 0, ++ky;
            v4i fan = fa;  // the next step's fragment, requested in front of this step's MFMAs
            if (st + 1 < nsteps) fan = *reinterpret_cast<const v4i *>(wf + (st + 1) * 1024);
            const int off = ky * g.pitch + s * 32;
            v4i fb[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const uint32_t *q = reinterpret_cast<const uint32_t *>(smem + p0[i] + off);
                const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
                fb[i][0] = (int)__builtin_amdgcn_alignbyte(d1, d0, shift[i]);
                fb[i][1] = (int)__builtin_amdgcn_alignbyte(d2, d1, shift[i]);
                fb[i][2] = (int)__builtin_amdgcn_alignbyte(d3, d2, shift[i]);
                fb[i][3] = (int)__builtin_amdgcn_alignbyte(d4, d3, shift[i]);
            }
#pragma unroll
            for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb[i], acc[i], 0, 0, 0);
            fa = fan;
        }
        const int c0 = oc0 + half * 16;  // this lane's 16 channels after tile_channels_16
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int t = stream + i * nstream;
            const int tby = t / g.btx, tbx = t - tby * g.btx;
            uint32_t pk[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 mu = *reinterpret_cast<const float4 *>(a.mult + tab_l + q * 8);
                const float4 bi = *reinterpret_cast<const float4 *>(a.bias + tab_l + q * 8);
                pk[q] = requant4_i8_t<EPI>(acc[i][4 * q], acc[i][4 * q + 1], acc[i][4 * q + 2], acc[i][4 * q + 3], mu, bi, a);
            }
            const uint4 v = tile_channels_16(pk);  // 16 consecutive channels per lane (dw_mfma.h)
            const int oy = oy0 + tby * 4 + py, ox = ox0 + tbx * 8 + px;
            if (oy >= a.Ho || ox >= a.Wo || c0 >= a.Co) continue;
            char *o = static_cast<char *>(a.out) + (((int64_t)n * a.Ho + oy) * a.Wo + ox) * a.Co + c0;
            if ((a.Co & 15) == 0) {
                *reinterpret_cast<uint4 *>(o) = v;
            } else {  // pieces at odd addresses, the last one ragged
                const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if ((a.Co & 3) == 0) {
                        if (c0 + 4 * e < a.Co) *reinterpret_cast<uint32_t *>(o + 4 * e) = w4[e];
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (c0 + 4 * e + k < a.Co) o[4 * e + k] = (char)(w4[e] >> (8 * k));
                    }
                }
            }
        }
    };
    switch (nmine) {  // wave-uniform; a wave without a pair is done (no barrier follows)
        case 1: run(std::integral_constant<int, 1>{}); break;
        case 2: run(std::integral_constant<int, 2>{}); break;
        case 3: run(std::integral_constant<int, 3>{}); break;
        case 4: run(std::integral_constant<int, 4>{}); break;
        default: break;
    }
}

// int8, group 1, symmetric weights and the fast epilogue are the caller's business (conv_plan.hip:stem_kxk_takes); this is the
// scope of the geometry and, with by_rule, the measured default rule (stem_kxk.h).  N: the plan's batch.
bool conv_stem_kxk_pick(int N, int C, int Co, int H, int W, int Ho, int Wo, int Kh, int Kw, int sh, int sw, int dh, int dw, int in_zp,
                        bool nchw, bool by_rule)
{
    if (!sk_scope(C, Kh, Kw, sh, sw, dh, dw, in_zp) || N < 1 || H < 1 || W < 1) return false;
    const int64_t M = (int64_t)N * Ho * Wo;
    if (M <= 0 || M >= ((int64_t)1 << 31) || (int64_t)N * H * W * C >= ((int64_t)1 << 31)) return false;
    SkGeom g;
    if (!sk_geometry(C, Co, Kh, Kw, sh, sw, Ho, Wo, N, g)) return false;
    return !by_rule || sk_default(M, C, Co, Kh, Kw, sh, sw, nchw);
}

size_t conv_stem_kxk_weight_bytes(int C, int Co, int Kh, int Kw)
{
    return (size_t)((Co + 31) / 32) * Kh * (Kw * C > 32 ? 2 : 1) * 1024;
}

void conv_stem_kxk_pack(const int8_t *ohwi, int C, int Co, int Kh, int Kw, int in_zp, int8_t *dst, int32_t *acc_init)
{
    SkGeom g = {};
    g.nblk = (Co + 31) / 32, g.spr = Kw * C > 32 ? 2 : 1, g.kh = Kh;
    sk_pack(ohwi, C, Co, Kh, Kw, in_zp, g, dst, acc_init);
}

// a: the NHWC view (conv_plan.hip's re-layout scratch on both sides of an NCHW layer), a.w the fragment-ordered weights
int launch_conv_stem_kxk(const ConvArgs &a, hipStream_t s)
{
    SkGeom g;
    if (a.group != 1 || !sk_scope(a.C, a.Kh, a.Kw, a.sh, a.sw, a.dh, a.dw, a.in_zp) ||
        (int64_t)a.N * a.H * a.W * a.C >= ((int64_t)1 << 31) || !sk_geometry(a.C, a.Co, a.Kh, a.Kw, a.sh, a.sw, a.Ho, a.Wo, a.N, g)) {
        set_error("conv_stem_kxk: channels, kernel size, stride or grid out of range");
        return SHL_MI355X_ENOTSUP;
    }
    const dim3 grid((unsigned)((g.nblk + g.ncb - 1) / g.ncb), (unsigned)g.tiles_x, (unsigned)(g.tiles_y * a.N));
    const size_t lds = (size_t)sk_lds_bytes(g);
    switch (epi_code(a)) {
        case 0: hipLaunchKernelGGL((conv_stem_kxk_i8_kernel<0>), grid, dim3(256), lds, s, a, g); break;
        case 1: hipLaunchKernelGGL((conv_stem_kxk_i8_kernel<1>), grid, dim3(256), lds, s, a, g); break;
        case 2: hipLaunchKernelGGL((conv_stem_kxk_i8_kernel<2>), grid, dim3(256), lds, s, a, g); break;
        case 3: hipLaunchKernelGGL((conv_stem_kxk_i8_kernel<3>), grid, dim3(256), lds, s, a, g); break;
        case 4: hipLaunchKernelGGL((conv_stem_kxk_i8_kernel<4>), grid, dim3(256), lds, s, a, g); break;
        default: hipLaunchKernelGGL((conv_stem_kxk_i8_kernel<5>), grid, dim3(256), lds, s, a, g); break;
    }
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

}  // namespace shl

// dwconv_kxk.hip -- depthwise Kh x Kw (1..7 per axis, not 3x3) int8 NHWC: matrix cores + LDS patch, taps outermost.
//
// The generic kernel (dwconv.hip, dwconv_nhwc_kernel<true, 0>) runs these layers -- MobileNetV3 / EfficientNet / MnasNet 5x5,
// ConvNeXt 7x7 -- one thread per four channels of an output pixel: Kh Kw dependent loads behind bounds branches, four VALU
// operations per multiply-add, every input byte fetched 25 or 49 times through L1.  dwconv_mfma.hip's idea carries over -- the
// patch goes HBM -> LDS once, a depthwise tap is one v_mfma_i32_32x32x32_i8 against diag(w_tap) -- but not its loop: it holds
// the nine diagonal fragments per wave, and 25 or 49 of them are 100 or 196 registers.  Here the loop is inverted:
//
//   workgroup  a rectangle of output pixels (btx x bty MFMA pixel tiles of 8 x 4; dw_kxk.h) x a block of cb = 32 / 64 / 128
//              channels.  Patch (+ halo Kh - 1, Kw - 1) HBM -> LDS once with global_load_lds_dwordx4; pixels outside the image
//              come from the pad page (= the input zero point, folded into acc_init): no bounds checks afterwards.
//              [pixel][cb], 16-byte slot XOR-swizzled by the pixel (dw_patch_swizzle).  Behind the patch: the epilogue tables
//              [acc_init | mult | bias][cb], the block's weights [tap][cb] as the plan keeps them (plain 1HWO, no packing) and,
//              in a fused launch, the table.  One barrier.
//   wave       one 32-channel group x up to FOUR pixel tiles (128 / cb waves deal a group's tiles out), one v16i accumulator
//              per tile live across the tap loop
//   per tap    one weight byte per lane from LDS -> the diagonal A fragment (a multiply and four ANDs against masks that place
//              the byte as dw_diag_fragments does), the tap's swizzled offset (~10 VALU), then per tile one ds_read_b128 and
//              one MFMA.  The first tap's C operand is acc_init.
//   store      dwconv_mfma.hip's: requantise from the LDS tables, tile_channels_16, one uint4 per lane, masked at the map's edge
//
// Bank conflicts under tap offsets up to 6 (dw_patch_swizzle was chosen for 0..2), by reasoning: the swizzle reads only low
// bits of the patch row and column (stride 1: pc bit 1, pr bits 0-1; stride 2: pc bits 1-2, pr bit 1), and the lanes a
// ds_read_b128 serves together cover every value of those bits.  A tap moves ALL of them by the same (ky, kx), which permutes
// the residues they cover: the set of (bank half, slot) pairs, and so the conflict degree, is that of tap (0, 0) for every
// offset -- conflict-free at stride 1, two-way at stride 2 and at mixed strides, as in the 3x3 kernel.  The one condition is
// the one dw_mfma.h names, an even row pitch at stride 1 (the pixel's bank half must depend on the column alone): 8 btx - 1 + Kw
// is odd for an even Kw, so dwk_patch rounds the pitch up by one column there.
//
// Cost, by dwconv_mfma.hip's cycle count (32 cycles per MFMA on one of four matrix pipes) and NOT by measurement: 25 MFMAs per
// 1 024 outputs put 5x5 near the HBM rate, 49 put 7x7 on the matrix pipes.  Measured: profiles/dw_kxk_notes.md.
// LDS: patch + 12 cb + Kh Kw cb (+ 256) bytes, at most 48 KiB where the rectangle can shrink to it, never above 80 KiB.  48 KiB
// (three workgroups per CU) over 80 KiB (two, with larger rectangles and less halo) is argued too, not measured: no A/B of the
// two targets was run.
// Registers (tools/dev/kregs.py): 114 - 118 VGPRs, 0 AGPRs, no scratch in the twelve instantiations -- four waves per SIMD;
// build.py's NO_SPILL_SOURCES holds it there.
// Restates shl_ref_depthwise_conv2d_quant (source/reference/convolution.c:416-460) + relu variants.
#include <stdlib.h>

#include <type_traits>

#include "dw_kxk.h"
#include "dw_mfma.h"
#include "igemm_common.h"
#include "lut_step.h"

namespace shl {

template <int EPI, bool kLut = false>
__global__ __launch_bounds__(256, 4) void dwconv_kxk_i8_mfma_kernel(typename std::conditional<kLut, LutConvArgs, ConvArgs>::type a, DwkGeom g)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = lane & 31, half = lane >> 5;
    const int cblk = blockIdx.x;  // channel block
    const int tx = blockIdx.y;
    int ty = blockIdx.z, n = 0;
    if (a.N > 1) {
        n = ty / g.tiles_y;
        ty -= n * g.tiles_y;
    }
    const int ox0 = tx * g.btx * 8, oy0 = ty * g.bty * 4;
    const int ix0 = ox0 * a.sw - a.pl, iy0 = oy0 * a.sh - a.pt;  // patch origin in the image
    const int nch = g.cb >> 4, nch_mask = nch - 1;               // 16-byte slots per pixel
    const int nch_shift = nch == 8 ? 3 : (nch == 4 ? 2 : 1);
    const bool s2 = a.sw == 2;

    // ---- patch -> LDS: piece k fills LDS bytes [k * 1024, +1024), lane = one 16-byte slot
    const char *img = static_cast<const char *>(a.in) + (int64_t)n * a.H * a.W * a.C + cblk * g.cb;
    const char *pad = static_cast<const char *>(a.pad_page) + (lane << 4);
    const int npix = g.pw * g.ph;
    for (int k = wave; k < g.npieces; k += 4) {
        const int slot = k * 64 + lane;
        const int pix = slot >> nch_shift, j = slot & nch_mask;
        const int pr = (int)__umulhi((uint32_t)pix, g.pw_magic);
        const int pc = pix - pr * g.pw;
        const int y = iy0 + pr, x = ix0 + pc;
        const bool ok = pix < npix && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W;
        const char *src = img + ((int64_t)y * a.W + x) * a.C + ((j ^ (dw_patch_swizzle(s2, pr, pc) & nch_mask)) << 4);
        glds16(ok ? src : pad, smem + k * 1024);
    }
    // ---- the channel block's epilogue tables and its weights -> LDS
    char *tab = smem + g.npieces * 1024;
    {
        const int q4 = g.cb >> 2;  // 16-byte pieces per table
        if (tid < 3 * q4) {
            const int which = tid / q4, i = tid - which * q4;
            const void *src = which == 0 ? (const void *)(a.acc_init + cblk * g.cb)
                              : which == 1 ? (const void *)(a.mult + cblk * g.cb) : (const void *)(a.bias + cblk * g.cb);
            reinterpret_cast<uint4 *>(tab)[which * q4 + i] = static_cast<const uint4 *>(src)[i];
        }
    }
    char *wl = tab + g.cb * 12;  // [tap][cb]
    {
        const char *wsrc = static_cast<const char *>(a.w) + cblk * g.cb;
        for (int i = tid; i < g.ntaps * nch; i += 256) {
            const int tp = i >> nch_shift, j = i & nch_mask;
            reinterpret_cast<uint4 *>(wl)[i] = *reinterpret_cast<const uint4 *>(wsrc + (int64_t)tp * a.C + (j << 4));
        }
    }
    const uint8_t *lut = nullptr;
    if constexpr (kLut) {  // the first wave copies, one dword per lane; the barrier below publishes
        uint32_t *lut_lds = reinterpret_cast<uint32_t *>(wl + ((g.ntaps * g.cb + 15) & ~15));
        if (tid < 64) late_lut(lut_lds);
        lut = reinterpret_cast<const uint8_t *>(lut_lds);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- this wave's channel group and its tiles
    const int ncg = g.cb >> 5;  // channel groups per workgroup: 1, 2 or 4
    const int cgl = wave & (ncg - 1);
    const int stream = ncg == 4 ? 0 : (ncg == 2 ? wave >> 1 : wave);
    const int nstream = 4 / ncg;
    const int ntile = g.btx * g.bty;
    const int nmine = stream < ntile ? (ntile - stream + nstream - 1) / nstream : 0;  // <= DWK_TILES_PER_WAVE (dw_kxk.h)
    const int ch0 = cblk * g.cb + cgl * 32;  // first channel of the group
    const int lchunk = cgl * 2 + half;       // this lane's logical 16-byte slot inside a pixel
    const char *tab_l = tab + (cgl * 32 + 4 * half) * 4;  // this lane's first channel in each table
    const int tab_stride = g.cb * 4;
    const uint8_t *w_l = reinterpret_cast<const uint8_t *>(wl) + cgl * 32 + row;  // this lane's channel, tap 0
    char *outp = static_cast<char *>(a.out) + ch0 + half * 16;
    // where diag(w) has this lane's byte: matrix row `row`, k = 16 half .. +15 -- dword (row & 15) >> 2, byte row & 3, and only
    // where row >> 4 == half (dw_diag_fragments' placement, as masks against the byte replicated four times)
    uint32_t wmask[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) wmask[k] = ((row >> 4) == half && k == ((row & 15) >> 2)) ? 0xFFu << (8 * (row & 3)) : 0u;
    const int px = row & 7, py = row >> 3;
    const int lane_p0 = ((py * a.sh) * g.pw + px * a.sw) * g.cb;  // tap (0, 0) of tile 0

    auto run = [&](auto nt_c) {
        constexpr int NT = decltype(nt_c)::value;
        int p0[NT];
        v16i acc[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int t = stream + i * nstream;
            const int tby = g.btx == 2 ? t >> 1 : t, tbx = g.btx == 2 ? t & 1 : 0;
            p0[i] = lane_p0 + ((tby * 4 * a.sh) * g.pw + tbx * 8 * a.sw) * g.cb;
        }
        // a tile moves a lane's pixel by multiples of 4 rows and 8 columns (stride 2: 8 and 16) and the swizzle looks at lower
        // bits only, so a tap's offset is the same for every tile of the wave
        auto tap = [&](int tp, int ky, int kx, auto first) {
            const int sz = dw_patch_swizzle(s2, py * a.sh + ky, px * a.sw + kx) & nch_mask;
            const int off = (ky * g.pw + kx) * g.cb + ((lchunk ^ sz) << 4);
            const uint32_t wb = (uint32_t)w_l[tp * g.cb] * 0x01010101u;
            v4i fa, fb[NT];
#pragma unroll
            for (int k = 0; k < 4; ++k) fa[k] = (int)(wb & wmask[k]);
#pragma unroll
            for (int i = 0; i < NT; ++i) fb[i] = *reinterpret_cast<const v4i *>(smem + p0[i] + off);
            if constexpr (decltype(first)::value) {
                v16i ainit;  // acc_init (the folded input zero point): the first MFMA's C operand, no copy per tile
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int4 ai = *reinterpret_cast<const int4 *>(tab_l + q * 32);
                    ainit[4 * q] = ai.x, ainit[4 * q + 1] = ai.y, ainit[4 * q + 2] = ai.z, ainit[4 * q + 3] = ai.w;
                }
#pragma unroll
                for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb[i], ainit, 0, 0, 0);
            } else {
#pragma unroll
                for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb[i], acc[i], 0, 0, 0);
            }
        };
        tap(0, 0, 0, std::true_type{});
        for (int tp = 1, ky = 0, kx = 1; tp < g.ntaps; ++tp, ++kx) {
            if (kx == g.kw) kx = 0, ++ky;
            tap(tp, ky, kx, std::false_type{});
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int t = stream + i * nstream;
            const int tby = g.btx == 2 ? t >> 1 : t, tbx = g.btx == 2 ? t & 1 : 0;
            uint32_t pk[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 mu = *reinterpret_cast<const float4 *>(tab_l + tab_stride + q * 32);
                const float4 bi = *reinterpret_cast<const float4 *>(tab_l + 2 * tab_stride + q * 32);
                pk[q] = requant4_i8_t<EPI>(acc[i][4 * q], acc[i][4 * q + 1], acc[i][4 * q + 2], acc[i][4 * q + 3], mu, bi, a);
                if constexpr (kLut) pk[q] = lut4(lut, pk[q]);
            }
            const uint4 v = tile_channels_16(pk);  // 16 consecutive channels per lane (dw_mfma.h)
            const int oy = oy0 + tby * 4 + py, ox = ox0 + tbx * 8 + px;
            if (oy < a.Ho && ox < a.Wo) *reinterpret_cast<uint4 *>(outp + (((int64_t)n * a.Ho + oy) * a.Wo + ox) * a.C) = v;
        }
    };
    switch (nmine) {  // wave-uniform
        case 1: run(std::integral_constant<int, 1>{}); break;
        case 2: run(std::integral_constant<int, 2>{}); break;
        case 3: run(std::integral_constant<int, 3>{}); break;
        case 4: run(std::integral_constant<int, 4>{}); break;
        default: break;
    }
}

// int8 NHWC, depth multiplier 1, dilation 1 and plain [tap][C] weights are the caller's business (dwconv_i8_kernel,
// conv_plan.hip); this is the scope of the geometry, the switch and the measured size rule (dw_kxk.h)
bool dwconv_kxk_pick(int64_t M, int N, int C, int H, int W, int Ho, int Wo, int Kh, int Kw, int sh, int sw)
{
    if (M <= 0 || M >= ((int64_t)1 << 31) || (int64_t)H * W * C >= ((int64_t)1 << 31)) return false;
    static const char *env = getenv("SHL_MI355X_DWKXK");  // "0" never, "1" wherever the geometry fits (A/B), default: by size
    if (env && env[0] == '0') return false;
    DwkGeom g;
    if (!dwk_geometry(C, Kh, Kw, sh, sw, Ho, Wo, N, g)) return false;
    if (env && env[0] == '1') return true;
    return dwk_default(M, C, Kh * Kw, sh > 1 || sw > 1);
}

template <bool kLut>
static int launch_dwconv_kxk_t(const typename std::conditional<kLut, LutConvArgs, ConvArgs>::type &a, hipStream_t s)
{
    DwkGeom g;
    if (a.dh != 1 || a.dw != 1 || a.C != a.Co || !dwk_geometry(a.C, a.Kh, a.Kw, a.sh, a.sw, a.Ho, a.Wo, a.N, g)) {
        set_error("dwconv_kxk: kernel size, stride or grid out of range");
        return SHL_MI355X_ENOTSUP;
    }
    const dim3 grid((unsigned)(a.C / g.cb), (unsigned)g.tiles_x, (unsigned)(g.tiles_y * a.N));
    const size_t lds = (size_t)dwk_lds_bytes(g, kLut);
    static LdsOptIn opted[6];
    {
        const void *fns[6] = {reinterpret_cast<const void *>(dwconv_kxk_i8_mfma_kernel<0, kLut>), reinterpret_cast<const void *>(dwconv_kxk_i8_mfma_kernel<1, kLut>),
                              reinterpret_cast<const void *>(dwconv_kxk_i8_mfma_kernel<2, kLut>), reinterpret_cast<const void *>(dwconv_kxk_i8_mfma_kernel<3, kLut>),
                              reinterpret_cast<const void *>(dwconv_kxk_i8_mfma_kernel<4, kLut>), reinterpret_cast<const void *>(dwconv_kxk_i8_mfma_kernel<5, kLut>)};
        const int e = epi_code(a);
        if (e >= 0 && e < 6) lds_opt_in(opted[e], fns[e]);
    }
    switch (epi_code(a)) {
        case 0: hipLaunchKernelGGL((dwconv_kxk_i8_mfma_kernel<0, kLut>), grid, dim3(256), lds, s, a, g); break;
        case 1: hipLaunchKernelGGL((dwconv_kxk_i8_mfma_kernel<1, kLut>), grid, dim3(256), lds, s, a, g); break;
        case 2: hipLaunchKernelGGL((dwconv_kxk_i8_mfma_kernel<2, kLut>), grid, dim3(256), lds, s, a, g); break;
        case 3: hipLaunchKernelGGL((dwconv_kxk_i8_mfma_kernel<3, kLut>), grid, dim3(256), lds, s, a, g); break;
        case 4: hipLaunchKernelGGL((dwconv_kxk_i8_mfma_kernel<4, kLut>), grid, dim3(256), lds, s, a, g); break;
        default: hipLaunchKernelGGL((dwconv_kxk_i8_mfma_kernel<5, kLut>), grid, dim3(256), lds, s, a, g); break;
    }
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

int launch_dwconv_kxk(const ConvArgs &a, hipStream_t s) { return launch_dwconv_kxk_t<false>(a, s); }

int launch_dwconv_kxk_lut(const LutConvArgs &a, hipStream_t s) { return launch_dwconv_kxk_t<true>(a, s); }

}  // namespace shl

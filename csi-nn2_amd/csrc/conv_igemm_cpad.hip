// conv_igemm_cpad.hip -- dense int8 convolutions whose input channel count is NOT a multiple of 16 (24, 40, 58, 72, 116, 120,
// 184, 200, 232: the pointwise and 3x3 layers of MobileNetV2 / V3, EfficientNet and ShuffleNetV2) on the matrix cores, on the
// NHWC view.  The second form of a SHL_MI355X_ALGO_DIRECT plan (conv_plan.hip: kstride == 16), chosen for ALGO_AUTO only.
//
// Such a layer fails igemm_supports (a pixel is no whole number of 16-byte chunks) and ran on conv_direct_kernel, one output per
// thread.  Here the pixel is PADDED to whole chunks where it costs nothing -- in LDS and in the packed weights:
//
//   GEMM view  M = output pixels (B operand, 32 per tile), N = output channels (A operand, blocks of 32), K = Kh Kw taps x Cp
//              bytes, Cp = in_c rounded up to 16.  One v_mfma_i32_32x32x32_i8 step is two 16-byte chunks; chunk q is tap
//              q / (Cp / 16), channels 16 (q % (Cp / 16)) .. + 15, so a step may straddle two taps (Cp = 48); an odd chunk count
//              ends in a half step whose weights are zero (its B half re-reads the last chunk).
//   weights    packed once (cpad.h) as A fragments [block of 32 channels][step][lane][16 B], zeros in the channel padding, in
//              the K tail and beyond Cout: a wave fetches a step's fragment with one coalesced 1 KiB load, one step ahead of its
//              use.  They never touch LDS.  acc_init carries -zp_in sum(w) over the real channels of all taps.
//   workgroup  four waves: a rectangle of btx x bty pixel tiles (8 x 4) of one image x one or two blocks of 32 output channels.
//              The rectangle's input patch with its halo is staged ONCE, re-pitched [row][x][pp]: a pixel's in_c bytes, then
//              Cp - in_c zero bytes; pixels outside the image hold zp_in in the real channels.  Every B fragment is then ONE
//              aligned ds_read_b128 whatever in_c is.  How many tiles a wave holds (1 .. 4) grows with the layer, so that a
//              small layer still makes a few hundred workgroups (cpad.h:cp_geometry).
//   pitches    CHANGED from "row pitch" to the PIXEL pitch: pp = Cp, plus 16 bytes where Cp / 16 is even, i.e. always an odd
//              number of 16-byte slots.  The lanes of a fragment read are one pixel apart (stride 1), so with an even slot count
//              (Cp = 32, 64, 128: 24, 58, 116 channels) they would share 8, 4 or 2 of the 16 slots of a bank line; an odd count
//              walks all 16.  The row pitch is made odd in slots as well (tile rows then start on different slots).  At stride
//              2 the lanes are 2 pp apart and share slots in pairs.  REASONED, not counted.
//   staging    one item = one dword of the patch; a thread takes eight items at a time, issues ALL their global loads, then
//              writes LDS.  Loads are aligned dwords only: a pixel starts at any byte when in_c % 4 != 0, so an item reads the one
//              or two aligned dwords that cover its four bytes and shifts them into place with v_alignbyte_b32 (in_c % 4 == 0:
//              always one).  A dword that would end behind the tensor's last byte is read byte by byte, so nothing outside the
//              input is touched.  16-byte loads are NOT used: a pixel of 24 or 40 bytes is 16-byte aligned every second pixel
//              only, and the re-pitch scatters a vector's dwords over two pixels -- dwords keep one code path (not measured).
//   pointwise  1x1, stride 1, no padding (FLAT): no halo, no rows -- a tile is 32 CONSECUTIVE pixels of the [N H W] order, the
//              patch one contiguous run of the input, chunk q of a pixel is at 16 q (no offset table, no tile raggedness at the
//              map's edge: 7x7 and 14x14 maps fill their tiles across images).  Otherwise a lane reads its step's chunk offset
//              from a small table in LDS, one step ahead.
//   store      requant4_i8_t<EPI>, tile_channels_16 (v_permlane32_swap): 16 consecutive channels per lane; one uint4 where
//              Cout % 16 == 0, dwords where Cout % 4 == 0, bytes otherwise; masked at the map's edge and behind Cout.
//
// An NCHW layer goes through the plan's re-layout scratch in front and behind (conv_plan.hip), as the grouped kernels do.
// Pointers: the input must be 4-byte aligned (the staging's aligned dwords are counted from it), the output as its store form
// needs -- 16 bytes where Cout % 16 == 0, 4 where Cout % 4 == 0, none for byte stores; anything else is EINVAL, where the direct
// kernel took any pointer.  A runtime batch above the plan's re-derives the geometry; should it then exceed a grid limit the call
// is ENOTSUP with no way back to the direct kernel, because the plan's weights are fragment-packed (N Ho Wo beyond ~10^7 pixels).
// Measured against the direct kernel: profiles/cpad_notes.md.
// Restates shl_ref_conv2d_nhwc (source/reference/convolution.c) + relu variants for these shapes.
#include <stdlib.h>

#include <type_traits>

#include "cpad.h"
#include "dw_mfma.h"

namespace shl {

constexpr int CP_STAGE_BATCH = 8;  // items whose loads a thread has in flight before its first LDS write

// the aligned dword at byte offset ga of the input; the bytes behind the tensor's end (total) are not read
__device__ __forceinline__ uint32_t cp_load_dword(const char *in, int ga, int total)
{
    if (ga + 4 <= total) return *reinterpret_cast<const uint32_t *>(in + ga);
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
        if (ga + k < total) v |= (uint32_t)(uint8_t)in[ga + k] << (8 * k);
    return v;
}

template <int EPI, bool FLAT>
__global__ __launch_bounds__(256, 2) void conv_igemm_cpad_i8_kernel(ConvArgs a, CpGeom g)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = lane & 31, half = lane >> 5;
    int n = 0, ox0 = 0, oy0 = 0, p0 = 0;
    if constexpr (FLAT) {
        p0 = blockIdx.y * g.btx * 32;
    } else {
        int ty = blockIdx.z;
        if (a.N > 1) {
            n = ty / g.tiles_y;
            ty -= n * g.tiles_y;
        }
        ox0 = blockIdx.y * g.btx * 8, oy0 = ty * g.bty * 4;
    }
    const int iy0 = oy0 * a.sh - a.pt, ix0 = ox0 * a.sw - a.pl;
    const char *in = static_cast<const char *>(a.in);
    const int total = a.N * a.H * a.W * a.C;  // (below 2^31: cp_geometry)
    const uint32_t zp4 = (uint32_t)(a.in_zp & 0xff) * 0x01010101u;

    // ---- the patch: item j = (staged pixel, dword of its Cp bytes)
    {
        const int dpp = g.cp >> 2;
        // -> LDS byte address, byte offset in the input (-1: outside the image), real bytes of the dword (0 .. 4)
        auto decode = [&](int j, int &lds, int &goff, int &nb) {
            const int pix = (int)__umulhi((uint32_t)j, g.dq_magic);
            const int d = j - pix * dpp;
            nb = a.C - 4 * d;
            nb = nb < 0 ? 0 : nb > 4 ? 4 : nb;
            if constexpr (FLAT) {
                const int p = p0 + pix;
                lds = pix * g.pp + 4 * d;
                goff = p < a.M ? p * a.C + 4 * d : -1;
            } else {
                const int r = (int)__umulhi((uint32_t)pix, g.pw_magic);
                const int x = pix - r * g.pw;
                const int y = iy0 + r, xx = ix0 + x;
                lds = g.tab_bytes + r * g.pitch + x * g.pp + 4 * d;
                goff = ((unsigned)y < (unsigned)a.H && (unsigned)xx < (unsigned)a.W) ? ((n * a.H + y) * a.W + xx) * a.C + 4 * d : -1;
            }
        };
        for (int j0 = tid; j0 < g.nitems; j0 += 256 * CP_STAGE_BATCH) {
            uint32_t lo[CP_STAGE_BATCH], hi[CP_STAGE_BATCH];
#pragma unroll
            for (int b = 0; b < CP_STAGE_BATCH; ++b) {
                const int j = j0 + 256 * b;
                lo[b] = zp4, hi[b] = zp4;
                if (j < g.nitems) {
                    int lds, goff, nb;
                    decode(j, lds, goff, nb);
                    if (goff >= 0 && nb > 0) {
                        const int ga = goff & ~3;
                        lo[b] = cp_load_dword(in, ga, total);
                        if ((goff & 3) + nb > 4) hi[b] = cp_load_dword(in, ga + 4, total);  // (its first byte is the item's own: inside)
                    }
                }
            }
#pragma unroll
            for (int b = 0; b < CP_STAGE_BATCH; ++b) {
                const int j = j0 + 256 * b;
                if (j < g.nitems) {
                    int lds, goff, nb;
                    decode(j, lds, goff, nb);
                    const uint32_t v = goff >= 0 ? __builtin_amdgcn_alignbyte(hi[b], lo[b], (uint32_t)goff & 3u) : zp4;
                    const uint32_t mask = nb >= 4 ? 0xffffffffu : (1u << (8 * nb)) - 1u;
                    *reinterpret_cast<uint32_t *>(smem + lds) = v & mask;
                }
            }
        }
        if constexpr (!FLAT) {  // byte offset of chunk q from a pixel's first tap; entries behind the last chunk repeat it
            for (int q = tid; q < 2 * g.nsteps + 2; q += 256) {
                const int qq = q < g.nchunk ? q : g.nchunk - 1;
                const int tap = qq / g.cpc, c = qq - tap * g.cpc, ky = tap / a.Kw, kx = tap - ky * a.Kw;
                reinterpret_cast<int *>(smem)[q] = ky * g.pitch + kx * g.pp + 16 * c;
            }
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
    const int nmine = stream < ntile ? (ntile - stream + nstream - 1) / nstream : 0;  // <= CP_PAIRS_PER_WAVE (cpad.h)
    const int oc0 = blk * 32;
    const int nsteps = g.nsteps;
    const char *wf = static_cast<const char *>(a.w) + (int64_t)blk * nsteps * 1024 + lane * 16;
    const int tab_l = oc0 + 4 * half;  // this lane's first channel in each table (C layout: dw_mfma.h)
    const int px = row & 7, py = row >> 3;

    auto run = [&](auto nt_c) {
        constexpr int NT = decltype(nt_c)::value;
        int base[NT];
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
                if constexpr (FLAT) {
                    base[i] = (t * 32 + row) * g.pp;
                } else {
                    const int tby = t / g.btx, tbx = t - tby * g.btx;
                    base[i] = g.tab_bytes + ((tby * 4 + py) * a.sh) * g.pitch + ((tbx * 8 + px) * a.sw) * g.pp;
                }
                acc[i] = ainit;
            }
        }
        v4i fa = *reinterpret_cast<const v4i *>(wf);
        const int qlast = g.nchunk - 1;
        int off = 0;
        if constexpr (FLAT) off = 16 * (half < qlast ? half : qlast);
        else off = reinterpret_cast<const int *>(smem)[half];
        for (int st = 0; st < nsteps; ++st) {
            v4i fan = fa;  // the next step's fragment, requested in front of this step's MFMAs
            if (st + 1 < nsteps) fan = *reinterpret_cast<const v4i *>(wf + (st + 1) * 1024);
            int offn;  // the next step's chunk offset (the table holds two entries behind the last step)
            if constexpr (FLAT) {
                const int q = 2 * st + 2 + half;
                offn = 16 * (q < qlast ? q : qlast);
            } else {
                offn = reinterpret_cast<const int *>(smem)[2 * st + 2 + half];
            }
            v4i fb[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) fb[i] = *reinterpret_cast<const v4i *>(smem + base[i] + off);
#pragma unroll
            for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb[i], acc[i], 0, 0, 0);
            fa = fan;
            off = offn;
        }
        const int c0 = oc0 + half * 16;  // this lane's 16 channels after tile_channels_16
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int t = stream + i * nstream;
            uint32_t pk[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 mu = *reinterpret_cast<const float4 *>(a.mult + tab_l + q * 8);
                const float4 bi = *reinterpret_cast<const float4 *>(a.bias + tab_l + q * 8);
                pk[q] = requant4_i8_t<EPI>(acc[i][4 * q], acc[i][4 * q + 1], acc[i][4 * q + 2], acc[i][4 * q + 3], mu, bi, a);
            }
            const uint4 v = tile_channels_16(pk);  // 16 consecutive channels per lane (dw_mfma.h)
            int64_t pix;
            if constexpr (FLAT) {
                pix = p0 + t * 32 + row;
                if (pix >= a.M) continue;
            } else {
                const int tby = t / g.btx, tbx = t - tby * g.btx;
                const int oy = oy0 + tby * 4 + py, ox = ox0 + tbx * 8 + px;
                if (oy >= a.Ho || ox >= a.Wo) continue;
                pix = ((int64_t)n * a.Ho + oy) * a.Wo + ox;
            }
            if (c0 >= a.Co) continue;
            char *o = static_cast<char *>(a.out) + pix * a.Co + c0;
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

// int8, group 1, symmetric weights and the fast epilogue are the caller's business (conv_plan.hip:cpad_takes); this is the scope,
// the geometry and, with by_rule, the measured default rule (cpad.h).  N: the plan's batch.
bool conv_igemm_cpad_pick(int N, int C, int Co, int H, int W, int Ho, int Wo, int Kh, int Kw, int sh, int sw, int pt, int pl, int dh, int dw,
                          int in_zp, bool nchw, bool by_rule)
{
    CpGeom g;
    if (!cp_scope(C, Kh, Kw, sh, sw, dh, dw, in_zp) || !cp_geometry(C, Co, Kh, Kw, sh, sw, pt, pl, H, W, Ho, Wo, N, g)) return false;
    return !by_rule || cp_default((int64_t)N * Ho * Wo, C, Co, Kh, Kw, sh, sw, nchw);
}

size_t conv_igemm_cpad_weight_bytes(int C, int Co, int Kh, int Kw)
{
    const int nchunk = Kh * Kw * ((C + 15) / 16);
    return (size_t)((Co + 31) / 32) * ((nchunk + 1) / 2) * 1024;
}

void conv_igemm_cpad_pack(const int8_t *ohwi, int C, int Co, int Kh, int Kw, int in_zp, int8_t *dst, int32_t *acc_init)
{
    CpGeom g = {};
    g.cpc = (C + 15) / 16, g.nchunk = Kh * Kw * g.cpc, g.nsteps = (g.nchunk + 1) / 2, g.nblk = (Co + 31) / 32;
    cp_pack(ohwi, C, Co, Kh, Kw, in_zp, g, dst, acc_init);
}

// a: the NHWC view (conv_plan.hip's re-layout scratch on both sides of an NCHW layer), a.w the fragment-ordered weights
int launch_conv_igemm_cpad(const ConvArgs &a, hipStream_t s)
{
    CpGeom g;
    if (a.group != 1 || !cp_scope(a.C, a.Kh, a.Kw, a.sh, a.sw, a.dh, a.dw, a.in_zp) ||
        !cp_geometry(a.C, a.Co, a.Kh, a.Kw, a.sh, a.sw, a.pt, a.pl, a.H, a.W, a.Ho, a.Wo, a.N, g)) {
        set_error("conv_igemm_cpad: channels, kernel size, stride, LDS patch or grid out of range");
        return SHL_MI355X_ENOTSUP;
    }
    const uintptr_t out_mask = (a.Co & 15) == 0 ? 15 : (a.Co & 3) == 0 ? 3 : 0;  // uint4 / dword / byte stores
    if (((uintptr_t)a.in & 3) || ((uintptr_t)a.out & out_mask)) {
        set_error("conv_igemm_cpad: the input must be 4-byte aligned, the output %d-byte (its store form)", (int)out_mask + 1);
        return SHL_MI355X_EINVAL;
    }
    const dim3 grid((unsigned)((g.nblk + g.ncb - 1) / g.ncb), (unsigned)g.tiles_x, (unsigned)(g.tiles_y * (g.flat ? 1 : a.N)));
    const size_t lds = (size_t)cp_lds_bytes(g);
#define SHL_CPAD_LAUNCH(E)                                                                                         \
    if (g.flat) hipLaunchKernelGGL((conv_igemm_cpad_i8_kernel<E, true>), grid, dim3(256), lds, s, a, g);         \
    else hipLaunchKernelGGL((conv_igemm_cpad_i8_kernel<E, false>), grid, dim3(256), lds, s, a, g);               \
    break
    switch (epi_code(a)) {
        case 0: SHL_CPAD_LAUNCH(0);
        case 1: SHL_CPAD_LAUNCH(1);
        case 2: SHL_CPAD_LAUNCH(2);
        case 3: SHL_CPAD_LAUNCH(3);
        case 4: SHL_CPAD_LAUNCH(4);
        default: SHL_CPAD_LAUNCH(5);
    }
#undef SHL_CPAD_LAUNCH
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

}  // namespace shl

// cpad.h -- the host half of conv_igemm_cpad.hip (dense int8 convolutions whose input channel count is no multiple of 16, on the
// matrix cores over an LDS patch re-pitched to whole 16-byte chunks): which layers the kernel takes, how the output is cut into
// workgroup rectangles, the LDS patch and its budget, the plan-time weight packing and the default rule.  Pure host code that
// includes no HIP header, so that a stand-alone program can compile it with the sanitizers (tests/test_cpad_cpu.py).
#pragma once
#include <stdint.h>
#include <string.h>

namespace shl {

constexpr int CP_MIN_C = 8;              // below: the stem kernels' (1..4 channels) or the direct kernel's
constexpr int CP_MAX_K = 7;              // taps per axis
constexpr int CP_MAX_STRIDE = 4;
constexpr int CP_PAIRS_PER_WAVE = 4;     // (tile, channel block) pairs of a wave: one v16i accumulator each, live across the K loop
constexpr int CP_LDS_LIMIT = 48 * 1024;  // offset table + patch: three workgroups per CU's 160 KiB (argued, as in stem_kxk.h)
constexpr int CP_PAIRS_PER_TILE_STEP = 2048;  // pairs of the whole layer per tile a wave holds: ~512 workgroups before a wave takes a second tile

struct CpGeom {
    int32_t flat;        // 1: pointwise, stride 1, no padding -- the tiles are runs of 32 consecutive pixels of the [N H W] order
    int32_t cp;          // bytes of a staged pixel that fragments read: in_c rounded up to 16
    int32_t pp;          // bytes between staged pixels: cp, plus 16 where cp / 16 is even (an ODD number of 16-byte slots)
    int32_t cpc;         // 16-byte chunks per tap: cp / 16
    int32_t nchunk;      // Kh Kw cpc
    int32_t nsteps;      // K steps of 32 bytes: ceil(nchunk / 2); an odd chunk count ends in a half step of zero weights
    int32_t nblk;        // blocks of 32 output channels: ceil(Cout / 32); the weights are zero beyond Cout
    int32_t ncb;         // channel blocks of a workgroup: 1 or 2 (grid.x = ceil(nblk / ncb))
    int32_t btx, bty;    // pixel tiles per workgroup: 8 x 4 outputs each in x / y (flat: btx runs of 32 pixels, bty = 1)
    int32_t tiles_x, tiles_y;  // workgroup rectangles per image in x / y (flat: tiles_x over the whole batch, tiles_y = 1)
    int32_t pw, ph;      // staged pixels per patch row, patch rows (flat: 32 btx, 1)
    int32_t pitch;       // bytes between patch rows: pw pp, plus 16 where that is an even number of 16-byte slots
    int32_t tab_bytes;   // the chunk offset table in front of the patch: 2 nsteps + 2 dwords rounded up to 16 bytes (flat: 0)
    int32_t nitems;      // dwords staged: ph pw cp / 4
    uint32_t dq_magic;   // j / (cp / 4) == umulhi(j, dq_magic) for j < 2^16
    uint32_t pw_magic;   // j / pw == umulhi(j, pw_magic) for j < 2^16
};

// int8, group 1, symmetric weights and the fast epilogue are the caller's; this is the shape class
static inline bool cp_scope(int C, int Kh, int Kw, int sh, int sw, int dh, int dw, int in_zp)
{
    if (C < CP_MIN_C || C % 16 == 0 || Kh < 1 || Kw < 1 || Kh > CP_MAX_K || Kw > CP_MAX_K) return false;
    if (sh < 1 || sw < 1 || sh > CP_MAX_STRIDE || sw > CP_MAX_STRIDE || dh != 1 || dw != 1) return false;
    return in_zp >= -128 && in_zp <= 127;
}

static inline void cp_patch(CpGeom &g, int Kh, int Kw, int sh, int sw)
{
    g.pw = g.flat ? 32 * g.btx : (g.btx * 8 - 1) * sw + Kw;
    g.ph = g.flat ? 1 : (g.bty * 4 - 1) * sh + Kh;
    g.pitch = g.pw * g.pp;
    if (!((g.pitch >> 4) & 1)) g.pitch += 16;
    g.nitems = g.ph * g.pw * (g.cp / 4);
}

static inline int64_t cp_lds_bytes(const CpGeom &g) { return (int64_t)g.tab_bytes + (int64_t)g.ph * g.pitch; }
static inline int64_t cp_weight_bytes(const CpGeom &g) { return (int64_t)g.nblk * g.nsteps * 1024; }

// byte offset of chunk q of a pixel's receptive field from the pixel's first tap (the kernel's table; flat: 16 q)
static inline int32_t cp_chunk_offset(const CpGeom &g, int Kw, int q)
{
    const int tap = q / g.cpc, c = q - tap * g.cpc, ky = tap / Kw, kx = tap - ky * Kw;
    return ky * g.pitch + kx * g.pp + 16 * c;
}

// The furthest LDS byte (exclusive) a B fragment read touches: the last pixel of the last tile, the last chunk (the half step
// behind an odd chunk count re-reads the last chunk: its weights are zero).
static inline int64_t cp_furthest_read(const CpGeom &g, int Kw, int sh, int sw)
{
    if (g.flat) return (int64_t)(32 * g.btx - 1) * g.pp + 16 * (g.nchunk - 1) + 16;
    return g.tab_bytes + (int64_t)(g.bty * 4 - 1) * sh * g.pitch + (int64_t)(g.btx * 8 - 1) * sw * g.pp + cp_chunk_offset(g, Kw, g.nchunk - 1) + 16;
}

static inline uint32_t cp_magic(int d) { return (uint32_t)((((uint64_t)1 << 32) / (uint32_t)d) + 1); }  // exact for j < 2^16, d < 2^16

// false: outside the kernel's scope, its LDS budget or its grid limits (the layer stays on the direct kernel)
static inline bool cp_geometry(int C, int Co, int Kh, int Kw, int sh, int sw, int pt, int pl, int H, int W, int Ho, int Wo, int N, CpGeom &g)
{
    if (!cp_scope(C, Kh, Kw, sh, sw, 1, 1, 0) || Co < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || N < 1) return false;
    const int64_t M = (int64_t)N * Ho * Wo;
    if (M >= ((int64_t)1 << 31) || (int64_t)N * H * W * C >= ((int64_t)1 << 31)) return false;
    g.flat = Kh == 1 && Kw == 1 && sh == 1 && sw == 1 && pt == 0 && pl == 0 && Ho == H && Wo == W;
    g.cp = (C + 15) / 16 * 16;
    g.cpc = g.cp / 16;
    // an odd number of 16-byte slots between pixels: the lanes of a fragment read (one pixel each, 16 bytes) then fall on
    // different slots of the LDS's 256-byte bank line at stride 1 -- reasoning, not a counter (conv_igemm_cpad.hip)
    g.pp = (g.cpc & 1) ? g.cp : g.cp + 16;
    g.nchunk = Kh * Kw * g.cpc;
    g.nsteps = (g.nchunk + 1) / 2;
    g.nblk = (Co + 31) / 32;
    g.ncb = g.nblk > 1 ? 2 : 1;
    g.tab_bytes = g.flat ? 0 : ((2 * g.nsteps + 2) * 4 + 15) / 16 * 16;
    const int tx_all = (Wo + 7) / 8, ty_all = (Ho + 3) / 4;
    const int64_t tiles_all = g.flat ? (M + 31) / 32 : (int64_t)N * tx_all * ty_all;
    // tiles per wave: one while the layer is small (more workgroups), up to four when it is large (fewer weight fetches per pixel)
    int64_t nt = tiles_all * g.nblk / CP_PAIRS_PER_TILE_STEP;
    nt = nt < 1 ? 1 : nt > CP_PAIRS_PER_WAVE ? CP_PAIRS_PER_WAVE : nt;
    const int cap = 4 * (int)nt / g.ncb;
    if (g.flat) {
        g.bty = 1;
        g.btx = tiles_all < cap ? (int)tiles_all : cap;
        for (cp_patch(g, Kh, Kw, sh, sw); g.btx > 1 && cp_lds_bytes(g) > CP_LDS_LIMIT; cp_patch(g, Kh, Kw, sh, sw)) --g.btx;
        if (cp_lds_bytes(g) > CP_LDS_LIMIT) return false;
        const int64_t rects = (tiles_all + g.btx - 1) / g.btx;
        if (rects > 65535) return false;
        g.tiles_x = (int32_t)rects, g.tiles_y = 1;
    } else {
        // of all rectangles: the most tiles whose patch fits LDS, then the smallest patch (the least halo), as in stem_kxk.h
        int best_x = 0, best_y = 0;
        int64_t best_bytes = 0;
        for (int bx = 1; bx <= cap && bx <= tx_all; ++bx) {
            g.btx = bx, g.bty = cap / bx < ty_all ? cap / bx : ty_all;
            for (cp_patch(g, Kh, Kw, sh, sw); g.bty > 1 && cp_lds_bytes(g) > CP_LDS_LIMIT; cp_patch(g, Kh, Kw, sh, sw)) --g.bty;
            if (cp_lds_bytes(g) > CP_LDS_LIMIT) continue;
            const int n = bx * g.bty, best_n = best_x * best_y;
            if (n > best_n || (n == best_n && cp_lds_bytes(g) < best_bytes)) best_x = bx, best_y = g.bty, best_bytes = cp_lds_bytes(g);
        }
        if (!best_x) return false;
        g.btx = best_x, g.bty = best_y;
        cp_patch(g, Kh, Kw, sh, sw);
        g.tiles_x = (tx_all + g.btx - 1) / g.btx;
        g.tiles_y = (ty_all + g.bty - 1) / g.bty;
        if (g.tiles_x > 65535 || (int64_t)g.tiles_y * N > 65535) return false;
    }
    g.dq_magic = cp_magic(g.cp / 4);
    g.pw_magic = cp_magic(g.pw);
    return g.nitems < (1 << 16) && (g.nblk + g.ncb - 1) / g.ncb <= 65535 && cp_weight_bytes(g) < ((int64_t)1 << 31);
}

// The plan-time packing: OHWI weights [Cout][Kh][Kw][C] -> MFMA A fragments [block of 32 channels][step][lane][16 B], lane =
// (matrix row = output channel of the block, 16-byte half of the step): chunk q = 2 step + half is tap q / cpc, channels
// 16 (q % cpc) .. + 15 -- zero where the channel is >= C (the padding of a pixel), where q >= nchunk (the half step behind an odd
// chunk count) and for channels beyond Cout.  The inverse map is tests/test_cpad_cpu.py's.
// acc_init[oc] = -zp_in sum(w[oc]) over all taps and the real channels: the patch holds zp_in where the image ends.
static inline void cp_pack(const int8_t *ohwi, int C, int Co, int Kh, int Kw, int in_zp, const CpGeom &g, int8_t *dst, int32_t *acc_init)
{
    const int taps = Kh * Kw;
    for (int b = 0; b < g.nblk; ++b)
        for (int s = 0; s < g.nsteps; ++s)
            for (int lane = 0; lane < 64; ++lane, dst += 16) {
                const int oc = b * 32 + (lane & 31), q = 2 * s + (lane >> 5), tap = q / g.cpc, c0 = 16 * (q - tap * g.cpc);
                for (int k = 0; k < 16; ++k)
                    dst[k] = (oc < Co && q < g.nchunk && c0 + k < C) ? ohwi[((int64_t)oc * taps + tap) * C + c0 + k] : (int8_t)0;
            }
    for (int oc = 0; oc < Co; ++oc) {
        int64_t sum = 0;
        for (int64_t k = 0; k < (int64_t)taps * C; ++k) sum += ohwi[(int64_t)oc * taps * C + k];
        acc_init[oc] = (int32_t)(-(int64_t)in_zp * sum);
    }
}

// The layers the kernel takes when SHL_MI355X_CPAD is unset: the classes where its median was MEASURED below the direct kernel's
// by more than the two sides' run-to-run spreads together (0 - 2 %), an NCHW layer's two re-layout launches in its time
// (tools/cpad_bench.py, profiles/cpad_notes.md).  Class = (kernel, stride, layout); new / direct at batch 1 .. batch 32:
//   1x1 s1 NHWC  24->144 @56 0.65 .. 0.12   72->24 @56 0.77 .. 0.10   72->40 @28 0.83 .. 0.15   40->120 @28 0.86 .. 0.14
//                120->40 @28 0.70 .. 0.10   200->80 @14 0.61 .. 0.13  184->80 @14 0.62 .. 0.14  58->58 @28 0.97 .. 0.19
//                116->116 @14 0.72 .. 0.13  232->232 @7 0.44 .. 0.11  -- every shape measured wins: on for any M
//   3x3 s1 NHWC  24->24 @56 0.36 .. 0.04    40->40 @28 0.36 .. 0.04   -- on for any M
//   1x1 s1 NCHW  three launches.  By the bytes the two re-layouts move, B = M (C + Cout): wins at B = 526 848 (24->144 @56 batch 1,
//                0.81), 727 552 (58->58 batch 8, 0.84) and above (.. 0.12); 1.00 at 301 056 (72->24 @56 batch 1) and 1.39 at 90 944
//                (58->58 @28 batch 1): on for B >= 526 848, the smallest B measured to win
//   3x3 s1 NCHW  24->24 @56: 0.41 at batch 1 (B = 150 528) .. 0.05: on for B >= 150 528
// No upper bound: in every class the ratio only falls with the batch, and nothing in either kernel changes beyond batch 32 (more
// workgroups of the same work) -- an extrapolation, as are other channel counts in a class (the direct kernel's time grows with
// C Cout per pixel, this kernel's with ceil(C / 16) ceil(Cout / 32)).  Every other kernel size and stride in scope was not
// measured and stays on the direct kernel.
static inline bool cp_default(int64_t M, int C, int Co, int Kh, int Kw, int sh, int sw, bool nchw)
{
    if (M <= 0 || Kh != Kw || (Kh != 1 && Kh != 3) || sh != 1 || sw != 1) return false;
    if (!nchw) return true;
    return M * (C + Co) >= (Kh == 1 ? 526848 : 150528);
}

}  // namespace shl

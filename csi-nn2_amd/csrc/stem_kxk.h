// stem_kxk.h -- the host half of conv_stem_kxk.hip (Kh x Kw convolutions with 1..4 input channels on the matrix cores): which
// layers the kernel takes, how the output map is cut into workgroup rectangles, the LDS patch of a rectangle, the plan-time
// weight packing and the default rule.  Pure host code that includes no HIP header, so that a stand-alone program can compile
// it with the sanitizers (tests/test_stem_kxk_cpu.py).
#pragma once
#include <stdint.h>
#include <string.h>

namespace shl {

constexpr int SK_MAX_K = 16;             // taps per axis
constexpr int SK_MAX_ROW_BYTES = 64;     // Kw in_c: one filter row is one or two K steps of 32 bytes
constexpr int SK_MAX_STRIDE = 16;
constexpr int SK_PAIRS_PER_WAVE = 4;     // (tile, channel block) pairs of a wave: one v16i accumulator each, live across the K loop
constexpr int SK_LDS_LIMIT = 48 * 1024;  // the patch with its tail: three workgroups per CU's 160 KiB
constexpr int SK_TAIL = 48;              // bytes behind the last patch row: a fragment read goes at most 35 past it (sk_furthest_read)

struct SkGeom {
    int32_t nblk;        // blocks of 32 output channels: ceil(Cout / 32); the weights are zero beyond Cout
    int32_t ncb;         // channel blocks of a workgroup: 1 or 2 (grid.x = ceil(nblk / ncb))
    int32_t spr;         // K steps per filter row: 1 (Kw in_c <= 32) or 2
    int32_t kh;          // filter rows: the K loop is kh x spr steps
    int32_t btx, bty;    // MFMA pixel tiles (8 wide x 4 high) per workgroup in x / y
    int32_t tiles_x, tiles_y;
    int32_t row_bytes;   // input bytes of a patch row: ((8 btx - 1) sw + Kw) in_c
    int32_t ph;          // patch rows: (4 bty - 1) sh + Kh
    int32_t pitch;       // bytes between patch rows: row_bytes rounded up to an ODD number of dwords
    int32_t ndw;         // dwords staged: ph pitch / 4
    uint32_t rdw_magic;  // j / (pitch / 4) == umulhi(j, rdw_magic) for j < 2^16
};

// int8, group 1 are the caller's; this is the shape class.  3x3 is excluded outright: with three NHWC channels it is the
// register-built stem kernel's (conv_stem.hip), and the fused stem + depthwise pairs expect every other 3x3 stem where it is today.
static inline bool sk_scope(int C, int Kh, int Kw, int sh, int sw, int dh, int dw, int in_zp)
{
    if (C < 1 || C > 4 || Kh < 1 || Kw < 1 || Kh > SK_MAX_K || Kw > SK_MAX_K || Kw * C > SK_MAX_ROW_BYTES) return false;
    if (sh < 1 || sw < 1 || sh > SK_MAX_STRIDE || sw > SK_MAX_STRIDE || dh != 1 || dw != 1) return false;
    if (Kh == 3 && Kw == 3) return false;
    return in_zp >= -128 && in_zp <= 127;
}

static inline void sk_patch(SkGeom &g, int C, int Kh, int Kw, int sh, int sw)
{
    g.row_bytes = ((g.btx * 8 - 1) * sw + Kw) * C;
    g.ph = (g.bty * 4 - 1) * sh + Kh;
    // an odd number of dwords: the four rows of a pixel tile (sh pitch apart) start in different banks (reasoning, not a counter)
    g.pitch = (((g.row_bytes + 3) / 4) | 1) * 4;
    g.ndw = g.ph * (g.pitch / 4);
}

static inline int64_t sk_lds_bytes(const SkGeom &g) { return (int64_t)g.ph * g.pitch + SK_TAIL; }
static inline int64_t sk_weight_bytes(const SkGeom &g) { return (int64_t)g.nblk * g.kh * g.spr * 1024; }

// The furthest LDS byte (exclusive) a B fragment read touches: the last pixel of the last tile, the last filter row, the last
// step's upper half -- 16 bytes at an arbitrary address are fetched as the five aligned dwords that cover them.
static inline int64_t sk_furthest_read(const SkGeom &g, int C, int sh, int sw)
{
    const int64_t a = (int64_t)((g.bty * 4 - 1) * sh + g.kh - 1) * g.pitch + (int64_t)(g.btx * 8 - 1) * sw * C + 32 * (g.spr - 1) + 16;
    return (a & ~(int64_t)3) + 20;
}

// false: outside the kernel's scope or its grid limits (the layer stays on the direct kernel)
static inline bool sk_geometry(int C, int Co, int Kh, int Kw, int sh, int sw, int Ho, int Wo, int N, SkGeom &g)
{
    if (!sk_scope(C, Kh, Kw, sh, sw, 1, 1, 0) || Co < 1 || Ho < 1 || Wo < 1 || N < 1) return false;
    g.nblk = (Co + 31) / 32;
    g.ncb = g.nblk > 1 ? 2 : 1;
    g.spr = Kw * C > 32 ? 2 : 1;
    g.kh = Kh;
    const int tx_all = (Wo + 7) / 8, ty_all = (Ho + 3) / 4;
    // four waves x four pairs = 16 / ncb tiles at most.  Of all rectangles: the most tiles whose patch fits LDS, then the
    // smallest patch (the squarest in input pixels: the least halo).  A single tile always fits: 16 x 16 at stride 16 with four
    // channels is 64 rows of 512 bytes.
    const int cap = 4 * SK_PAIRS_PER_WAVE / g.ncb;
    int best_x = 0, best_y = 0;
    int64_t best_bytes = 0;
    for (int bx = 1; bx <= cap && bx <= tx_all; ++bx) {
        g.btx = bx, g.bty = cap / bx < ty_all ? cap / bx : ty_all;
        for (sk_patch(g, C, Kh, Kw, sh, sw); g.bty > 1 && sk_lds_bytes(g) > SK_LDS_LIMIT; sk_patch(g, C, Kh, Kw, sh, sw)) --g.bty;
        if (sk_lds_bytes(g) > SK_LDS_LIMIT) continue;
        const int n = bx * g.bty, best_n = best_x * best_y;
        if (n > best_n || (n == best_n && sk_lds_bytes(g) < best_bytes)) best_x = bx, best_y = g.bty, best_bytes = sk_lds_bytes(g);
    }
    if (!best_x) return false;
    g.btx = best_x, g.bty = best_y;
    sk_patch(g, C, Kh, Kw, sh, sw);
    g.tiles_x = (tx_all + g.btx - 1) / g.btx;
    g.tiles_y = (ty_all + g.bty - 1) / g.bty;
    g.rdw_magic = (uint32_t)((((uint64_t)1 << 32) / (uint32_t)(g.pitch / 4)) + 1);  // exact for j < 2^16 (pitch / 4 >= 3, ndw < 2^14)
    return g.tiles_x <= 65535 && (int64_t)g.tiles_y * N <= 65535 && sk_weight_bytes(g) < ((int64_t)1 << 31);
}

// The plan-time packing: OHWI weights [Cout][Kh][Kw][C] -> MFMA A fragments [block of 32 channels][ky][step][lane][16 B], lane =
// (matrix row = output channel of the block, 16-byte half of the step's 32 K bytes): bytes 32 step + 16 half .. + 15 of the
// channel's filter row ky, which is Kw C bytes long -- zero behind it, and zero for channels beyond Cout.
// acc_init[oc] = -zp_in sum(w[oc]): the patch holds zp_in where the image ends.
static inline void sk_pack(const int8_t *ohwi, int C, int Co, int Kh, int Kw, int in_zp, const SkGeom &g, int8_t *dst, int32_t *acc_init)
{
    const int rb = Kw * C;
    for (int b = 0; b < g.nblk; ++b)
        for (int ky = 0; ky < Kh; ++ky)
            for (int s = 0; s < g.spr; ++s)
                for (int lane = 0; lane < 64; ++lane, dst += 16) {
                    const int oc = b * 32 + (lane & 31), k0 = 32 * s + 16 * (lane >> 5);
                    for (int k = 0; k < 16; ++k)
                        dst[k] = (oc < Co && k0 + k < rb) ? ohwi[((int64_t)oc * Kh + ky) * rb + k0 + k] : (int8_t)0;
                }
    for (int oc = 0; oc < Co; ++oc) {
        int64_t sum = 0;
        for (int64_t k = 0; k < (int64_t)Kh * rb; ++k) sum += ohwi[(int64_t)oc * Kh * rb + k];
        acc_init[oc] = (int32_t)(-(int64_t)in_zp * sum);
    }
}

// The layers the kernel takes when SHL_MI355X_STEMKXK is unset: the classes where it was MEASURED faster than the direct kernel
// by more than the larger of the two run-to-run spreads (0 - 1 %), an NCHW layer's two re-layout launches in its time
// (tools/stem_kxk_bench.py, profiles/stem_kxk_notes.md).  Class = (input channels, kernel, stride, layout) of the four stems
// measured; the class variable is E = M Cout output bytes, M = N Ho Wo, as in group_mfma.h.  new / direct at the smallest E
// measured (batch 1) .. at the largest (batch 32):
//   7x7 s2, 3 ch (ResNet, 3 -> 64 @224)     NHWC  E >=   802 816   0.10 .. 0.01      NCHW  E >=   802 816   0.16 .. 0.02
//   4x4 s4, 3 ch (ConvNeXt, 3 -> 96 @224)   NHWC  E >=   301 056   0.60 .. 0.05      NCHW  E >=   301 056   0.86 .. 0.15
//   16x16 s16, 3 ch (ViT, 3 -> 768 @224)    NHWC  E >=   150 528   0.03 .. 0.01      NCHW  E >=   150 528   0.13 .. 0.03
//   5x5 s2, 1 ch (3 -> 32 @128)             NHWC  E >=   131 072   0.93 .. 0.10      NCHW  E >= 1 048 576   0.46 .. 0.21
//                                                                                   [131 072, batch 1: 1.35 -- out: three launches]
// No upper bound on E: in every class the ratio only falls with E up to batch 32, and nothing in either kernel changes beyond it
// (more workgroups of the same work) -- an extrapolation, as is another Cout at the same E.  Every other kernel size, stride and
// channel count in scope was not measured and stays on the direct kernel.
static inline bool sk_default(int64_t M, int C, int Co, int Kh, int Kw, int sh, int sw, bool nchw)
{
    static const struct { int c, k, s; int64_t min_e[2]; } rule[] = {
        {3, 7, 2, {802816, 802816}}, {3, 4, 4, {301056, 301056}}, {3, 16, 16, {150528, 150528}}, {1, 5, 2, {131072, 1048576}}};
    if (M <= 0 || Kh != Kw || sh != sw) return false;
    for (const auto &r : rule)
        if (C == r.c && Kh == r.k && sh == r.s) return M * Co >= r.min_e[nchw ? 1 : 0];
    return false;
}

}  // namespace shl

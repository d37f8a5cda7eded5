// group_mfma.h -- the host half of conv_group_mfma.hip (grouped int8 convolution on the matrix cores): which layers the kernel
// takes, how a layer is cut into units and an output map into workgroup rectangles, the LDS patch of a rectangle, the plan-time
// weight packing and the default rule.  Pure host code that includes no HIP header, so that a stand-alone program can compile
// it with the sanitizers (tests/test_group_mfma_cpu.py).
#pragma once
#include <stdint.h>
#include <string.h>

namespace shl {

constexpr int GM_MAX_K = 7;             // taps per axis
constexpr int GM_TILES_PER_WAVE = 4;    // one v16i accumulator each, live across the slab and tap loops
constexpr int GM_PIX_BYTES = 48;        // a patch pixel in LDS: 32 channel bytes of the slab + 16 bytes of padding
constexpr int GM_STAGE = 5;             // 16-byte pieces of the patch a thread moves HBM -> LDS: bounds the patch at 640 pixels
constexpr int GM_PREFETCH = 3;          // ... and where the NEXT K slab's pieces wait in registers under the MFMAs: 384 pixels
constexpr int GM_LDS_LIMIT = 40 * 1024; // four workgroups per CU's 160 KiB (argued, not measured against other targets)

struct GmGeom {
    int32_t nunits;      // grid.x: a unit = nblk blocks of 32 output channels over ONE window of kc input channels
    int32_t nblk;        // 1, 2 or 4: unit u is output channels 32 nblk u .. +32 nblk - 1
    int32_t upg;         // consecutive units that share a window: unit u reads input channels (u / upg) kc .. + kc - 1
    int32_t kc, nslab;   // window width (a multiple of 32) and its 32-channel K slabs
    int32_t btx, bty;    // MFMA pixel tiles (8 wide x 4 high) per workgroup in x / y
    int32_t tiles_x, tiles_y;
    int32_t pw, ph;      // patch size in input pixels
    int32_t row_pitch;   // bytes between patch rows (>= pw GM_PIX_BYTES, see gm_row_pitch)
    int32_t nslots;      // 16-byte pieces of the patch: 2 pw ph
    int32_t ntaps, kw;   // Kh Kw and Kw (the tap loop's inner extent)
    uint32_t pw_magic;   // j / pw == umulhi(j, pw_magic) for j < 2^16
};

// The bank argument (reasoning, not measurement: profiles/group_mfma_notes.md).  A ds_read_b128 of a wave takes lane & 31 = a
// pixel of the 8 x 4 tile, lane >> 5 = the 16-byte half.  With 48-byte pixels consecutive pixels of a tile row are 3 (stride 2:
// 6) sixteen-byte bank groups apart, so the eight pixels of a row fall on eight different ones of the sixteen groups; the next
// tile row must fall on the other eight: (sh row_pitch / 16) % 16 == 8 at stride 1 in x, an odd row pitch (in 16-byte units) at
// stride 2 in x and 1 in y.  Stride 2 on both axes has no such pitch (two-way at best).
static inline int gm_row_pitch(int pw, int sh, int sw)
{
    int rp = pw * (GM_PIX_BYTES / 16);
    if (sw == 1)
        while ((sh * rp) % 16 != 8) ++rp;
    else if (sh == 1)
        rp |= 1;
    return rp * 16;
}

static inline void gm_patch(GmGeom &g, int Kh, int Kw, int sh, int sw)
{
    g.pw = (g.btx * 8 - 1) * sw + Kw;
    g.ph = (g.bty * 4 - 1) * sh + Kh;
    g.row_pitch = gm_row_pitch(g.pw, sh, sw);
    g.nslots = 2 * g.pw * g.ph;
}

static inline int64_t gm_lds_bytes(const GmGeom &g) { return (int64_t)g.ph * g.row_pitch; }
static inline int64_t gm_weight_bytes(const GmGeom &g) { return (int64_t)g.nunits * g.nblk * g.nslab * g.ntaps * 1024; }

// The units of a layer.  Narrow groups (C/G == Cout/G in {4, 8, 16}): unit u = output channels 32 u .. over input channels 32 u ..,
// 8 / 4 / 2 groups on the diagonal of its 32 x 32 weight matrix.  Wide groups (C/G and Cout/G multiples of 32): up to four of a
// group's output blocks over the group's own channels.  false: not a layer of this kernel.
static inline bool gm_units(int C, int Co, int G, GmGeom &g)
{
    if (G < 2 || C < 32 || Co < 32 || C % 32 || Co % 32 || C % G || Co % G) return false;
    const int cpg = C / G, opg = Co / G;
    if (cpg == opg && (cpg == 4 || cpg == 8 || cpg == 16)) {
        g.nblk = 1, g.upg = 1, g.kc = 32;
    } else if (cpg % 32 == 0 && opg % 32 == 0) {
        const int nb = opg / 32;
        g.nblk = nb % 4 == 0 ? 4 : (nb % 2 == 0 ? 2 : 1);
        g.upg = nb / g.nblk, g.kc = cpg;
    } else {
        return false;
    }
    g.nslab = g.kc / 32;
    g.nunits = Co / (32 * g.nblk);
    return true;
}

// false: outside the kernel's scope or its grid limits (the layer stays on the direct kernel)
static inline bool gm_geometry(int C, int Co, int G, int Kh, int Kw, int sh, int sw, int Ho, int Wo, int N, GmGeom &g)
{
    if (!gm_units(C, Co, G, g)) return false;
    if (Kh < 1 || Kw < 1 || Kh > GM_MAX_K || Kw > GM_MAX_K || sh < 1 || sh > 2 || sw < 1 || sw > 2 || Ho < 1 || Wo < 1 || N < 1) return false;
    g.ntaps = Kh * Kw, g.kw = Kw;
    const int tx_all = (Wo + 7) / 8, ty_all = (Ho + 3) / 4;
    // a wave owns one block and at most four tiles: 4 / nblk waves share a block's tiles.  Of the rectangles one or two tiles
    // wide, the one with the most tiles whose patch fits the prefetch registers and the LDS target (a single tile always does:
    // 7x7 at stride 2 is 21 x 13 pixels)
    const int cap = GM_TILES_PER_WAVE * (4 / g.nblk);
    const int max_slots = (g.nslab > 1 ? GM_PREFETCH : GM_STAGE) * 256;
    int best_x = 0, best_y = 0;
    for (int bx = 2; bx >= 1; --bx) {
        if (bx > tx_all) continue;
        g.btx = bx, g.bty = cap / bx < ty_all ? cap / bx : ty_all;
        for (gm_patch(g, Kh, Kw, sh, sw); g.bty > 1 && (g.nslots > max_slots || gm_lds_bytes(g) > GM_LDS_LIMIT); gm_patch(g, Kh, Kw, sh, sw)) --g.bty;
        if (g.nslots > max_slots || gm_lds_bytes(g) > GM_LDS_LIMIT) continue;
        if (bx * g.bty > best_x * best_y) best_x = bx, best_y = g.bty;
    }
    if (!best_x) return false;
    g.btx = best_x, g.bty = best_y;
    gm_patch(g, Kh, Kw, sh, sw);
    g.tiles_x = (tx_all + g.btx - 1) / g.btx;
    g.tiles_y = (ty_all + g.bty - 1) / g.bty;
    g.pw_magic = (uint32_t)((((uint64_t)1 << 32) / (uint32_t)g.pw) + 1);  // exact for j < 2^16 (pw < 2^6)
    return g.tiles_x <= 65535 && (int64_t)g.tiles_y * N <= 65535 && gm_weight_bytes(g) < ((int64_t)1 << 31);
}

// The plan-time packing: OIHW weights [Cout][C/G][Kh][Kw] -> MFMA A fragments [unit][block][K slab][tap][lane][16 B], lane =
// (matrix row = output channel of the block, 16-byte half of the slab's 32 input channels).  A byte whose input channel lies
// outside the output channel's group is zero -- this is everything the kernel ever learns about groups.
// acc_init[oc] = -zp_in sum(w[oc]): the patch holds zp_in where the image ends.
static inline void gm_pack(const int8_t *oihw, int C, int Co, int G, int Kh, int Kw, int in_zp, const GmGeom &g, int8_t *dst, int32_t *acc_init)
{
    const int cpg = C / G, opg = Co / G, taps = Kh * Kw;
    for (int u = 0; u < g.nunits; ++u)
        for (int b = 0; b < g.nblk; ++b)
            for (int s = 0; s < g.nslab; ++s)
                for (int tap = 0; tap < taps; ++tap)
                    for (int lane = 0; lane < 64; ++lane, dst += 16) {
                        const int oc = (u * g.nblk + b) * 32 + (lane & 31);
                        const int c_first = (u / g.upg) * g.kc + s * 32 + (lane >> 5) * 16;  // input channel of byte 0
                        const int grp = oc / opg;
                        for (int k = 0; k < 16; ++k) {
                            const int ic = c_first + k - grp * cpg;  // inside the group
                            dst[k] = (ic >= 0 && ic < cpg) ? oihw[((int64_t)oc * cpg + ic) * taps + tap] : (int8_t)0;
                        }
                    }
    for (int oc = 0; oc < Co; ++oc) {
        int64_t sum = 0;
        for (int64_t k = 0; k < (int64_t)cpg * taps; ++k) sum += oihw[(int64_t)oc * cpg * taps + k];
        acc_init[oc] = (int32_t)(-(int64_t)in_zp * sum);
    }
}

// The layers the kernel takes when SHL_MI355X_GROUPMFMA is unset: the classes where it was MEASURED faster than the direct
// kernel by more than the larger of the two run-to-run spreads, the two re-layout launches in its time (tools/group_bench.py,
// profiles/group_mfma_notes.md; spreads 0 - 1 %).  Class = (channels per group, strided or not), 3x3 kernels with
// C/G == Cout/G only; the class variable is E = M Cout output bytes, M = N Ho Wo.  The new kernel's three launches cost
// 10 - 14 us whatever the size, the direct kernel's time grows with E and with its serial loop of 9 C/G products per output, so
// each class has a smallest E from which it wins; new / direct at that E, and at the largest E measured:
//   C/G   stride 1: E >=, ratio there .. at batch 32        stride 2: E >=, ratio there .. at batch 32
//    4    401 408  (128 @56 b1)   0.92 .. 0.12               3 211 264 (128 @56 b32)  0.33     [100 352, b1: 1.38 -- out]
//    8    200 704  (256 @28 b1)   0.85 .. 0.11               1 605 632 (256 @28 b32)  0.30     [ 50 176, b1: 1.15 -- out]
//   16    100 352  (512 @14 b1; RegNetX-800MF 128 @28) 0.74 / 0.77 .. 0.09      25 088 (512 @14 b1)  0.65 .. 0.19
//   32     50 176  (1024 @7 b1)   0.38 .. 0.06                  16 384 (1024 @7 b1)   0.36 .. 0.13
//   64    100 352  (ResNeXt-101 32x8d 2048 @7 b1) 0.21 .. 0.02  100 352 (2048 @14 b1) 0.20 .. 0.02
// No upper bound on E: in every class the ratio only falls with E up to the largest size measured (batch 32), and nothing in
// either kernel changes beyond it (more workgroups of the same work) -- an extrapolation, and said so in the notes.  Other
// kernel sizes, other group widths (96, 128, ...) and C/G != Cout/G were not measured and stay on the direct kernel, as does
// everything below the thresholds: N=3, 9x7, C=128, G=32 (E = 24 192, which tests/test_group_conv.py pins to the direct
// kernel's name) lies under the smallest size of its class that was measured at all, and that one lost.
static inline bool gm_default(int64_t M, int C, int Co, int G, int taps, bool strided)
{
    if (M <= 0 || C != Co || G < 1 || C % G || taps != 9) return false;
    static const struct { int cpg; int64_t min_e[2]; } rule[] = {
        {4, {401408, 3211264}}, {8, {200704, 1605632}}, {16, {100352, 25088}}, {32, {50176, 16384}}, {64, {100352, 100352}}};
    for (const auto &r : rule)
        if (C / G == r.cpg) return M * Co >= r.min_e[strided ? 1 : 0];
    return false;
}

}  // namespace shl

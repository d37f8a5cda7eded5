// group_mfma_f16.h -- the host half of conv_group_mfma_f16.hip (grouped binary16 convolution on the matrix cores): which layers
// the kernel takes, how a layer is cut into blocks and units and an output map into workgroup rectangles, the LDS patch of a
// rectangle, the plan-time weight packing and the default rule.  Pure host code that includes no HIP header, so that a
// stand-alone program can compile it with the sanitizers (tests/test_group_mfma_f16_cpu.py).
#pragma once
#include <stdint.h>
#include <string.h>

namespace shl {

constexpr int GH_MAX_K = 7;              // taps per axis
constexpr int GH_TILES_PER_WAVE = 8;     // one 16 x 16 fp32 accumulator (four registers) each, live across the K loop
constexpr int GH_PIX_BYTES = 80;         // a patch pixel in LDS: 32 halves of the K window + 16 bytes of padding
constexpr int GH_STAGE = 10;             // 16-byte pieces of the patch a thread moves HBM -> LDS: bounds the patch at 640 pixels
constexpr int GH_PREFETCH = 6;           // ... and where the NEXT K slab's pieces wait in registers under the MFMAs: 384 pixels
constexpr int GH_LDS_LIMIT = 48 * 1024;  // patch + tap table: three workgroups per CU's 160 KiB (argued, not measured)
constexpr int GH_TAP_SLOTS = 64;         // the tap table: 49 taps rounded up to whole MFMAs of 8 taps

struct GhGeom {
    int32_t nunits;      // grid.x: a unit = nblk blocks over ONE window of kc input channels
    int32_t nblk;        // 2, 4 or 8 blocks per unit; a block = 16 matrix rows = output channels of ONE group
    int32_t upg;         // consecutive units that share a window: unit u reads input channels (u / upg) kc .. + kc - 1
    int32_t kc, nslab;   // window width (a multiple of 32) and its 32-channel K slabs
    int32_t cpg;         // narrow groups: C/G = Cout/G (4, 8 or 16), block b of a unit is group b of its window; 0: wide groups
    int32_t mvalid;      // rows of a block that are output channels (C/G of a narrow group, else 16); the others are padding
    int32_t tpm;         // taps per MFMA: 32 / cpg, 1 for wide groups (K = one slab of one tap)
    int32_t spslab;      // MFMA steps per slab: ceil(taps / tpm)
    int32_t bpw;         // blocks a wave runs one after the other (2 for 4-wide groups, else 1)
    int32_t btx, bty;    // MFMA pixel tiles (8 wide x 2 high) per workgroup in x / y
    int32_t tiles_x, tiles_y;
    int32_t pw, ph;      // patch size in input pixels
    int32_t row_pitch;   // bytes between patch rows (>= pw GH_PIX_BYTES, see gh_row_pitch)
    int32_t nslots;      // 16-byte pieces of the patch: 4 pw ph
    int32_t ntaps, kw;   // Kh Kw and Kw
    uint32_t pw_magic;   // j / pw == umulhi(j, pw_magic) for j < 2^16
};

// The bank argument (reasoning, NOT measured).  The sixteen lanes that share a K quarter of the B operand read the 8 x 2 pixels
// of a tile at one channel offset, 16 bytes each (ds_read_b128; two ds_read_b64 for 4-wide groups).  With 80-byte pixels
// consecutive pixels of a tile row are 5 (stride 2: 10) sixteen-byte bank groups apart, so the eight pixels of a row fall on
// eight different ones of the sixteen groups of a 64-bank LDS; the second tile row must fall on the other eight:
// (sh row_pitch / 16) % 16 == 8 at stride 1 in x, an odd row pitch (in 16-byte units) at stride 2 in x and 1 in y.  Stride 2 on
// both axes has no such pitch (two-way at best).  The four K quarters of a wave differ by channel offset or by tap, which this
// pitch does not separate.
static inline int gh_row_pitch(int pw, int sh, int sw)
{
    int rp = pw * (GH_PIX_BYTES / 16);
    if (sw == 1)
        while ((sh * rp) % 16 != 8) ++rp;
    else if (sh == 1)
        rp |= 1;
    return rp * 16;
}

static inline void gh_patch(GhGeom &g, int Kh, int Kw, int sh, int sw)
{
    g.pw = (g.btx * 8 - 1) * sw + Kw;
    g.ph = (g.bty * 2 - 1) * sh + Kh;
    g.row_pitch = gh_row_pitch(g.pw, sh, sw);
    g.nslots = 4 * g.pw * g.ph;
}

static inline int64_t gh_lds_bytes(const GhGeom &g) { return (int64_t)g.ph * g.row_pitch + GH_TAP_SLOTS * 4; }  // patch, tap table
static inline int64_t gh_nblocks(const GhGeom &g) { return (int64_t)g.nunits * g.nblk; }
static inline int64_t gh_weight_bytes(const GhGeom &g) { return gh_nblocks(g) * g.nslab * g.spslab * 1024; }

// The blocks and units of a layer.  A block is the M = 16 of one v_mfma_f32_16x16x32_f16 and never holds output channels of two
// groups, so no product of one group's input ever meets another group's weights -- not even a zero one: 0 x inf is NaN.
//   narrow groups (C/G == Cout/G in {4, 8, 16}): block = one group (rows past C/G are padding); unit u = the 8 / 4 / 2 groups
//     whose input channels are 32 u .. 32 u + 31;
//   wide groups (C/G and Cout/G multiples of 32): block = 16 of a group's output channels, unit = 4 (else 2) consecutive blocks
//     of one group over the group's own channels.
// false: not a layer of this kernel.
static inline bool gh_units(int C, int Co, int G, int taps, GhGeom &g)
{
    if (G < 2 || C < 32 || Co < 32 || C % 32 || Co % 32 || C % G || Co % G || taps < 1) return false;
    const int cpg = C / G, opg = Co / G;
    if (cpg == opg && (cpg == 4 || cpg == 8 || cpg == 16)) {
        g.cpg = cpg, g.mvalid = cpg, g.tpm = 32 / cpg;
        g.nblk = 32 / cpg, g.upg = 1, g.kc = 32;
        g.nunits = C / 32;
    } else if (cpg % 32 == 0 && opg % 32 == 0) {
        g.cpg = 0, g.mvalid = 16, g.tpm = 1;
        g.nblk = (opg / 16) % 4 == 0 ? 4 : 2;
        g.upg = opg / (16 * g.nblk), g.kc = cpg;
        g.nunits = Co / (16 * g.nblk);
    } else {
        return false;
    }
    g.bpw = g.nblk > 4 ? g.nblk / 4 : 1;
    g.nslab = g.kc / 32;
    g.spslab = (taps + g.tpm - 1) / g.tpm;
    return true;
}

// false: outside the kernel's scope or its grid limits (the layer stays on the direct kernel)
static inline bool gh_geometry(int C, int Co, int G, int Kh, int Kw, int sh, int sw, int Ho, int Wo, int N, GhGeom &g)
{
    if (Kh < 1 || Kw < 1 || Kh > GH_MAX_K || Kw > GH_MAX_K || sh < 1 || sh > 2 || sw < 1 || sw > 2 || Ho < 1 || Wo < 1 || N < 1) return false;
    if (!gh_units(C, Co, G, Kh * Kw, g)) return false;
    g.ntaps = Kh * Kw, g.kw = Kw;
    const int tx_all = (Wo + 7) / 8, ty_all = (Ho + 1) / 2;
    // a wave owns its block(s) and at most eight tiles: 4 / nblk waves share a block's tiles.  Of the rectangles one or two tiles
    // wide, the one with the most tiles whose patch fits the staging registers and the LDS target (a single tile always does:
    // 7x7 at stride 2 is 21 x 9 pixels)
    const int cap = GH_TILES_PER_WAVE * (g.nblk >= 4 ? 1 : 4 / g.nblk);
    const int max_slots = (g.nslab > 1 ? GH_PREFETCH : GH_STAGE) * 256;
    int best_x = 0, best_y = 0;
    for (int bx = 2; bx >= 1; --bx) {
        if (bx > tx_all) continue;
        g.btx = bx, g.bty = cap / bx < ty_all ? cap / bx : ty_all;
        for (gh_patch(g, Kh, Kw, sh, sw); g.bty > 1 && (g.nslots > max_slots || gh_lds_bytes(g) > GH_LDS_LIMIT); gh_patch(g, Kh, Kw, sh, sw)) --g.bty;
        if (g.nslots > max_slots || gh_lds_bytes(g) > GH_LDS_LIMIT) continue;
        if (bx * g.bty > best_x * best_y) best_x = bx, best_y = g.bty;
    }
    if (!best_x) return false;
    g.btx = best_x, g.bty = best_y;
    gh_patch(g, Kh, Kw, sh, sw);
    g.tiles_x = (tx_all + g.btx - 1) / g.btx;
    g.tiles_y = (ty_all + g.bty - 1) / g.bty;
    g.pw_magic = (uint32_t)((((uint64_t)1 << 32) / (uint32_t)g.pw) + 1);  // exact for j < 2^16 (pw < 2^6)
    return g.tiles_x <= 65535 && (int64_t)g.tiles_y * N <= 65535 && gh_weight_bytes(g) < ((int64_t)1 << 31);
}

// The plan-time packing: OIHW binary16 weights [Cout][C/G][Kh][Kw] -> MFMA A fragments [block][slab][step][lane][8 halves] in
// the order a wave consumes them; lane = (matrix row = lane & 15, K quarter = lane >> 4), K index k = 8 (lane >> 4) + e.
//   narrow groups: k = (tap of the step) cpg + input channel of the group, tap = step tpm + k / cpg
//   wide groups:   k = channel of the slab, the step is the tap
// Rows past the group's output channels and K positions past the last tap are +0 (the kernel zeroes the same K positions of B).
static inline void gh_pack(const uint16_t *oihw, int C, int Co, int G, int Kh, int Kw, const GhGeom &g, uint16_t *dst)
{
    const int cpg = C / G, opg = Co / G, taps = Kh * Kw;
    for (int64_t b = 0; b < gh_nblocks(g); ++b) {
        const int oc0 = g.cpg ? (int)b * opg : (int)b * 16;
        for (int s = 0; s < g.nslab; ++s)
            for (int j = 0; j < g.spslab; ++j)
                for (int lane = 0; lane < 64; ++lane, dst += 8) {
                    const int m = lane & 15;
                    for (int e = 0; e < 8; ++e) {
                        const int k = 8 * (lane >> 4) + e;
                        const int tap = g.cpg ? j * g.tpm + k / g.cpg : j;
                        const int ic = g.cpg ? k % g.cpg : s * 32 + k;
                        dst[e] = (m < g.mvalid && tap < taps) ? oihw[((int64_t)(oc0 + m) * cpg + ic) * taps + tap] : (uint16_t)0;
                    }
                }
    }
}

// The layers the kernel takes when SHL_MI355X_GROUPMFMA_F16 is unset: the classes where it was MEASURED faster than the direct
// kernel by more than the larger of the two run-to-run spreads (below 0.5 % everywhere), the two re-layout launches in its time
// (tools/group_bench.py --dtype f16, profiles/group_mfma_f16_notes.md).  Class = (channels per group, strided or not), 3x3
// kernels with C/G == Cout/G only; the class variable is E = M Cout outputs, M = N Ho Wo.  The three launches cost 14 - 26 us
// whatever the size, so each class has a smallest E from which the kernel wins.  Each class was measured at two sizes (batch 1
// and 32); the threshold is the smallest size that WON, so where batch 1 lost the class is on from its batch-32 size only and
// the sizes in between stay on the direct kernel, unmeasured.  new / direct at the threshold:
//   C/G   stride 1: E >=                  ratio     stride 2: E >=                  ratio
//    4    12 845 056 (128 @56 b32)        0.31      3 211 264 (128 @56 b32)         0.55      [b1: 2.27 / 3.41 -- out]
//    8     6 422 528 (256 @28 b32)        0.20      1 605 632 (256 @28 b32)         0.35      [b1: 1.57 / 1.89 -- out]
//   16     3 211 264 (512 @14, 128 @28 b32) 0.17      802 816 (512 @14 b32)         0.29      [b1: 1.28, 1.27 / 1.13 -- out]
//   32        50 176 (1024 @7 b1)         0.79         16 384 (1024 @7 b1)          0.61      b32: 0.15 / 0.18
//   64       100 352 (2048 @7 b1)         0.38        100 352 (2048 @14 b1)         0.33      b32: 0.07 / 0.04
// No upper bound on E (the ratio only falls with E in every class; beyond the largest size it is an extrapolation).  Other
// kernel sizes, other group widths and C/G != Cout/G were not measured and stay on the direct kernel.
static inline bool gh_default(int64_t M, int C, int Co, int G, int taps, bool strided)
{
    if (M <= 0 || C != Co || G < 1 || C % G || taps != 9) return false;
    static const struct { int cpg; int64_t min_e[2]; } rule[] = {
        {4, {12845056, 3211264}}, {8, {6422528, 1605632}}, {16, {3211264, 802816}}, {32, {50176, 16384}}, {64, {100352, 100352}}};
    for (const auto &r : rule)
        if (C / G == r.cpg) return M * Co >= r.min_e[strided ? 1 : 0];
    return false;
}

}  // namespace shl

// dw_nchw_kxk.h -- the host half of dwconv_kxk_nchw.hip (depthwise NCHW layers whose kernel is not 3x3, int8 and binary16, over an
// LDS patch per plane): which layers the kernel takes, how the planes are cut into workgroup rectangles, the LDS patch and its
// budget, the plan-time packing of the int8 filter rows and the default rule.  Pure host code that includes no HIP header, so
// that a stand-alone program can compile it with the sanitizers (tests/test_dw_nchw_kxk_cpu.py).
#pragma once
#include <stdint.h>
#include <string.h>

namespace shl {

constexpr int DN_MAX_K = 7;               // taps per axis: a filter row is two dwords of int8 weights
constexpr int DN_TX = 4;                  // consecutive outputs of one row per thread
constexpr int DN_THREADS = 256;
constexpr int DN_MAX_CG = 16;             // column groups of a rectangle: 64 output columns
constexpr int DN_LDS_LIMIT = 32 * 1024;   // patches + binary16 filters: five workgroups per CU's 160 KiB (argued, not measured)
constexpr int DN_WG_TARGET = 512;         // workgroups wanted before a workgroup takes more planes than fill one wave: two per CU
constexpr int DN_W_SLOT = 56;             // binary16: LDS dwords per owned plane's filter, widened to fp32 as [7 rows][8]

struct DnGeom {
    int32_t es;          // element bytes: 1 int8, 2 binary16
    int32_t cg;          // column groups (DN_TX outputs each) of a workgroup
    int32_t rw;          // output rows of a workgroup
    int32_t pl;          // planes of a workgroup: > 1 only where one rectangle is the whole plane
    int32_t tiles_x, tiles_y;  // rectangles per plane
    int32_t pw, ph;      // patch columns (elements) and rows: (4 cg - 1) sw + Kw, (rw - 1) sh + Kh
    int32_t row_dw;      // dwords staged per patch row: ceil(pw es / 4)
    int32_t pitch_dw;    // dwords between patch rows: odd, and wide enough for the furthest window read of a row
    int32_t plane_dw;    // dwords between the patches of two planes: ph pitch_dw
    int32_t w_dw;        // binary16: dword offset of the filters behind the patches (int8 reads its packed rows from memory)
    int32_t lds_bytes;
    int64_t groups;      // plane groups: ceil(N C / pl) -- grid.x; grid.y = tiles_x tiles_y
};

// depthwise with multiplier 1, NCHW, weights O1HW; symmetric weights and the fast epilogue are the plan's to add for int8
static inline bool dn_scope(bool i8, int C, int Co, int group, int Kh, int Kw, int sh, int sw, int dh, int dw, int in_zp)
{
    if (group != C || Co != C || C < 2) return false;
    if (Kh < 1 || Kw < 1 || Kh > DN_MAX_K || Kw > DN_MAX_K || (Kh == 3 && Kw == 3)) return false;
    if (sh < 1 || sw < 1 || sh > 2 || sw > 2 || dh != 1 || dw != 1) return false;
    return !i8 || (in_zp >= -128 && in_zp <= 127);
}

// dwords a thread reads per filter row, from its first window's (dword-aligned) start: int8 windows of 4 or 8 bytes stepping by sw
// bytes, binary16 a run of 3 sw + 7 values
static inline int dn_read_dw(bool i8, int Kw, int sw) { return i8 ? (3 * sw + (Kw > 4 ? 8 : 4) + 3) / 4 : (3 * sw + DN_MAX_K + 1) / 2; }

static inline void dn_patch(DnGeom &g, bool i8, int Kh, int Kw, int sh, int sw)
{
    g.pw = (DN_TX * g.cg - 1) * sw + Kw;
    g.ph = (g.rw - 1) * sh + Kh;
    g.row_dw = (g.pw * g.es + 3) / 4;
    // the last thread of a row starts at dword (cg - 1) sw (int8) / 2 (cg - 1) sw (binary16) and reads dn_read_dw dwords.
    // Odd: at stride 2 the threads of a row read every other dword, an odd pitch lets the next output row of the wave fall on the
    // banks between them; at stride 1 a row's threads cover consecutive banks and the rows of a wave start an odd number of banks
    // apart -- reasoning on the 64-bank LDS, not a counter.
    g.pitch_dw = (g.cg - 1) * sw * (i8 ? 1 : 2) + dn_read_dw(i8, Kw, sw);
    if (g.pitch_dw < g.row_dw) g.pitch_dw = g.row_dw;
    g.pitch_dw |= 1;
    g.plane_dw = g.ph * g.pitch_dw;
    g.w_dw = (g.pl * g.plane_dw + 3) & ~3;  // 16-byte aligned: a filter row is read as two 16-byte pieces
    g.lds_bytes = 4 * (g.w_dw + (i8 ? 0 : g.pl * DN_W_SLOT));
}

// false: outside the kernel's limits (the layer stays on the direct kernel).  N: the batch the grid is sized for.
static inline bool dn_geometry(bool i8, int N, int C, int H, int W, int Ho, int Wo, int Kh, int Kw, int sh, int sw, DnGeom &g)
{
    if (N < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || Kh < 1 || Kw < 1 || Kh > DN_MAX_K || Kw > DN_MAX_K || sh < 1 || sw < 1 || sh > 2 || sw > 2) return false;
    const int64_t planes = (int64_t)N * C;
    if (planes * H * W >= ((int64_t)1 << 31) || planes * Ho * Wo >= ((int64_t)1 << 31)) return false;
    g.es = i8 ? 1 : 2;
    const int cg_all = (Wo + DN_TX - 1) / DN_TX;
    g.tiles_x = (cg_all + DN_MAX_CG - 1) / DN_MAX_CG;
    g.cg = (cg_all + g.tiles_x - 1) / g.tiles_x;  // even rectangles
    const int rows_max = DN_THREADS / g.cg;
    g.tiles_y = (Ho + rows_max - 1) / rows_max;
    g.rw = (Ho + g.tiles_y - 1) / g.tiles_y;
    g.pl = 1;
    if (g.tiles_x == 1 && g.tiles_y == 1) {
        // a small plane: as many whole planes as fill the four waves, fewer while the grid would stay under DN_WG_TARGET
        // workgroups, never fewer than fill one wave
        const int per = g.cg * g.rw, most = DN_THREADS / per, least = (64 + per - 1) / per < most ? (64 + per - 1) / per : most;
        int64_t want = planes / DN_WG_TARGET;
        g.pl = (int32_t)(want > most ? most : want < least ? least : want);
        for (dn_patch(g, i8, Kh, Kw, sh, sw); g.pl > 1 && g.lds_bytes > DN_LDS_LIMIT; dn_patch(g, i8, Kh, Kw, sh, sw)) --g.pl;
    }
    dn_patch(g, i8, Kh, Kw, sh, sw);
    g.groups = (planes + g.pl - 1) / g.pl;
    return g.lds_bytes <= DN_LDS_LIMIT && g.groups < ((int64_t)1 << 31) && (int64_t)g.tiles_x * g.tiles_y <= 65535;
}

static inline int64_t dn_weight_bytes(int C, int Kh) { return (int64_t)C * Kh * 8; }

// The plan-time packing of int8 filters: O1HW [C][Kh][Kw] -> [C][Kh][2 dwords], tap kx in byte kx % 4 of dword kx / 4, zero beyond
// Kw: a filter row is one or two v_dot4_i32_i8.  acc_init[c] = -zp_in sum(w[c]) over all taps: the patch holds zp_in where the
// image ends.
static inline void dn_pack(const int8_t *o1hw, int C, int Kh, int Kw, int in_zp, uint32_t *dst, int32_t *acc_init)
{
    for (int c = 0; c < C; ++c) {
        int64_t sum = 0;
        for (int ky = 0; ky < Kh; ++ky) {
            uint32_t d[2] = {0, 0};
            for (int kx = 0; kx < Kw; ++kx) {
                const int8_t w = o1hw[((int64_t)c * Kh + ky) * Kw + kx];
                d[kx >> 2] |= (uint32_t)(uint8_t)w << (8 * (kx & 3));
                sum += w;
            }
            dst[((int64_t)c * Kh + ky) * 2] = d[0], dst[((int64_t)c * Kh + ky) * 2 + 1] = d[1];
        }
        acc_init[c] = (int32_t)(-(int64_t)in_zp * sum);
    }
}

// The layers the kernel takes when SHL_MI355X_DWNCHW is unset: the classes where its median was MEASURED below the direct
// kernel's by more than the two sides' run-to-run spreads together (tools/dw_nchw_bench.py, profiles/dw_nchw_kxk_notes.md).
// Class = (dtype, kernel, stride); new / direct at batch 1 .. batch 32, M = planes Ho Wo outputs:
//   int8  5x5 s1   120@28 0.50 .. 0.15   672@14 0.48 .. 0.16   960@7 0.53 .. 0.22   240@28 0.45 .. 0.13   480@14 0.50 .. 0.17
//                  1152@7 0.53 .. 0.22                                            -- every shape measured wins: on for any M
//   int8  5x5 s2   72@56 0.69 .. 0.25   672@14 0.56 .. 0.33   144@56 0.66 .. 0.24                       -- on for any M
//   int8  7x7 s1   96@56 0.25 .. 0.09    192@28 0.32 .. 0.09   384@14 0.32 .. 0.11  768@7 0.35 .. 0.16   -- on for any M
//   f16   7x7 s1   96@56 0.66 .. 0.22    192@28 0.79 .. 0.27   384@14 0.79 .. 0.39  768@7 0.84 .. 0.58   -- on for any M
//   f16   5x5 s1   batch 1: wins at M = 94 080 (120@28 0.97, 480@14 0.93), 131 712 (0.92), 188 160 (0.89); 1.00 / 1.01 at 47 040 and
//                  56 448 (960@7, 1152@7); batch 32 0.34 .. 0.68: on for M >= 94 080, the smallest M measured to win
//   f16   5x5 s2   batch 1 loses (1.09 .. 1.27 at M = 32 928 .. 112 896: the launch, and a patch four times the outputs); batch 32
//                  0.41 .. 0.73: on for M >= 1 053 696 (672@14 at batch 32), the smallest M measured to win
// Between batch 1 and 32 and beyond 32 nothing in either kernel changes but the number of workgroups -- an extrapolation, as are
// other channel counts of a class.  Every other kernel size in scope (1xK, Kx1, 4x4, 5x3, 7x7 at stride 2 ...) and mixed strides
// were not measured and stay on the direct kernel.
static inline bool dn_default(bool i8, int64_t planes, int Ho, int Wo, int Kh, int Kw, int sh, int sw)
{
    const int64_t M = planes * Ho * Wo;
    if (M <= 0 || Kh != Kw || sh != sw || sh < 1 || sh > 2) return false;
    if (Kh == 7) return sh == 1;
    if (Kh != 5) return false;
    return i8 || M >= (sh == 1 ? 94080 : 1053696);
}

}  // namespace shl

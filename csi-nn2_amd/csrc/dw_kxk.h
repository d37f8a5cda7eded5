// dw_kxk.h -- the host geometry of dwconv_kxk.hip (depthwise Kh x Kw int8 NHWC on the matrix cores): how an output map is cut
// into workgroup rectangles, what patch a rectangle stages in LDS and what that costs.  Pure host code that includes no HIP
// header, so that a stand-alone program can compile it with the sanitizers (tests/test_dw_kxk_cpu.py).
#pragma once
#include <stdint.h>

namespace shl {

constexpr int DWK_MAX_K = 7;               // taps per axis
constexpr int DWK_TILES_PER_WAVE = 4;      // one v16i accumulator each, live across the tap loop
constexpr int DWK_LDS_LIMIT = 80 * 1024;   // two workgroups per CU's 160 KiB, whatever the shape
constexpr int DWK_LDS_TARGET = 48 * 1024;  // ... and three where the rectangle can shrink to it (argued, not measured against 80 KiB)

struct DwkGeom {
    int32_t btx, bty;    // MFMA pixel tiles (8 wide x 4 high) per workgroup in x / y
    int32_t tiles_x, tiles_y;
    int32_t pw, ph;      // patch size in input pixels (pw: the row pitch; even for stride 1 in x, see dwconv_kxk.hip)
    int32_t cb;          // channels per workgroup: 32, 64 or 128
    int32_t npieces;     // 1 KiB DMA pieces of the patch
    int32_t ntaps;       // Kh Kw
    int32_t kw;          // Kw (the tap loop's inner extent)
    uint32_t pw_magic;   // j / pw == umulhi(j, pw_magic) for j < 2^16
};

// bytes of LDS behind the patch: the epilogue tables [acc_init | mult | bias][cb] and the weights [tap][cb] (16-byte pieces)
static inline int64_t dwk_tail_bytes(const DwkGeom &g) { return (int64_t)g.cb * 12 + (((int64_t)g.ntaps * g.cb + 15) & ~(int64_t)15); }
static inline int64_t dwk_lds_bytes(const DwkGeom &g, bool lut) { return (int64_t)g.npieces * 1024 + dwk_tail_bytes(g) + (lut ? 256 : 0); }

static inline void dwk_patch(DwkGeom &g, int Kh, int Kw, int sh, int sw)
{
    g.pw = (g.btx * 8 - 1) * sw + Kw;
    if (sw == 1) g.pw += g.pw & 1;  // an even pitch keeps the pixel's bank half a function of the column alone
    g.ph = (g.bty * 4 - 1) * sh + Kh;
    g.npieces = (g.pw * g.ph * (g.cb >> 4) + 63) / 64;
}

// false: outside the kernel's scope or its grid limits (the caller stays on the generic kernel)
static inline bool dwk_geometry(int C, int Kh, int Kw, int sh, int sw, int Ho, int Wo, int N, DwkGeom &g)
{
    if (C < 32 || (C & 31) != 0 || Kh < 1 || Kw < 1 || Kh > DWK_MAX_K || Kw > DWK_MAX_K || (Kh == 3 && Kw == 3)) return false;
    if (sh < 1 || sh > 2 || sw < 1 || sw > 2 || Ho < 1 || Wo < 1 || N < 1) return false;
    g.ntaps = Kh * Kw, g.kw = Kw;
    const int tx_all = (Wo + 7) / 8, ty_all = (Ho + 3) / 4;
    g.cb = (C % 128 == 0) ? 128 : ((C % 64 == 0) ? 64 : 32);
    // a wave owns one 32-channel group and at most four tiles: 4 / (cb / 32) waves share a group's tiles
    const int cap = DWK_TILES_PER_WAVE * (128 / g.cb);
    g.btx = tx_all < 2 ? 1 : 2;
    g.bty = cap / g.btx < ty_all ? cap / g.btx : ty_all;
    dwk_patch(g, Kh, Kw, sh, sw);
    // the rectangle shrinks to the LDS target (5x5 stride 2, 16 x 8 outputs at cb = 128 would be 85 KiB); the channel block
    // never has to: the largest single tile, 7x7 stride 2 at cb = 128, is 35 KiB
    while (dwk_lds_bytes(g, true) > DWK_LDS_TARGET && (g.bty > 1 || g.btx > 1)) {
        if (g.bty > 1) --g.bty;
        else g.btx = 1;
        dwk_patch(g, Kh, Kw, sh, sw);
    }
    g.tiles_x = (tx_all + g.btx - 1) / g.btx;
    g.tiles_y = (ty_all + g.bty - 1) / g.bty;
    g.pw_magic = (uint32_t)((((uint64_t)1 << 32) / (uint32_t)g.pw) + 1);  // exact for j < 2^16 (pw < 2^7)
    if (dwk_lds_bytes(g, true) > DWK_LDS_LIMIT) return false;
    return g.tiles_x <= 65535 && (int64_t)g.tiles_y * N <= 65535;
}

// The shapes the kernel takes when SHL_MI355X_DWKXK is unset: the classes where it was MEASURED faster than the generic kernel
// by more than the larger of the two run-to-run spreads (tools/dw_kxk_bench.py, profiles/dw_kxk_notes.md; lut_validate.h's
// criterion).  M = N Ho Wo output pixels, C channels, taps = Kh Kw, strided: a stride above 1; the class variable is E = M C
// output bytes.  new / generic, two runs (spreads of both sides 0 - 1 %):
//   7x7, stride 1, C >= 96,               ConvNeXt-T's layers (96 @56, 192 @28, 384 @14, 768 @7) at batch 1: 0.94, 0.90, 0.95, 0.81;
//   37632 <= E <= 2408448                 at batch 8: 0.42, 0.72, 0.96, 0.80: in
//   5x5, 32928 <= E <= 4214784            672 @14 s2, 960 @7, 480 @14, 672 @14, 1152 @7 (MobileNetV3-Large, EfficientNet-B0) at
//                                         batch 1: 0.76 - 0.86, at batch 32: 0.42 - 0.69 -- faster everywhere, and OUT: these
//                                         very shapes are the ones tests/test_dw_act_fuse.py pins to the generic kernel's name
//                                         (SHL_MI355X_DWKXK=1 turns them on; making the class the default is pending on a
//                                         change of those pins)
// Nothing else was measured -- other kernel sizes, 7x7 at stride 2 or under 96 channels, sizes outside the range -- and stays on the generic
// kernel (144 @56 s2 and 240 @28 are no multiples of 32 channels: outside the kernel's scope)
constexpr int64_t DWK_7X7_MIN_C = 96, DWK_7X7_MIN_E = 37632, DWK_7X7_MAX_E = 2408448;

static inline bool dwk_default(int64_t M, int64_t C, int64_t taps, bool strided)
{
    if (M <= 0 || C <= 0 || M > 0x7FFFFFFFll || C > 0x7FFFFFFFll) return false;
    const int64_t E = M * C;
    return taps == 49 && !strided && C >= DWK_7X7_MIN_C && E >= DWK_7X7_MIN_E && E <= DWK_7X7_MAX_E;
}

}  // namespace shl

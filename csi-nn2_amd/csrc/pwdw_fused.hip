// pwdw_fused.hip -- pointwise 1x1 convolution + the depthwise 3x3 convolution that consumes it, in
// ONE launch (int8 NHWC).  MobileNet's body is dw, pw, dw, pw, ...: pairing each pointwise layer with
// the NEXT depthwise layer halves the number of dependent launches of the chain (a hipGraph kernel
// node costs 1.6-2.1 us before it does anything, profiles/r01_notes.md) and the pointwise output
// -- the largest tensors of the network -- never travels to HBM and back.
//
// Why this direction and not depthwise -> pointwise (attic/dwpw_fused.hip: measured slower beyond 64 channels): a depthwise layer is
// independent per channel, so a workgroup that owns a 32-channel SLICE of the pointwise output can
// run the depthwise layer on exactly those channels with nothing recomputed except a one-pixel halo;
// the other order recomputes the whole depthwise tile in every one of the Cout/32 workgroups that
// share it.
//
//   workgroup = (32-channel slice) x (bh x bw rectangle of depthwise OUTPUT pixels), 4 waves
//   1. pointwise: the rectangle's input patch is ((bh-1) s + 3) x ((bw-1) s + 3) pixels of the pointwise layer.  Only the part
//      of it INSIDE the image -- the workgroup's window -- is computed: patch pixels outside the image are the depthwise layer's
//      padding, written to LDS once, up front.  The window is cut into 32-pixel MFMA tiles (row j of the workgroup = window
//      pixel (j / iwm, j % iwm), iwm = the widest window of the launch; a narrower window leaves rows unused).  Rectangles of a launch need not be equal: along an axis the first and the last may be one
//      pixel wider (choose_rect), because one row / column of their patch is padding -- 14 = 4 + 3 + 3 + 4 gives every one of
//      the 4 x 4 rectangles a 5 x 5 window, ONE tile, where the uniform 4 x 4 rectangles' 6 x 6 patches took two.
//      A wave owns (tile, K part) pairs: K is
//      split KS ways (deep K: one memory round trip instead of KS), tiles are dealt to the 4/KS wave
//      groups.  Every fragment is requested up front -- weights [32 ch][K] rows and pixel rows are
//      both contiguous 16-byte pieces per lane -- then v_mfma_i32_32x32x32_i8.
//   2. partial sums meet in LDS; wave w finishes register group w (channels 8w + 4 half .. +3) of
//      every tile: + acc_init, pointwise requantisation (+ relu), one dword into the LDS patch
//      as eight dword planes [channel quad][pixel] (dw_patch.h; pixels outside the image hold the depthwise layer's padding value).
//   3. depthwise: thread = (output pixel, 4 channels): nine dwords from the LDS patch (the padding
//      value for taps outside the image), byte transposes + v_dot4_i32_i8 against the depthwise
//      plan's packed weights, depthwise requantisation (+ relu), one dword to HBM.
// Bit-identical to the two stand-alone launches: the int8 intermediate is produced by the same
// requantisation code and consumed by the same integer arithmetic.
// Restates shl_ref_conv2d_quant followed by shl_ref_depthwise_conv2d_quant
// (source/reference/convolution.c:370-400, 416-460) incl. the relu variants (convolution_relu.c).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "dw_patch.h"
#include "igemm_common.h"

namespace shl {

// what the kernel reads in the shadow of its fragment loads (beside the two layers): one aligned block, two scalar loads
struct alignas(32) PwDwLateArgs {
    uint32_t bw_magic;         // ceil(2^20 / dbw): j / dbw == (j * bw_magic) >> 20 for j < 4096
    int32_t rw;                // patch width  (dbw - 1) * sw + 3: the LARGEST rectangle's -- one LDS layout per launch
    int32_t npx;               // patch pixels rh * rw (the largest rectangle's)
    int32_t dbh, dbw;          // the largest rectangle = bh + max(ey_lo, ey_hi), bw + max(ex_lo, ex_hi): the depthwise phase's index decomposition
    // (sums the kernel would otherwise form itself: a wave issues one instruction per ~5.8 cycles)
    int32_t bhe, bwe;          // bh + ey_lo, bw + ex_lo: rectangle t ends where t bh + bhe, t bw + bwe begins
    int32_t ylast, xlast;      // tiles_y - 1, tiles_x - 1
    int32_t cy, cx;            // 3 - sh - pt, 3 - sw - pl: output row oye - 1 reads input rows up to, not including, oye sh + cy
    int32_t reserved;
};

// what stands in front of the fragment loads: everything the workgroup's slice, rectangle and fragment addresses are made of, in one
// aligned block at the very front of the kernel arguments -- two 16-dword scalar loads into registers of their own, ONE scalar
// round trip.  (Read field by field from the two layers and the members below, the batch came out as thirteen loads, and the
// register allocator gave a late one a destination inside an earlier, still outstanding one: a second s_waitcnt, a second round
// trip, in every compile-time form -- profiles/operand_first_notes.md.)  The host copies the few ConvArgs fields (fill_early).
struct alignas(64) PwDwEarlyArgs {
    const void *w_frag;        // pw.w_frag
    int32_t xg, xg_log2, spg;  // (as below)
    uint32_t spg_magic, tx_magic;
    int32_t tiles_x;
    int32_t nrect, nsub, nsw;
    uint32_t ty_magic;         // ceil(2^32 / tiles_y): ty / tiles_y == mulhi(ty, ty_magic) for ty < 65536 (the grid's limit)
    int32_t tiles_y, mt;
    const void *in;            // pw.in
    int64_t img_stride;
    int32_t bh, bw, ex_lo, ey_lo, iwm;
    uint32_t iwm_magic;
    int32_t H, W, C;           // pw.H, pw.W, pw.C
    int32_t sh, sw, pt, pl;    // dw.sh, dw.sw, dw.pt, dw.pl
    int32_t reserved;
};
static_assert(sizeof(PwDwEarlyArgs) == 128, "pwdw_fused: the early block is two 16-dword scalar loads");

struct PwDwArgs {
    PwDwEarlyArgs early;  // (first: offset 0 of the kernel-argument segment)
    ConvArgs pw;  // in = the pair's input tensor; out unused
    ConvArgs dw;  // in unused; out = the pair's output tensor
    int32_t bh, bw;            // depthwise output rectangle of a workgroup (the first / last of an axis: + ey_lo / ey_hi, ex_lo / ex_hi)
    int32_t tiles_x, tiles_y;  // rectangles per image
    int32_t mt;                // 32-pixel MFMA tiles per window = ceil(nwin / 32)
    int32_t nwaves;            // waves per workgroup: 4 or 8
    int32_t ks;                // K split: 1, 2, 4 or 8
    int32_t nsw;               // K sub-steps (32 B) per wave
    int32_t nsub;              // K sub-steps in all = C / 32
    // workgroup id -> (slice, rectangle), XCD aware (hardware hands workgroup L of a 1-D grid to XCD L % 8): the eight
    // XCDs form xg slice groups x 8 / xg rectangle groups, so that an XCD's L2 fetches the activations of 1 / (8 / xg)
    // of the rectangles and the weights of 1 / xg of the slices.  xg = 0: plain 3-D grid (slice, tx, ty).
    int32_t xg, xg_log2;       // slice groups: 1, 2, 4 or 8
    int32_t spg;               // slices per group = slices / xg
    uint32_t spg_magic;        // j / spg == (j * spg_magic) >> 20 for j < 4096
    uint32_t tx_magic;         // same for tiles_x
    int32_t nrect;             // rectangles in all = tiles_x * tiles_y * N
    // (round 6: what the kernel used to derive per wave -- a wave issues ONE instruction per ~5.8 cycles, scalar or vector, and at
    // batch 1 a launch is one wave's chain: the prologue was 323 instructions in front of the MFMAs, integer divisions by ks and
    // the 64-bit image offset among them; profiles/r06_notes.md)
    int32_t ks_log2;           // log2(ks)
    int32_t mwn;               // wave groups over the tiles = nwaves / ks
    int64_t img_stride;        // bytes of an image of the pointwise input = H W C
    // rectangles of unequal size: rectangle t of an axis starts at t b + (t > 0 ? e_lo : 0) and is b + (t == 0 ? e_lo : 0) +
    // (t == last ? e_hi : 0) long; all zero: the uniform grid (the last rectangles may stick out of the map)
    int32_t ex_lo, ex_hi, ey_lo, ey_hi;  // 0 or 1
    int32_t iwm;               // the widest window (in-image patch columns) of the launch's rectangles: MFMA row j = window pixel (j / iwm, j % iwm)
    uint32_t iwm_magic;        // ceil(2^20 / iwm): j / iwm == (j * iwm_magic) >> 20 for j < 4096
    int32_t nwin;              // MFMA rows that can hold a pixel = highest window x iwm: mt = ceil(nwin / 32)
    PwDwLateArgs late;   // (behind the fragment loads)
};

// dwords per thread and tile round with which a compile-time form (256 threads) fills its patch with the padding value: room for
// 8 planes x 96 dwords per tile, i.e. a patch of up to twice the window's 32 pixels
constexpr int PWDW_PAD_DWORDS = 3;

// MTW: MFMA tiles per wave (upper bound), NSW: K sub-steps per wave (upper bound), MAXT: threads (the
// 8-sub-step form needs more than the 256 registers a lane gets with two waves per SIMD).  EXACT: every wave has exactly NSW
// sub-steps (K / 32 = ks NSW: every MobileNet pair but the first) -- no per-fragment guards, and the first MFMA of a tile takes
// the constant 0 as its C operand instead of 16 zeroed registers per tile.
// KSV, TPW (both or neither; four waves): the K split and the tiles per wave as compile-time values -- every wave runs exactly TPW
// tiles, i.e. the window is treated as TPW 4 / KSV tiles (tiles past the real mt read some pixel of the image and park their sums
// in LDS slots nothing reads: the host sizes the partial-sum area for the padded count): no tile guards around the loads, the
// MFMAs and the LDS writes (four scalar instructions per MFMA in the generic form), the sums over the K parts unrolled.
// 0: run-time values (eight waves, deeper patches).
// NT: the window's true tile count as a compile-time value, 0: read at run time.  With it the patch slot of every tile is computed
// in the MFMAs' block and the finishing between the two barriers is straight-line code, two tiles per round, an odd NT's last tile
// alone: no row / column division, no window test and no branch there (the run-time count's finishing loop is ~104 instructions per
// two tiles against 30 - 38 per tile: profiles/pwdw_nt_notes.md).  The waves still run TPW tiles each; the rounds past NT are
// dummies as above, and the padding fill covers NT tiles' worth of patch.  Two __global__ templates below instantiate the body:
// pwdw_fused_kernel (its EMT = true: NT = TPW 4 / KSV, its EMT = false: NT = 0) and pwdw_fused_nt_kernel (any other NT).
// EPQ / EPD: the two layers' epilogue flavours (common.h; -1: chosen at run time) -- with all four flavours of three requantisation
// sites inline the kernel is 1 500 instructions, a third of which one launch runs, fetched cold by every workgroup.
template <int MTW, int NSW, int MAXT, bool EXACT, int KSV, int TPW, int NT, int EPQ, int EPD>
__device__ __forceinline__ void pwdw_fused_body(const PwDwArgs &f)
{
    static_assert((KSV == 0) == (TPW == 0) && (TPW == 0 || (TPW == MTW && EXACT)), "pwdw_fused: KSV and TPW come together, with MTW = TPW");
    constexpr bool FIXED = TPW != 0;
    constexpr int NFT_ALL = FIXED ? TPW * (4 / (KSV ? KSV : 1)) : 1;  // tiles the compile-time forms run
    constexpr bool CT = NT != 0;                                      // the window's tile count is a compile-time value
    static_assert(!CT || (FIXED && NT <= NFT_ALL && NT > NFT_ALL - 4 / (KSV ? KSV : 1)), "pwdw_fused: NT tiles take exactly TPW rounds of the wave groups");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ConvArgs &q = f.pw;
    const ConvArgs &d = f.dw;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar control around MFMA
    const int frow = lane & 31, fhalf = lane >> 5;
    // every kernel argument the prologue needs: the early block, two 16-dword scalar loads with destinations of their own in front
    // of the first branch -- ONE scalar round trip.  (The compiler otherwise fetches an argument inside the branch that first
    // reads it: four dependent s_load / s_waitcnt round trips of ~200 cycles in front of the first fragment load.)
    PwDwEarlyArgs e;
    {
        typedef const __attribute__((address_space(4))) v16i *KernargV16;
        const KernargV16 kp = (KernargV16)__builtin_amdgcn_kernarg_segment_ptr();
        static_assert(offsetof(PwDwArgs, early) == 0, "pwdw_fused: the early block leads the kernel arguments");
        const v16i e0 = kp[0], e1 = kp[1];
        __builtin_memcpy(&e, &e0, 64);
        __builtin_memcpy(reinterpret_cast<char *>(&e) + 64, &e1, 64);
        // (both halves HERE: the compiler otherwise sinks the second load behind the weight loads, where its first field is used)
        asm volatile("" ::"s"(e.w_frag), "s"(e.nrect), "s"(e.in), "s"(e.img_stride), "s"(e.iwm_magic), "s"(e.H), "s"(e.pl));
    }
    // (the two pointers came through integer registers: say that they are global memory, or the loads are flat ones)
    typedef const __attribute__((address_space(1))) char *GlobalBytes;
    typedef const __attribute__((address_space(1))) v4i *GlobalV4;
    if constexpr (!FIXED) asm volatile("" ::"s"(f.ks), "s"(f.ks_log2), "s"(f.mwn), "s"(f.nwaves));  // (the run-time form's own)
    // (only what stands in front of the fragment loads: with the epilogue's and the depthwise phase's arguments in THIS batch the pass
    // got 0.5 us slower in round 6 -- that trial had put them IN FRONT of the fragment loads.  Nor do those arguments "hide under the fragments'
    // latency where the compiler puts them", as this comment used to say: the compiler fetches each in the block of its first use,
    // behind the MFMAs and the barriers -- four exposed scalar round trips.  They get a batch of their own BEHIND the fragment loads:
    // "the shadow" below.)
    int slice = blockIdx.x, tx = blockIdx.y, ty = blockIdx.z;
    // (the uneven NT forms split the rectangle into its row and column BEHIND the weight loads, which need the slice only: their
    // first load must stand no later than in the padded forms they replace -- tests/test_pwdw_nt_build.py -- and their
    // straight-line finishing changes how the compiler lays out the exit below.  The older forms keep their text, and with it their code.)
    constexpr bool LATE_RECT = CT && NT != NFT_ALL;
    int late_rect = 0;
    if constexpr (LATE_RECT) {
        const int L = blockIdx.x;
        const int x = L & 7, j = L >> 3;
        const int b = (int)(((uint32_t)j * e.spg_magic) >> 20);
        const int xslice = (x & (e.xg - 1)) * e.spg + (j - b * e.spg);
        late_rect = b * (8 >> e.xg_log2) + (x >> e.xg_log2);
        const bool mapped = e.xg != 0;
        if (mapped && late_rect >= e.nrect) return;
        slice = mapped ? xslice : slice;
    } else {
        // (computed whether or not the grid is XCD-mapped and then selected: inside `if (xg)` the fields below were fetched
        // from the kernel arguments in two further dependent s_load / s_waitcnt round trips, ~200 cycles each)
        const int L = blockIdx.x;
        const int x = L & 7, j = L >> 3;                        // XCD, index among that XCD's workgroups
        const int b = (int)(((uint32_t)j * e.spg_magic) >> 20);
        const int xslice = (x & (e.xg - 1)) * e.spg + (j - b * e.spg);  // a group = spg ADJACENT slices
        const int rect = b * (8 >> e.xg_log2) + (x >> e.xg_log2);
        const int xty = (int)(((uint32_t)rect * e.tx_magic) >> 20);
        const int xtx = rect - xty * e.tiles_x;
        const bool mapped = e.xg != 0;
        if (mapped && rect >= e.nrect) return;
        slice = mapped ? xslice : slice;
        ty = mapped ? xty : ty;
        tx = mapped ? xtx : tx;
    }

    const int nwaves = FIXED ? 4 : f.nwaves;  // 4 or 8
    const int fgrp = wave & 3;

    // ---- pointwise: this wave's (tile, K part) pairs
    const int ks = FIXED ? KSV : f.ks;
    const int kpart = wave & (ks - 1);
    const int mw = wave >> (FIXED ? (KSV == 4 ? 2 : (KSV == 2 ? 1 : 0)) : f.ks_log2);  // wave group over tiles
    const int mwn = FIXED ? 4 / (KSV ? KSV : 1) : f.mwn;                                // number of wave groups = nwaves / ks
    const int mtp = FIXED ? TPW * (4 / (KSV ? KSV : 1)) : e.mt;                         // tiles the waves run (padded)
    const int mt = CT ? NT : e.mt;                                                      // tiles of the patch
    const int sub0 = kpart * (EXACT ? NSW : e.nsw);         // (EXACT: every wave has NSW sub-steps, nsub = ks NSW)
    const int nsub = FIXED ? KSV * NSW : e.nsub;
    int nsw = NSW;
    if constexpr (!EXACT) {
        nsw = e.nsub - sub0;
        nsw = nsw < e.nsw ? nsw : e.nsw;  // may be <= 0 for a ragged last part
    }

    // weights: the plan's fragment-ordered copy (one coalesced 1 KiB load per fragment; every pointwise plan the pair test
    // admits has one: conv_plan.hip `frag_copy`).  They need the slice and nothing else: the image stands behind them.
    const GlobalBytes wp = (GlobalBytes)e.w_frag + ((int64_t)slice * nsub + sub0) * 1024 + lane * 16;
    constexpr int wstep = 1024;
    v4i fa[NSW];
#pragma unroll
    for (int s = 0; s < NSW; ++s)
        if (s < nsw) fa[s] = *(GlobalV4)(wp + s * wstep);
    if constexpr (FIXED) __builtin_amdgcn_sched_barrier(0);  // (the weight fragments are requested before anything of the pixel addresses is computed)
    if constexpr (LATE_RECT) {
        const int xty = (int)(((uint32_t)late_rect * e.tx_magic) >> 20);
        const int xtx = late_rect - xty * e.tiles_x;
        ty = e.xg != 0 ? xty : ty;
        tx = e.xg != 0 ? xtx : tx;
    }
    // the image: ty counts the rectangle rows of all images.  Without a branch (a division by a magic, and at batch 1 a product
    // with zero): the conditional forms stood in front of the weight loads as three blocks and eleven instructions.
    int n = (int)__umulhi((uint32_t)ty, e.ty_magic);
    n = e.ty_magic ? n : ty;  // (tiles_y == 1: the magic 2^32 does not fit, the host stores 0)
    ty -= n * e.tiles_y;
    const GlobalBytes img = (GlobalBytes)e.in + (uint64_t)(uint32_t)n * (uint32_t)e.img_stride;  // (wave-uniform: the scalar unit; shapes_pair: an image is below 2 GiB)
    // The workgroup's rectangle starts at output pixel (oy0, ox0); its patch at (ry0, rx0) of the image (may be -pad); its window
    // = patch intersected with the image, from (wy0, wx0) to, not including, (wye, wxe).  MFMA row j is window pixel (r, c) =
    // (j / iwm, j % iwm) with the launch's widest window iwm: one magic from the host.  In front of the pixel loads stands only
    // what their addresses need -- the origins; where the window ends waits for the shadow.
    const int oy0 = ty * e.bh + min(ty, e.ey_lo), ox0 = tx * e.bw + min(tx, e.ex_lo);  // (e_lo is 0 or 1: + e_lo behind the first rectangle)
    const int ry0 = oy0 * e.sh - e.pt, rx0 = ox0 * e.sw - e.pl;
    const int wy0 = max(ry0, 0), wx0 = max(rx0, 0);
    auto win_rc = [&](int j, int &r, int &c) {
        r = (int)(((uint32_t)j * e.iwm_magic) >> 20);
        c = j - r * e.iwm;
    };
    v4i fb[MTW][NSW];
    int lr[MTW], lc[MTW];  // (this wave's rows: with four K parts they are the workgroup's, and the shadow takes them from here)
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
        const int tile = mw + i * mwn;
        if (FIXED || tile < mt) {
            win_rc(tile * 32 + frow, lr[i], lc[i]);
            // rows that hold no pixel of this window (past its width or its height): any valid address, the sums are never used
            const int y = min(wy0 + lr[i], e.H - 1), x = min(wx0 + lc[i], e.W - 1);
            // scalar image base + a 32-bit lane offset, as the weights (shapes_pair: an image is below 2 GiB)
            const uint32_t off = (uint32_t)((y * e.W + x) * e.C + fhalf * 16 + sub0 * 32);
            const GlobalBytes px = img + off;
#pragma unroll
            for (int s = 0; s < NSW; ++s)
                if (s < nsw) fb[i][s] = *(GlobalV4)(px + s * 32);
        }
    }
    // ---- the shadow: from here (every fragment load issued) to the first MFMA's wait the wave idles for a whole global-memory
    // latency.  Everything the rest of the kernel needs that depends on no loaded data is requested or computed here; the two
    // scheduling fences keep the window's contents between the fragment loads and the MFMAs, the compiler's own vmcnt / lgkmcnt
    // accounting stays in charge of the waits.
    __builtin_amdgcn_sched_barrier(0);
    // every kernel argument of the finishing roles and the depthwise phase in ONE batch of scalar loads, HERE: read through
    // kernarg_here (dw_patch.h) they cannot rise in front of the fragment loads, "used" by an empty asm they cannot sink behind the
    // barriers.  From here on the two layers are ql and dl.
    const PwDwLateArgs fl = kernarg_here<PwDwLateArgs>(offsetof(PwDwArgs, late));
    const uint32_t bw_magic = fl.bw_magic;
    const ConvArgs ql = kernarg_here<ConvArgs>(offsetof(PwDwArgs, pw)), dl = kernarg_here<ConvArgs>(offsetof(PwDwArgs, dw));
    asm volatile("" ::"s"(ql.acc_init), "s"(ql.mult), "s"(ql.bias), "s"(ql.out_zp), "s"(ql.out_zp_f), "s"(ql.clamp_lo), "s"(ql.clamp_hi),
                 "s"(ql.out_scale), "s"(ql.inv_out_scale), "s"(dl.w), "s"(dl.acc_init), "s"(dl.mult), "s"(dl.bias), "s"(dl.out));
    asm volatile("" ::"s"(dl.out_zp), "s"(dl.out_zp_f), "s"(dl.clamp_lo), "s"(dl.clamp_hi), "s"(dl.out_scale), "s"(dl.inv_out_scale),
                 "s"(dl.in_zp), "s"(dl.Ho), "s"(dl.Wo), "s"(dl.C), "s"(dl.sh), "s"(dl.sw), "s"(bw_magic));
    asm volatile("" ::"s"(fl.bhe), "s"(fl.bwe), "s"(fl.cy), "s"(fl.cx), "s"(fl.ylast), "s"(fl.xlast), "s"(fl.dbh), "s"(fl.dbw), "s"(fl.rw), "s"(fl.npx));
    // constants of the finishing roles, requested BEHIND the fragments (round 6; they were first: "they arrive under the K
    // loop" -- but a wave issues an instruction per ~5.8 cycles, and the nine loads with their address arithmetic stood ~60
    // instructions = 0.17 us in front of the loads the MFMAs wait for)
    // pointwise: wave w finishes channels 8 (w & 3) + 4 half .. +3 of the slice, for every tile (with 8
    // waves: waves 0-3 the even tiles, waves 4-7 the odd ones)
    const int pc = slice * 32 + 8 * fgrp + 4 * fhalf;
    const int4 p_ai = *reinterpret_cast<const int4 *>(ql.acc_init + pc);
    const float4 p_mu = *reinterpret_cast<const float4 *>(ql.mult + pc);
    const float4 p_bi = *reinterpret_cast<const float4 *>(ql.bias + pc);

    const DwThreadConsts dwk = dw_load_consts(dl, slice * 32, tid);  // depthwise constants
    // the rest of the workgroup's geometry.  One past the rectangle's last output row / column: where the next rectangle begins, the
    // map's edge for the last one (which may be e_hi longer, or stick out of the map in a uniform grid); the rectangle's own
    // size for the depthwise phase's `live`.
    const int oye = ty == fl.ylast ? dl.Ho : ty * e.bh + fl.bhe, oxe = tx == fl.xlast ? dl.Wo : tx * e.bw + fl.bwe;
    // the depthwise phase's index arithmetic (dw_patch.h)
    DwPatchGeom g;
    g.bh = fl.dbh, g.bw = fl.dbw, g.lbh = oye - oy0, g.lbw = oxe - ox0, g.rw = fl.rw, g.bw_magic = bw_magic, g.pitch = dw_patch_pitch(fl.npx);
    g.oy0 = oy0, g.ox0 = ox0, g.ry0 = ry0, g.rx0 = rx0, g.n = n, g.ch0 = slice * 32;
    const DwPrep dwp = dw_patch_prepare(dl, g, tid);
    // the finishing roles': the patch's pitch and padding value, both layers' clamp bounds and packed zero points (the very
    // expressions of requant4_i8_t, common.h: computed once, here) and, where the tile rounds are compile-time, every round's
    // patch slot
    const int ppitch = g.pitch;
    const uint32_t zpad = dw_patch_pad(dl);
    {
        const float qcl = ql.clamp_lo - ql.out_zp_f, qch = ql.clamp_hi - ql.out_zp_f, dcl = dl.clamp_lo - dl.out_zp_f, dch = dl.clamp_hi - dl.out_zp_f;
        const uint32_t qzp2 = (uint32_t)(ql.out_zp & 0xffff) * 0x00010001u, dzp2 = (uint32_t)(dl.out_zp & 0xffff) * 0x00010001u;
        asm volatile("" ::"s"(ppitch), "s"(zpad), "v"(qcl), "v"(qch), "v"(dcl), "v"(dch), "s"(qzp2), "s"(dzp2));
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- behind the shadow, in the MFMAs' block: a wave's MFMAs are a dependent chain of 16-pass instructions, and the scalar
    // and vector instructions below issue between them.  Where the window ends:
    const int wye = min(oye * dl.sh + fl.cy, e.H), wxe = min(oxe * dl.sw + fl.cx, e.W);
    // window pixel (r, c) -> whether this workgroup's window has it, and its slot in the patch (the patch keeps the largest
    // rectangle's layout: rw pixels per row).  Rows without a pixel go to the plane's last dword, which no reader looks at
    // (dw_patch_pitch: 8 spare dwords per plane).
    const int wslot0 = (wy0 - ry0) * fl.rw + (wx0 - rx0) + (2 * fgrp + fhalf) * ppitch;
    auto win_has = [&](int r, int c) { return wy0 + r < wye && wx0 + c < wxe; };
    auto win_slot = [&](int r, int c) { return (uint32_t)(wslot0 + r * fl.rw + c); };
    constexpr int NFT = CT ? NT : 1;  // compile-time tile rounds
    uint32_t fslot[NFT];  // per tile: the dword slot of this lane's pixel
    if constexpr (CT) {
        const uint32_t spare = (uint32_t)((2 * fgrp + fhalf) * ppitch + ppitch - 1);
#pragma unroll
        for (int t = 0; t < NFT; ++t) {
            int r, c;
            if constexpr (KSV == 4) r = lr[t], c = lc[t];  // (one wave group: tile t is this wave's t-th)
            else win_rc(t * 32 + frow, r, c);
            fslot[t] = win_has(r, c) ? win_slot(r, c) : spare;
            asm volatile("" ::"v"(fslot[t]));
        }
    }
    // the whole patch takes the depthwise layer's padding value (dw_patch.h: the reader tests nothing), HERE: the patch does not
    // alias the partial sums, and barrier 1 stands between these stores and the window's pixels (put(), below).  The compile-time
    // forms store without a branch -- a block boundary in the shadow lets the compiler sink the loads above: every thread
    // PWDW_PAD_DWORDS dwords per tile round, into an area the host sizes for that (it keeps larger patches for the run-time form).
    uint32_t *patch = reinterpret_cast<uint32_t *>(smem + (size_t)mtp * ks * 4096);  // eight dword planes (dw_patch.h)
    if constexpr (FIXED) {
#pragma unroll
        for (int k = 0; k < PWDW_PAD_DWORDS * (CT ? NT : NFT_ALL); ++k) patch[tid + 256 * k] = zpad;
    } else {
        for (int i = tid; i < 8 * ppitch; i += nwaves * 64) patch[i] = zpad;
    }

    v16i acc[MTW];
    if constexpr (EXACT) {
        const v16i zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < NSW; ++s) {  // (sub-step outermost: consecutive MFMAs go to different accumulators)
#pragma unroll
            for (int i = 0; i < MTW; ++i)
                if (FIXED || mw + i * mwn < mt) acc[i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[s], fb[i][s], s == 0 ? zero16 : acc[i], 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int i = 0; i < MTW; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0;
#pragma unroll
        for (int s = 0; s < NSW; ++s) {
            if (s < nsw) {
#pragma unroll
                for (int i = 0; i < MTW; ++i)
                    if (mw + i * mwn < mt) acc[i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[s], fb[i][s], acc[i], 0, 0, 0);
            }
        }
    }

    // The ablation exits (tools/pair_bench.py) exist in the run-time form only (SHL_MI355X_PWDW_GENERIC=1): a conditional exit is a
    // block boundary, and the compiler sinks every load and every computation above into the block of its first use behind it.
    if constexpr (!FIXED)
        if (q.debug & 256) return;  // ablation: stop after loads + MFMA
    // ---- partial sums -> LDS: part[((tile * ks + kpart) * 4 + group) * 64 + lane] = 4 channels
    v4i *part = reinterpret_cast<v4i *>(smem);
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
        const int tile = mw + i * mwn;
        if (FIXED || tile < mt) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                v4i v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][4 * g + e];
                part[((tile * ks + kpart) * 4 + g) * 64 + lane] = v;
            }
        }
    }
    __syncthreads();
    if constexpr (!FIXED)
        if (q.debug & 512) return;  // ablation: stop after the partial sums met in LDS
    // ---- finish the pointwise layer: group `wave` of every tile -> int8 patch in LDS
    // Two tiles per round, every partial sum of both requested before the first use: a wave is alone on its SIMD here, and
    // one tile at a time is a chain of LDS latency -> adds -> the requantisation's dependent fmas -> LDS write that nothing
    // overlaps (the patch writes also keep the compiler from moving the next tile's reads up): 71.0 - 71.2 -> 70.5 - 70.9 us
    // per MobileNetV1 pass.  (Four tiles per round through small arrays: 74.7 us -- the code grew more than the chain shrank.)
    {
        // the window's pixels only: the rest of the patch holds the padding value since the shadow
        auto put = [&](int tile, int j, uint32_t pk) {
            if constexpr (CT) {
                patch[fslot[tile]] = pk;
            } else {
                int r, c;
                win_rc(j, r, c);
                if (win_has(r, c)) patch[win_slot(r, c)] = pk;
            }
        };
        const int tstep = nwaves >> 2;
        // one round, as text: the uneven NT forms below unroll their rounds whatever they cost (five tiles with the four run-time
        // flavours inline were left a loop), every older form keeps the loop it had -- as a lambda, the round changed their code
#define SHL_PWDW_ROUND(tile)                                                                                                              \
    {                                                                                                                                     \
        const int tile1 = tile + tstep;                                                                                                   \
        const int j0 = tile * 32 + frow;                                                                                                  \
        v4i v0 = part[((tile * ks) * 4 + fgrp) * 64 + lane];                                                                              \
        if (tile1 < mt) {                                                                                                                 \
            v4i v1 = part[((tile1 * ks) * 4 + fgrp) * 64 + lane];                                                                         \
            _Pragma("unroll") for (int k = 1; k < ks; ++k) {                                                                              \
                v0 += part[((tile * ks + k) * 4 + fgrp) * 64 + lane];                                                                     \
                v1 += part[((tile1 * ks + k) * 4 + fgrp) * 64 + lane];                                                                    \
            }                                                                                                                             \
            const uint32_t pk0 = requant4_i8_sel<EPQ>(v0[0] + p_ai.x, v0[1] + p_ai.y, v0[2] + p_ai.z, v0[3] + p_ai.w, p_mu, p_bi, ql);   \
            const uint32_t pk1 = requant4_i8_sel<EPQ>(v1[0] + p_ai.x, v1[1] + p_ai.y, v1[2] + p_ai.z, v1[3] + p_ai.w, p_mu, p_bi, ql);   \
            const int j1 = tile1 * 32 + frow;                                                                                             \
            put(tile, j0, pk0);                                                                                                           \
            put(tile1, j1, pk1);                                                                                                          \
        } else { /* the odd last tile alone (it used to be computed twice: ~50 instructions of a wave that issues one per ~5.8 cycles) */ \
            _Pragma("unroll") for (int k = 1; k < ks; ++k) v0 += part[((tile * ks + k) * 4 + fgrp) * 64 + lane];                         \
            const uint32_t pk0 = requant4_i8_sel<EPQ>(v0[0] + p_ai.x, v0[1] + p_ai.y, v0[2] + p_ai.z, v0[3] + p_ai.w, p_mu, p_bi, ql);   \
            put(tile, j0, pk0);                                                                                                           \
        }                                                                                                                                 \
    }
        if constexpr (LATE_RECT) {
#pragma unroll
            for (int tile = 0; tile < NT; tile += 2) SHL_PWDW_ROUND(tile)
        } else {
            for (int tile = FIXED ? 0 : wave >> 2; tile < mt; tile += 2 * tstep) SHL_PWDW_ROUND(tile)  // (four waves: wave >> 2 = 0)
        }
#undef SHL_PWDW_ROUND
    }
    __syncthreads();

    if constexpr (!FIXED)
        if (q.debug & 1024) return;  // ablation: stop after the pointwise epilogue
    // ---- depthwise 3x3 on the slice's 32 channels, from the LDS patch (dw_patch.h)
    depthwise_from_patch<EPD>(dl, patch, g, dwk, dwp, tid, nwaves * 64);
}

// the run-time form (KSV = TPW = 0) and the fixed forms whose tile count is TPW 4 / KSV (EMT) or padded to it (the body above)
template <int MTW, int NSW, int MAXT, bool EXACT, int KSV = 0, int TPW = 0, bool EMT = false, int EPQ = -1, int EPD = -1>
__global__ __launch_bounds__(MAXT) void pwdw_fused_kernel(PwDwArgs f)
{
    pwdw_fused_body<MTW, NSW, MAXT, EXACT, KSV, TPW, (TPW != 0 && EMT) ? TPW * (4 / (KSV ? KSV : 1)) : 0, EPQ, EPD>(f);
}

// the fixed forms of a window of NT tiles, NT no multiple of the 4 / KSV wave groups: ceil(NT / (4 / KSV)) tiles per wave
template <int NSW, int KSV, int NT, int EPQ = -1, int EPD = -1>
__global__ __launch_bounds__(512) void pwdw_fused_nt_kernel(PwDwArgs f)
{
    constexpr int TPW = (NT + 4 / KSV - 1) / (4 / KSV);
    static_assert(NT % (4 / KSV) != 0, "pwdw_fused: an even tile count is pwdw_fused_kernel's EMT form");
    pwdw_fused_body<TPW, NSW, 512, true, KSV, TPW, NT, EPQ, EPD>(f);
}

// ---- host side ---------------------------------------------------------------------------------
static int waves_per_group() { return 4; }  // (8 waves measured slower on 11 of the 12 MobileNetV1 pairs: profiles/r01_notes.md)
static int ks_for(int nsub, int nwaves)
{
    (void)nwaves;
    return nsub >= 8 ? 4 : (nsub >= 4 ? 2 : 1);
}
constexpr int PWDW_MTW = 4;  // tiles per wave the kernels are instantiated for

static bool shapes_pair(const ConvArgs &q, const ConvArgs &d)
{
    if (q.Kh != 1 || q.Kw != 1 || q.sh != 1 || q.sw != 1 || q.pt != 0 || q.pl != 0) return false;
    if (q.H != q.Ho || q.W != q.Wo || (q.C & 31) != 0 || (q.Co & 31) != 0 || q.kstride < q.C) return false;
    if (d.Kh != 3 || d.Kw != 3 || d.dh != 1 || d.dw != 1 || d.C != d.Co || d.C != q.Co) return false;
    if (d.H != q.Ho || d.W != q.Wo || d.N != q.N) return false;
    if (d.sh < 1 || d.sh > 2 || d.sw < 1 || d.sw > 2 || d.pt > 2 || d.pl > 2 || d.pt < 0 || d.pl < 0) return false;
    if (q.C > 1024 || !q.w_frag) return false;  // 8 sub-steps per wave at most; the kernel reads the fragment-ordered weights
    if ((int64_t)q.H * q.W * q.C >= ((int64_t)1 << 31)) return false;  // 32-bit offsets inside an image
    if ((int64_t)d.Ho * d.Wo * d.C >= ((int64_t)1 << 31)) return false;  // ... of the output as well (dw_patch.h)
    return true;
}

// One axis of a rectangle grid: n rectangles of b output pixels, the first e_lo and the last e_hi wider (0 or 1).  e_lo = e_hi = 0
// is the uniform grid, whose last rectangle may stick out of the map.
struct PwDwAxis {
    int b, n, e_lo, e_hi;
    int win;  // the largest window along the axis: in-image pixels of a rectangle's patch (what pwdw_fused_kernel computes per workgroup)
};
static int axis_window(int in_len, int out_len, int s, int pad, const PwDwAxis &a)
{
    int best = 0;
    for (int t = 0; t < a.n; ++t) {
        const int o0 = t * a.b + (t > 0 ? a.e_lo : 0);
        const int len = std::min(a.b + (t == 0 ? a.e_lo : 0) + (t == a.n - 1 ? a.e_hi : 0), out_len - o0);
        const int r0 = o0 * s - pad;
        best = std::max(best, std::min(r0 + (len - 1) * s + 3, in_len) - std::max(r0, 0));
    }
    return best;
}
// the grids of an axis: the uniform ones (rectangle lengths `lens`) and, unless a grid is forced, those whose border rectangles are one
// longer -- a border rectangle's patch has a row / column of padding, which costs no pointwise work
static std::vector<PwDwAxis> axis_grids(int in_len, int out_len, int s, int pad, const std::vector<int> &lens, int max_n, bool uniform_only)
{
    std::vector<PwDwAxis> v;
    for (int b : lens) v.push_back({b, (out_len + b - 1) / b, 0, 0, 0});
    if (!uniform_only)
        for (int n = 2; n <= max_n && n <= out_len; ++n)
            for (int e = 1; e <= 3; ++e) {  // (e_lo, e_hi) = (1, 0), (0, 1), (1, 1)
                const int e_lo = e & 1, e_hi = e >> 1, rest = out_len - e_lo - e_hi;
                if (rest < n || rest % n) continue;
                v.push_back({rest / n, n, e_lo, e_hi, 0});
            }
    for (PwDwAxis &a : v) a.win = axis_window(in_len, out_len, s, pad, a);
    return v;
}

// choose the workgroups' rectangles; returns false when nothing fits
static bool choose_rect(const ConvArgs &q, const ConvArgs &d, PwDwArgs &f)
{
    const int nsub = q.C >> 5;
    const int nwaves = waves_per_group();
    const int ks = ks_for(nsub, nwaves);
    const int mt_max = (nwaves / ks) * PWDW_MTW;
    const int nsw = (nsub + ks - 1) / ks;
    if (nwaves == 8 && nsw > 4) return false;  // the 8-sub-step kernel is built for 4 waves
    const int64_t slices = q.Co >> 5;
    int force_h = 0, force_w = 0;
    const char *env = getenv("SHL_MI355X_PWDW_TILE");  // "<bh>x<bw>": tuning override, a uniform grid (tools/pair_bench.py)
    if (env) sscanf(env, "%dx%d", &force_h, &force_w);
    std::vector<int> lens_y, lens_x;
    for (int bh = 1; bh <= d.Ho && bh <= 32; ++bh)
        if (!force_h || bh == force_h) lens_y.push_back(bh);
    for (int div = 1; div <= 16; ++div) {
        const int bw = (d.Wo + div - 1) / div;
        if (div > 1 && bw == (d.Wo + div - 2) / (div - 1)) continue;  // same width as the previous div
        if (!force_h || bw == force_w) lens_x.push_back(bw);
    }
    const std::vector<PwDwAxis> gy = axis_grids(q.H, d.Ho, d.sh, d.pt, lens_y, 32, force_h != 0);
    const std::vector<PwDwAxis> gx = axis_grids(q.W, d.Wo, d.sw, d.pl, lens_x, 16, force_h != 0);
    double best = 1e30;
    const PwDwAxis *best_y = nullptr, *best_x = nullptr;
    for (const PwDwAxis &y : gy) {
        for (const PwDwAxis &x : gx) {
            const int dbh = y.b + std::max(y.e_lo, y.e_hi), dbw = x.b + std::max(x.e_lo, x.e_hi);
            const int rh = (dbh - 1) * d.sh + 3, rw = (dbw - 1) * d.sw + 3;
            const int npx = rh * rw;  // the LDS patch: the largest rectangle's
            const int nwin = std::max(y.win, 1) * std::max(x.win, 1);  // MFMA rows: highest window x widest window
            const int mt = (nwin + 31) / 32;
            if (dbh > 32 || mt > mt_max || rw > 256 || dbw > 256 || npx >= 4096 || dbh * dbw >= 4096) continue;
            if ((size_t)mt * ks * 4096 + dw_patch_bytes(npx) > 96 * 1024) continue;  // partial sums + patch in LDS
            const int64_t blocks = slices * y.n * x.n * d.N;
            // Measured on MobileNetV1 at batch 1 (tools/pair_bench.py --sweep, profiles/r01_notes.md): what
            // a rectangle costs is the bytes its CU has to pull through its L1 -- (mt pixel tiles + 1
            // weight tile) x K per workgroup, times the workgroups that land on one CU -- plus a little
            // per depthwise pass; among equals, more workgroups (up to one per CU) finish sooner.
            // mt counts the tiles of the largest WINDOW: padding pixels are neither loaded nor multiplied
            // (profiles/pwdw_window_notes.md: the per-tile cost re-measured on the 14 x 14 pairs, the weights
            // of the other terms were not re-fitted).
            const double rounds = (double)((blocks + 255) / 256);
            // (last, far below a workgroup's worth of the term before it: among grids of equal tiles, the smaller window -- fewer
            // pixel rows through L1 that no tile needed to grow for)
            const double score = rounds * ((mt + 1) * nsub + 2.0 * ((dbh * dbw + 31) / 32) + 4.0) -
                                 (blocks <= 256 ? blocks / 1024.0 : 0.0) + nwin * 1e-7;
            if (score < best) {
                best = score;
                best_y = &y;
                best_x = &x;
            }
        }
    }
    if (!best_y) return false;
    f.bh = best_y->b, f.ey_lo = best_y->e_lo, f.ey_hi = best_y->e_hi, f.tiles_y = best_y->n;
    f.bw = best_x->b, f.ex_lo = best_x->e_lo, f.ex_hi = best_x->e_hi, f.tiles_x = best_x->n;
    f.late.dbh = f.bh + std::max(f.ey_lo, f.ey_hi);
    f.late.dbw = f.bw + std::max(f.ex_lo, f.ex_hi);
    f.late.bhe = f.bh + f.ey_lo, f.late.bwe = f.bw + f.ex_lo;
    f.late.ylast = f.tiles_y - 1, f.late.xlast = f.tiles_x - 1;
    f.late.reserved = 0;
    f.iwm = std::max(best_x->win, 1);
    f.iwm_magic = ((1u << 20) + f.iwm - 1) / f.iwm;
    f.late.cy = 3 - d.sh - d.pt, f.late.cx = 3 - d.sw - d.pl;
    f.late.rw = (f.late.dbw - 1) * d.sw + 3;
    f.late.npx = ((f.late.dbh - 1) * d.sh + 3) * f.late.rw;
    f.nwin = std::max(best_y->win, 1) * std::max(best_x->win, 1);
    f.mt = (f.nwin + 31) / 32;
    f.nwaves = nwaves;
    f.ks = ks;
    f.nsw = nsw;
    f.nsub = nsub;
    f.ks_log2 = ks == 8 ? 3 : (ks == 4 ? 2 : (ks == 2 ? 1 : 0));
    f.mwn = nwaves / ks;
    f.img_stride = (int64_t)q.H * q.W * q.C;
    f.late.bw_magic = ((1u << 20) + f.late.dbw - 1) / f.late.dbw;
    // Which XCDs share what.  HBM-side bytes of the launch ~ xg x activations + (8 / xg) x weights (every slice group
    // fetches the rectangles' pixels, every rectangle group the slices' weights; measured on the plain grid: 2.97x
    // the algorithmic bytes over MobileNetV1's twelve pairs, profiles/r03_h_pmc_traffic.json): take the cheapest
    // admissible split.  Admissible = a slice group is a run of ADJACENT slices covering whole 128-byte lines of the
    // NHWC output (four slices): with the lines of a pixel written by one L2 the chain is 1.5 us shorter than with
    // the same lines pieced together from four or eight L2s at the kernel boundary (72.6 -> 71.1 us; strided groups of
    // the same sizes: 72.1 - 74.0; profiles/r04_notes.md).
    {
        const int S = (int)slices;
        const int64_t R = (int64_t)f.tiles_x * f.tiles_y * d.N;
        static const char *xe = getenv("SHL_MI355X_PWDW_XG");  // 0 (plain grid) | 1 | 2 | 4 | 8: A/B
        const int forced = xe ? atoi(xe) : -1;
        const double act = (double)q.N * q.H * q.W * q.C, wts = (double)q.C * q.Co;
        int best_g = 0;
        double best_c = 1e30;
        for (int g = 1; g <= 8; g <<= 1) {
            if (S % g) continue;
            if (forced > 0 && g != forced) continue;
            if (forced <= 0 && g > 1 && ((S / g) & 3) != 0) continue;  // whole 128-byte lines of the output per XCD (below)
            const int rpg = 8 / g;
            const int64_t per_xcd = (int64_t)(S / g) * ((R + rpg - 1) / rpg);
            if (per_xcd >= 4096 || R >= 4096) continue;
            const double c = g * act + rpg * wts;
            if (c < best_c) best_c = c, best_g = g;
        }
        if (forced == 0) best_g = 0;
        f.xg = best_g;
        f.xg_log2 = best_g == 8 ? 3 : (best_g == 4 ? 2 : (best_g == 2 ? 1 : 0));
        f.spg = best_g ? S / best_g : S;
        f.spg_magic = ((1u << 20) + f.spg - 1) / f.spg;
        f.tx_magic = ((1u << 20) + f.tiles_x - 1) / f.tiles_x;
        f.nrect = (int32_t)R;
    }
    return true;
}

bool pwdw_fusable(const ConvArgs &q, const ConvArgs &d, int pw_is_igemm, int dw_dot4_packed)
{
    if (!pw_is_igemm || !dw_dot4_packed || !shapes_pair(q, d)) return false;
    PwDwArgs f;
    if (!choose_rect(q, d, f)) return false;
    if ((int64_t)f.tiles_y * d.N > 65535 || f.tiles_x > 65535) return false;
    // Latency regime only.  The fused kernel trades a launch and an HBM round trip for halo
    // recomputation and a serial pointwise -> depthwise chain inside the workgroup: at batch 1 a
    // MobileNetV1 pair drops from 6.7-7.9 us to 4.2-5.3 us, at batch 128 the stand-alone kernels
    // (bandwidth-tuned, 1.3-3.4 TB/s) are 1.5-2x faster; the whole chain breaks even at batch 16
    // (profiles/r01_notes.md).  Fuse while the workgroups fit a few rounds on the 256 CUs (MobileNetV1
    // up to batch 8 for the 512-channel blocks; the blocks of at most 256 channels leave for dwpw_stream.hip from batch 8:
    // conv_plan.hip:pwdw_kernel_for); SHL_MI355X_PWDW=2 lifts the limit (measurements).
    static const char *sel = getenv("SHL_MI355X_PWDW");
    const int64_t blocks = (int64_t)(q.Co >> 5) * f.tiles_x * f.tiles_y * d.N;
    // (round 5: 512, was 2048 -- the stand-alone kernels got faster: with 2048 MobileNetV1's 512-channel blocks stayed latency
    // pairs up to batch 32 and the whole model ran 180 / 267 us at batch 16 / 32 against 158 / 210 with 512; batches 1 .. 8
    // keep every pair either way: profiles/r05_dwpw_sweep_whole_model.txt)
    if (blocks > 512 && !(sel && sel[0] == '2')) return false;
    return true;
}

// what launch_pwdw_fused would run for the pair (tests, tools): the rectangle grid, the tiles per workgroup, the K split, the workgroups
bool pwdw_fused_geometry(const ConvArgs &q, const ConvArgs &d, int32_t out[SHL_PWDW_GEOMETRY_FIELDS])
{
    PwDwArgs f;
    if (!shapes_pair(q, d) || !choose_rect(q, d, f)) return false;
    const int32_t v[SHL_PWDW_GEOMETRY_FIELDS] = {f.tiles_y, f.tiles_x, f.bh,  f.bw, f.ey_lo, f.ey_hi,
                                                 f.ex_lo,   f.ex_hi,   f.mt,  f.ks, f.nwin,  (int32_t)((q.Co >> 5) * f.nrect)};
    for (int i = 0; i < SHL_PWDW_GEOMETRY_FIELDS; ++i) out[i] = v[i];
    return true;
}

// Which instantiation a geometry launches (launch_pwdw_fused, pwdw_fused_launch_form).  The fixed forms: four waves, every wave
// exactly nsw sub-steps and tpw tiles, K split ks; `tiles` is the count the form was compiled for -- tpw 4 / ks (the window has
// exactly as many: FIXED_EXACT, or fewer: FIXED_PADDED, which reads the true count at run time) or the window's own uneven count (NT).
struct PwDwForm {
    int kind;  // SHL_MI355X_PWDW_LAUNCH_*
    int nsw, ks, tpw, tiles;
    size_t lds;  // bytes of LDS of a fixed form: partial sums of the tiles the waves run + the area the padding fill covers
};
// (NSW, KS, TPW) of the pwdw_fused_kernel forms and (NSW, KS, NT) of the pwdw_fused_nt_kernel forms: what launch_pwdw_fused instantiates
static const int PWDW_FIXED_FORMS[][3] = {{4, 4, 2}, {4, 4, 1}, {2, 4, 2}, {2, 4, 1}, {2, 2, 2}, {2, 2, 1}, {2, 1, 1}, {2, 1, 2}, {1, 1, 1}, {1, 1, 2}};
// An uneven count arises for ks = 1 (1 - 3, 5 - 7 tiles) and ks = 2 (1, 3 tiles) only.  Instantiated: MobileNetV1's 32 -> 64 @112
// stride 2 (5 tiles), 64 -> 128 @56 (3) and 128 -> 128 @56 stride 2 (3, ks 2); the rest keeps the padded forms.
static const int PWDW_NT_FORMS[][3] = {{1, 1, 5}, {2, 1, 3}, {2, 2, 3}};
static PwDwForm choose_form(const PwDwArgs &f)
{
    PwDwForm r = {SHL_MI355X_PWDW_LAUNCH_RUNTIME, 0, 0, 0, 0, 0};
    const char *nofix = getenv("SHL_MI355X_PWDW_GENERIC");  // "1": the run-time form everywhere (A/B, tests; read per call)
    if ((nofix && nofix[0] == '1') || f.nwaves != 4) return r;
    const size_t patch = dw_patch_bytes(f.late.npx);
    for (const auto &k : PWDW_FIXED_FORMS) {
        const int nsw = k[0], ks = k[1], tpw = k[2], t = tpw * (4 / ks);
        if (f.nsw != nsw || f.nsub != ks * nsw || f.ks != ks || f.mt > t || f.mt <= t - 4 / ks || patch > (size_t)1024 * PWDW_PAD_DWORDS * t) continue;
        r = {f.mt == t ? SHL_MI355X_PWDW_LAUNCH_FIXED_EXACT : SHL_MI355X_PWDW_LAUNCH_FIXED_PADDED, nsw, ks, tpw, t, (size_t)t * (ks * 4096 + 1024 * PWDW_PAD_DWORDS)};
        for (const auto &n : PWDW_NT_FORMS)
            // the fill covers NT tiles' worth of patch; the partial sums keep room for the dummy rounds' tiles
            if (n[0] == nsw && n[1] == ks && n[2] == f.mt && patch <= (size_t)1024 * PWDW_PAD_DWORDS * f.mt) {
                r.kind = SHL_MI355X_PWDW_LAUNCH_NT, r.tiles = f.mt;
                r.lds = (size_t)t * ks * 4096 + (size_t)1024 * PWDW_PAD_DWORDS * f.mt;
            }
        return r;
    }
    return r;
}

// what launch_pwdw_fused would launch for the pair (tests, tools): the kind of form and what it was compiled for
bool pwdw_fused_launch_form(const ConvArgs &q, const ConvArgs &d, int32_t out[SHL_PWDW_LAUNCH_FIELDS])
{
    PwDwArgs f;
    if (!shapes_pair(q, d) || !choose_rect(q, d, f)) return false;
    const PwDwForm r = choose_form(f);
    const int32_t v[SHL_PWDW_LAUNCH_FIELDS] = {r.kind, r.nsw, r.ks, r.tpw, r.tiles};
    for (int i = 0; i < SHL_PWDW_LAUNCH_FIELDS; ++i) out[i] = v[i];
    return true;
}

// the early block: copies of what the kernel's prologue reads (PwDwEarlyArgs), from the two layers and the chosen geometry
static void fill_early(const ConvArgs &q, const ConvArgs &d, PwDwArgs &f)
{
    PwDwEarlyArgs &e = f.early;
    e.w_frag = q.w_frag, e.in = q.in;
    e.xg = f.xg, e.xg_log2 = f.xg_log2, e.spg = f.spg, e.spg_magic = f.spg_magic, e.tx_magic = f.tx_magic;
    e.tiles_x = f.tiles_x, e.tiles_y = f.tiles_y, e.nrect = f.nrect, e.nsub = f.nsub, e.nsw = f.nsw, e.mt = f.mt;
    // ceil(2^32 / tiles_y): exact for every ty < 65536 (pwdw_fusable admits tiles_y N <= 65535, and a grid's z extent is no larger); 0 stands for 2^32
    e.ty_magic = f.tiles_y > 1 ? (uint32_t)((((uint64_t)1 << 32) + f.tiles_y - 1) / f.tiles_y) : 0u;
    e.img_stride = f.img_stride;
    e.bh = f.bh, e.bw = f.bw, e.ex_lo = f.ex_lo, e.ey_lo = f.ey_lo, e.iwm = f.iwm, e.iwm_magic = f.iwm_magic;
    e.H = q.H, e.W = q.W, e.C = q.C;
    e.sh = d.sh, e.sw = d.sw, e.pt = d.pt, e.pl = d.pl;
    e.reserved = 0;
}

int launch_pwdw_fused(const ConvArgs &q, const ConvArgs &d, hipStream_t s)
{
    PwDwArgs f;
    f.pw = q;
    f.dw = d;
    if (!shapes_pair(q, d) || !choose_rect(q, d, f)) {
        set_error("pwdw_fused: the pair does not qualify");
        return SHL_MI355X_ENOTSUP;
    }
    fill_early(q, d, f);
    dim3 grid((unsigned)(q.Co >> 5), (unsigned)f.tiles_x, (unsigned)(f.tiles_y * d.N));
    if (f.xg) {
        const int rpg = 8 / f.xg;
        grid = dim3((unsigned)(8 * f.spg * ((f.nrect + rpg - 1) / rpg)), 1, 1);
    }
    size_t lds = (size_t)f.mt * f.ks * 4096 + dw_patch_bytes(f.late.npx);
    const PwDwForm form = choose_form(f);
    {
        static const char *pr = getenv("SHL_MI355X_PWDW_PRINT");  // "1": the geometry of every launch (tools/dev)
        if (pr && pr[0] == '1')
            fprintf(stderr, "pwdw_fused %d->%d @%dx%d s%d: %dx%d rects of %dx%d (+%d/+%d, +%d/+%d at the borders), npx %d, nwin %d, mt %d, ks %d, nsw %d, nsub %d, mwn %d, xg %d, grid %u, form %d (%d tiles)\n",
                    q.C, q.Co, d.H, d.W, d.sh, f.tiles_y, f.tiles_x, f.bh, f.bw, f.ey_lo, f.ey_hi, f.ex_lo, f.ex_hi, f.late.npx, f.nwin, f.mt, f.ks, f.nsw, f.nsub,
                    f.mwn, f.xg, grid.x * grid.y * grid.z, form.kind, form.tiles);
    }
#define SHL_PWDW2(NSWV, MAXT, EX)                                                                                    \
    do {                                                                                                       \
        static LdsOptIn opted_in;                                                                              \
        if (lds > 64 * 1024) lds_opt_in(opted_in, reinterpret_cast<const void *>(pwdw_fused_kernel<PWDW_MTW, NSWV, MAXT, EX>)); \
        hipLaunchKernelGGL((pwdw_fused_kernel<PWDW_MTW, NSWV, MAXT, EX>), grid, dim3(64 * f.nwaves), lds, s, f);               \
    } while (0)
    // every wave with exactly NSWV sub-steps: the guard-free instantiation
#define SHL_PWDW(NSWV, MAXT)                                           \
    do {                                                              \
        if (f.nsw == NSWV && f.nsub == f.ks * NSWV) SHL_PWDW2(NSWV, MAXT, true); \
        else SHL_PWDW2(NSWV, MAXT, false);                            \
    } while (0)
    // the fully specialised forms: four waves, every wave exactly NSWV sub-steps and TPWV tiles, K split KSV (choose_form;
    // MobileNetV1 at batch 1: nine of its twelve pairs on the forms with exactly TPWV 4 / KSV tiles, the other three -- 5, 3 and
    // 3 tiles -- on the NT forms)
    // ... with both layers' epilogues compiled in for the two flavours whole models come in: clamp epilogues with power-of-two
    // output scales (3) and with general scales (0)
    const int epq = (q.act != SHL_MI355X_ACT_NONE && !q.act_clamp) ? -1 : (q.div_exact ? 3 : 0);
    const int epd = (d.act != SHL_MI355X_ACT_NONE && !d.act_clamp) ? -1 : (d.div_exact ? 3 : 0);
#define SHL_PWDW_EPI(KERNEL, ...)                                                                  \
    do {                                                                                           \
        if (epq == 3 && epd == 3)                                                                  \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__, 3, 3>), grid, dim3(256), lds, s, f);           \
        else if (epq == 0 && epd == 0)                                                             \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__, 0, 0>), grid, dim3(256), lds, s, f);           \
        else                                                                                       \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__>), grid, dim3(256), lds, s, f);                 \
        SHL_HIP(hipGetLastError());                                                                \
        return SHL_MI355X_OK;                                                                      \
    } while (0)
#define SHL_PWDW_FIXED(NSWV, KSV, TPWV)                                                            \
    if (form.kind != SHL_MI355X_PWDW_LAUNCH_NT && form.nsw == NSWV && form.ks == KSV && form.tpw == TPWV) { \
        if (form.kind == SHL_MI355X_PWDW_LAUNCH_FIXED_EXACT)                                       \
            SHL_PWDW_EPI(pwdw_fused_kernel, TPWV, NSWV, 512, true, KSV, TPWV, true);               \
        else                                                                                       \
            SHL_PWDW_EPI(pwdw_fused_kernel, TPWV, NSWV, 512, true, KSV, TPWV, false);              \
    }
#define SHL_PWDW_NT(NSWV, KSV, NTV)                                                                \
    if (form.kind == SHL_MI355X_PWDW_LAUNCH_NT && form.nsw == NSWV && form.ks == KSV && form.tiles == NTV) \
        SHL_PWDW_EPI(pwdw_fused_nt_kernel, NSWV, KSV, NTV);
    if (form.kind != SHL_MI355X_PWDW_LAUNCH_RUNTIME) {
        lds = form.lds;
        SHL_PWDW_NT(1, 1, 5)
        SHL_PWDW_NT(2, 1, 3)
        SHL_PWDW_NT(2, 2, 3)
        SHL_PWDW_FIXED(4, 4, 2)
        SHL_PWDW_FIXED(4, 4, 1)
        SHL_PWDW_FIXED(2, 4, 2)
        SHL_PWDW_FIXED(2, 4, 1)
        SHL_PWDW_FIXED(2, 2, 2)
        SHL_PWDW_FIXED(2, 2, 1)
        SHL_PWDW_FIXED(2, 1, 1)
        SHL_PWDW_FIXED(2, 1, 2)
        SHL_PWDW_FIXED(1, 1, 1)
        SHL_PWDW_FIXED(1, 1, 2)
        set_error("pwdw_fused: choose_form names a form that is not instantiated");  // (its tables and the lists above differ)
        return SHL_MI355X_ENOTSUP;
    }
#undef SHL_PWDW_NT
#undef SHL_PWDW_FIXED
#undef SHL_PWDW_EPI
    if (f.nsw <= 2)
        SHL_PWDW(2, 512);
    else if (f.nsw <= 4)
        SHL_PWDW(4, 512);
    else
        SHL_PWDW(8, 256);
#undef SHL_PWDW
#undef SHL_PWDW2
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

}  // namespace shl

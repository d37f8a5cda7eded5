// conv_group_mfma_f16.hip -- grouped (not depthwise) binary16 convolution on the matrix cores, over an LDS patch, on the NHWC view.
//
// The binary16 twin of conv_group_mfma.hip, and a design of its own: the int8 kernel packs 8 / 4 / 2 narrow groups onto the
// diagonal of one 32 x 32 weight matrix, whose off-diagonal zeros multiply other groups' inputs -- exact in int32, but in
// binary16 0 x inf and 0 x NaN are NaN, and one non-finite activation would poison every group of its slab.  Here a matrix
// block never spans two groups:
//
//   block      the M = 16 of one v_mfma_f32_16x16x32_f16: output channels of ONE group (all 4 / 8 / 16 of a narrow group, rows
//              past them padding that is never stored; 16 of a wide group's).  N = 16 output pixels, a tile 8 wide x 2 high.
//   K          32 halves.  Narrow groups: 32 / (C/G) taps x the C/G channels of the block's group -- a lane's 8 halves of B are
//              half a tap (C/G = 16), one tap (8: one ds_read_b128) or two taps (4: two ds_read_b64); which tap is a per-lane
//              offset read from a 64-entry table in LDS.  K positions past the last tap are zero in BOTH operands (a select on
//              the B side, so that 0 x inf cannot arise there either).  Wide groups: one 32-channel slab of one tap.
//   unit       (plan time, group_mfma_f16.h) the 8 / 4 / 2 narrow groups of one 32-channel window, or 4 / 2 blocks of one wide
//              group over the group's own channels.
//   weights    packed once as A fragments [block][slab][step][lane][16 B]: a wave fetches a step's fragment with one coalesced
//              1 KiB load, one step ahead of its use.  They never touch LDS.
//   workgroup  four waves: one unit x one rectangle of output pixels (btx x bty tiles) of one image.  Per K slab the rectangle's
//              input patch with its halo is staged once, [patch pixel][64 B + 16], pixels outside the image as +0 (the reference
//              skips them; +0 adds nothing).  The NEXT slab's patch is requested into registers before this slab's MFMAs and
//              stored behind them, between two barriers.
//   wave       one block (4-wide groups: two, one after the other over the same patch) x up to EIGHT pixel tiles (4 / nblk
//              waves deal a block's tiles out), one four-register accumulator per tile live across the K loop: a weight
//              fragment serves up to eight MFMAs.
//   store      finish_f16 (bias, relu / relu6, the reference's rounding) on the fp32 sums, 4 channels = 8 bytes per lane, masked
//              at the map's edge and at the block's padding rows.
//
// The layer arrives NCHW; conv_plan.hip runs the re-layout pass of the implicit-GEMM families in front and behind (element
// size 2), into scratch of the plan.  Sums run in fp32 in the MFMA's order, not the reference's ky -> kx -> ic: results differ
// from conv_group_direct_f16 by summation order only (gate 1e-3 relative).
// LDS: at most 48 KiB (group_mfma_f16.h, with the pitch argument).  Registers and measurements: profiles/group_mfma_f16_notes.md;
// build.py's NO_SPILL_SOURCES holds the kernel free of spills.
// Restates shl_ref_group_conv2d_f32 inside the f16 wrappers (source/reference/convolution.c:271-354) + relu variants for NCHW.
#include <stdlib.h>

#include "common.h"
#include "group_mfma_f16.h"

namespace shl {

typedef float v4f __attribute__((ext_vector_type(4)));

// kFour: 4-wide groups (two taps per lane, two blocks per wave); kMulti: more than one K slab -- the next slab's patch waits in
// GH_PREFETCH registers per thread under the MFMAs; a single slab (every narrow group) stages through GH_STAGE registers that
// are dead before the first MFMA, and affords a larger patch
template <bool kFour, bool kMulti>
__global__ __launch_bounds__(256, 2) void conv_group_mfma_f16_kernel(ConvArgs a, GhGeom g)
{
    constexpr int NPF = kMulti ? GH_PREFETCH : GH_STAGE;
    constexpr int NT = GH_TILES_PER_WAVE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, kq = lane >> 4;
    const int u = blockIdx.x;  // unit
    const int tx = blockIdx.y;
    int ty = blockIdx.z, n = 0;
    if (a.N > 1) {
        n = ty / g.tiles_y;
        ty -= n * g.tiles_y;
    }
    const int ox0 = tx * g.btx * 8, oy0 = ty * g.bty * 2;
    const int ix0 = ox0 * a.sw - a.pl, iy0 = oy0 * a.sh - a.pt;  // patch origin in the image
    const char *img = static_cast<const char *>(a.in) + ((int64_t)n * a.H * a.W * a.C + (u / g.upg) * g.kc) * 2;
    const int npix = g.pw * g.ph;
    int *tapoff = reinterpret_cast<int *>(smem + g.ph * g.row_pitch);  // tap -> byte offset in the patch, -1 past the last tap
    if (tid < GH_TAP_SLOTS) {
        const int ky = tid / g.kw, kx = tid - ky * g.kw;
        tapoff[tid] = tid < g.ntaps ? ky * g.row_pitch + kx * GH_PIX_BYTES : -1;
    }

    // ---- a slab's patch: HBM -> registers (fetch), registers -> LDS (commit); piece = (patch pixel, 16-byte quarter)
    uint4 pf[NPF];
    auto fetch = [&](int s) {
#pragma unroll
        for (int k = 0; k < NPF; ++k) {
            if (k * 256 >= g.nslots) break;  // uniform
            const int slot = k * 256 + tid;
            const int pix = slot >> 2;
            const int pr = (int)__umulhi((uint32_t)pix, g.pw_magic);
            const int pc = pix - pr * g.pw;
            const int y = iy0 + pr, x = ix0 + pc;
            pf[k] = make_uint4(0u, 0u, 0u, 0u);
            if (pix < npix && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W)  // (an image is below 2^31 bytes: the pick)
                pf[k] = *reinterpret_cast<const uint4 *>(img + (y * a.W + x) * a.C * 2 + s * 64 + (slot & 3) * 16);
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int k = 0; k < NPF; ++k) {
            if (k * 256 >= g.nslots) break;
            const int slot = k * 256 + tid;
            const int pix = slot >> 2;
            const int pr = (int)__umulhi((uint32_t)pix, g.pw_magic);
            const int pc = pix - pr * g.pw;
            if (pix < npix) *reinterpret_cast<uint4 *>(smem + pr * g.row_pitch + pc * GH_PIX_BYTES + (slot & 3) * 16) = pf[k];
        }
    };
    fetch(0);
    commit();
    __syncthreads();

    // ---- this wave's blocks and its tiles
    const int blk0 = g.nblk >= 4 ? wave * g.bpw : wave & (g.nblk - 1);
    const int stream = g.nblk >= 4 ? 0 : wave / g.nblk;
    const int nstream = g.nblk >= 4 ? 1 : 4 / g.nblk;
    const int ntile = g.btx * g.bty;
    const int nmine = stream < ntile ? (ntile - stream + nstream - 1) / nstream : 0;  // wave-uniform, <= NT (group_mfma_f16.h)
    const int px = col & 7, py = col >> 3;
    // the lane's place in K: which tap of a step and which channel bytes of the pixel (narrow groups add the block's group below)
    const int lpt = g.cpg ? (g.cpg >= 8 ? g.cpg / 8 : 1) : 4;  // lanes (K quarters) per tap
    const int sub = kFour ? 2 * kq : kq / lpt;                   // tap of the step (kFour: and sub + 1)
    const int lane_c = kFour ? 0 : (kq % lpt) * 16;
    int p0[NT];  // tap (0, 0) of the lane's pixel in each tile
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int t = stream + i * nstream;
        const int tby = g.btx == 2 ? t >> 1 : t, tbx = g.btx == 2 ? t & 1 : 0;
        p0[i] = ((tby * 2 + py) * a.sh) * g.row_pitch + ((tbx * 8 + px) * a.sw) * GH_PIX_BYTES + lane_c;
    }

    // every wave runs the slab loop with its barriers, also one without a tile (nmine = 0)
    for (int bi = 0; bi < (kMulti ? 1 : g.bpw); ++bi) {
        const int blk = blk0 + bi;
        const int64_t gb = (int64_t)u * g.nblk + blk;                       // the block among all blocks of the layer
        const int oc0 = g.cpg ? (int)gb * g.cpg : (int)gb * 16;             // its first output channel
        const int grp_c = g.cpg ? blk * g.cpg * 2 : 0;                      // narrow: the group's channel bytes in the window
        const char *wf = static_cast<const char *>(a.w) + gb * g.nslab * g.spslab * 1024 + lane * 16;
        v4f acc[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[i] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        for (int s = 0; s < (kMulti ? g.nslab : 1); ++s) {
            const bool more = kMulti && s + 1 < g.nslab;
            if (more) fetch(s + 1);  // in flight under this slab's MFMAs
            if (nmine > 0) {
                const char *wp = wf + (int64_t)s * g.spslab * 1024;
                v8h fa = *reinterpret_cast<const v8h *>(wp);
                for (int j = 0; j < g.spslab; ++j) {
                    v8h fan = fa;  // the next step's fragment, requested in front of this step's MFMAs
                    if (j + 1 < g.spslab) fan = *reinterpret_cast<const v8h *>(wp + (j + 1) * 1024);
                    uint4 fb[NT];
                    if constexpr (kFour) {
                        const int2 to = *reinterpret_cast<const int2 *>(tapoff + j * 8 + sub);
                        const int o0 = (to.x < 0 ? 0 : to.x) + grp_c, o1 = (to.y < 0 ? 0 : to.y) + grp_c;
#pragma unroll
                        for (int i = 0; i < NT; ++i)
                            if (i < nmine) {
                                const uint2 lo = *reinterpret_cast<const uint2 *>(smem + p0[i] + o0);
                                const uint2 hi = *reinterpret_cast<const uint2 *>(smem + p0[i] + o1);
                                fb[i] = make_uint4(to.x < 0 ? 0u : lo.x, to.x < 0 ? 0u : lo.y, to.y < 0 ? 0u : hi.x, to.y < 0 ? 0u : hi.y);
                            }
                    } else {
                        const int to = tapoff[j * g.tpm + sub];
                        const int o = (to < 0 ? 0 : to) + grp_c;
#pragma unroll
                        for (int i = 0; i < NT; ++i)
                            if (i < nmine) {
                                fb[i] = *reinterpret_cast<const uint4 *>(smem + p0[i] + o);
                                if (to < 0) fb[i] = make_uint4(0u, 0u, 0u, 0u);
                            }
                    }
#pragma unroll
                    for (int i = 0; i < NT; ++i)
                        if (i < nmine) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, __builtin_bit_cast(v8h, fb[i]), acc[i], 0, 0, 0);
                    fa = fan;
                }
            }
            if (more) {
                __syncthreads();  // every wave is done with this slab's patch
                commit();
                __syncthreads();
            }
        }
        // C layout: lane = (pixel column lane & 15, rows 4 (lane >> 4) .. + 3)
        if (4 * kq < g.mvalid) {
            const float4 bi4 = *reinterpret_cast<const float4 *>(a.bias + oc0 + 4 * kq);
            char *outp = static_cast<char *>(a.out) + (oc0 + 4 * kq) * 2;
#pragma unroll
            for (int i = 0; i < NT; ++i)
                if (i < nmine) {
                    const int t = stream + i * nstream;
                    const int tby = g.btx == 2 ? t >> 1 : t, tbx = g.btx == 2 ? t & 1 : 0;
                    const int oy = oy0 + tby * 2 + py, ox = ox0 + tbx * 8 + px;
                    uint2 v;
                    v.x = (uint32_t)finish_f16(acc[i][0], bi4.x, a) | (uint32_t)finish_f16(acc[i][1], bi4.y, a) << 16;
                    v.y = (uint32_t)finish_f16(acc[i][2], bi4.z, a) | (uint32_t)finish_f16(acc[i][3], bi4.w, a) << 16;
                    if (oy < a.Ho && ox < a.Wo) *reinterpret_cast<uint2 *>(outp + (((int64_t)n * a.Ho + oy) * a.Wo + ox) * a.Co * 2) = v;
                }
        }
    }
}

// binary16 and NCHW are the caller's business (conv_plan.hip:group_mfma_f16_takes); this is the scope of the geometry and, when
// by_rule, the measured default rule (group_mfma_f16.h).  The switch SHL_MI355X_GROUPMFMA_F16 is read by the plan, per plan;
// the launch asks with by_rule = false.  N: the plan's batch.
bool conv_group_mfma_f16_pick(int N, int C, int Co, int G, int H, int W, int Ho, int Wo, int Kh, int Kw, int sh, int sw, int dh, int dw, bool by_rule)
{
    if (dh != 1 || dw != 1 || N < 1 || H < 1 || W < 1) return false;
    const int64_t M = (int64_t)N * Ho * Wo;
    if (M <= 0 || M >= ((int64_t)1 << 31) || (int64_t)H * W * C * 2 >= ((int64_t)1 << 31)) return false;
    GhGeom g;
    if (!gh_geometry(C, Co, G, Kh, Kw, sh, sw, Ho, Wo, N, g)) return false;
    return !by_rule || gh_default(M, C, Co, G, Kh * Kw, sh > 1 || sw > 1);
}

size_t conv_group_mfma_f16_weight_bytes(int C, int Co, int G, int Kh, int Kw)
{
    GhGeom g;
    return gh_units(C, Co, G, Kh * Kw, g) ? (size_t)gh_weight_bytes(g) : 0;
}

void conv_group_mfma_f16_pack(const uint16_t *oihw, int C, int Co, int G, int Kh, int Kw, uint16_t *dst)
{
    GhGeom g;
    if (gh_units(C, Co, G, Kh * Kw, g)) gh_pack(oihw, C, Co, G, Kh, Kw, g, dst);
}

// a: the NHWC view (conv_plan.hip's re-layout scratch on both sides), a.w the fragment-ordered weights
int launch_conv_group_mfma_f16(const ConvArgs &a, hipStream_t s)
{
    GhGeom g;
    if (a.dh != 1 || a.dw != 1 || !gh_geometry(a.C, a.Co, a.group, a.Kh, a.Kw, a.sh, a.sw, a.Ho, a.Wo, a.N, g)) {
        set_error("conv_group_mfma_f16: group widths, kernel size, stride or grid out of range");
        return SHL_MI355X_ENOTSUP;
    }
    const dim3 grid((unsigned)g.nunits, (unsigned)g.tiles_x, (unsigned)(g.tiles_y * a.N));
    const size_t lds = (size_t)gh_lds_bytes(g);
    if (g.cpg == 4) hipLaunchKernelGGL((conv_group_mfma_f16_kernel<true, false>), grid, dim3(256), lds, s, a, g);
    else if (g.nslab > 1) hipLaunchKernelGGL((conv_group_mfma_f16_kernel<false, true>), grid, dim3(256), lds, s, a, g);
    else hipLaunchKernelGGL((conv_group_mfma_f16_kernel<false, false>), grid, dim3(256), lds, s, a, g);
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

}  // namespace shl

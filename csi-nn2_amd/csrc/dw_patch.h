// dw_patch.h -- depthwise 3x3 (int8, 32 channels) from an int8 patch [pixel][32 B] in LDS: the second
// phase of the latency-form fused kernels (pwdw_fused.hip, stemdw_fused.hip).
//
// Patch layout (round 6): eight PLANES of dwords, plane g = channels 4 g .. 4 g + 3 of every patch pixel j = r * rw + c, `pitch`
// dwords apart (a multiple of 32, + 8).  The producer's stores (32 consecutive pixels of one group) are consecutive dwords; a
// reader's nine taps are three row bases + the immediate offsets 0 / 4 / 8 bytes (x sw).  It replaced [pixel][8 dwords] with the
// dword index XOR-swizzled by the pixel: conflict-free both ways, but six address instructions per tap -- 54 of the depthwise
// phase's ~95 instructions per thread, in kernels whose duration is one wave's instruction count (profiles/r06_notes.md); the
// two-way bank conflicts of this layout cost a few cycles on nine reads.  Patch pixels OUTSIDE the image hold the depthwise
// layer's input zero point (the producer writes it): the reader tests nothing.
#pragma once

#include <stddef.h>

#include "common.h"

namespace shl {

// where the producer phase must put channel group `group` (0..7) of patch pixel j
__device__ __forceinline__ int dw_patch_slot(int j, int group, int pitch) { return group * pitch + j; }
// plane pitch in dwords for a patch of npx pixels, and the bytes of the whole patch
__host__ __device__ __forceinline__ int dw_patch_pitch(int npx) { return ((npx + 31) & ~31) + 8; }
__host__ __device__ __forceinline__ size_t dw_patch_bytes(int npx) { return (size_t)dw_patch_pitch(npx) * 32; }
// what the producer stores for a patch pixel outside the image
__device__ __forceinline__ uint32_t dw_patch_pad(const ConvArgs &d) { return (uint32_t)(d.in_zp & 0xff) * 0x01010101u; }

// A kernel argument (or a whole argument struct: only the fields that are used are fetched) read at THIS point of the program:
// the pointer to the argument segment passes through an empty asm, so the scalar loads depend on it and cannot be hoisted above
// it -- arguments read the plain way are fetched wherever the compiler likes, in front of the first branch or behind the last
// barrier.  `off`: byte offset in the kernel-argument segment (the explicit arguments come first, naturally aligned).
template <class T>
__device__ __forceinline__ T kernarg_here(size_t off)
{
    typedef const __attribute__((address_space(4))) char *KernargPtr;
    KernargPtr p = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    T v;
    __builtin_memcpy(&v, (const __attribute__((address_space(4))) T *)(p + off), sizeof(T));
    return v;
}

struct DwPatchGeom {
    int bh, bw;         // output rectangle the threads decompose their output index by (the launch's largest)
    int lbh, lbw;       // the part of THIS workgroup's rectangle that lies in the output map (<= bh, bw): rectangles of a launch
                        // may differ (pwdw_fused.hip: wider border rectangles) and the last ones may stick out of the map
    int rw;             // patch width in pixels
    int pitch;          // plane pitch in dwords (dw_patch_pitch)
    uint32_t bw_magic;  // po / bw == (po * bw_magic) >> 20 for po < 4096
    int oy0, ox0;       // first output pixel of the rectangle
    int ry0, rx0;       // patch origin in the depthwise layer's input image (may be negative: padding)
    int n;              // image
    int ch0;            // first of the 32 channels in the output tensor
};

// A thread's 4 channels (group tid & 7 of the 32 starting at ch0) are the same for every output it
// computes: their dot4-packed weights and epilogue tables.  The callers request them right behind the producer phase's own
// global loads and keep them there (pwdw_fused.hip: scheduling fences around the window, no conditional exit behind it): the
// compiler otherwise sinks each load into the block of its first use -- behind the barriers, where its whole latency is exposed.
struct DwThreadConsts {
    uint4 w0, w1, w2;
    int4 ai;
    float4 mu, bi;
};

__device__ __forceinline__ DwThreadConsts dw_load_consts(const ConvArgs &d, int ch0, int tid)
{
    const int dc = ch0 + (tid & 7) * 4;
    const uint4 *dwp = reinterpret_cast<const uint4 *>(static_cast<const char *>(d.w) + (int64_t)dc * 12);
    DwThreadConsts k;
    k.w0 = dwp[0], k.w1 = dwp[1], k.w2 = dwp[2];
    k.ai = *reinterpret_cast<const int4 *>(d.acc_init + dc);
    k.mu = *reinterpret_cast<const float4 *>(d.mult + dc);
    k.bi = *reinterpret_cast<const float4 *>(d.bias + dc);
    return k;
}

// Where one output of a thread lives: everything below is index arithmetic on the thread id and the kernel's arguments -- no loaded data.
struct DwOutPos {
    uint32_t lds;  // dword index of tap (0, 0) in the patch: plane + (oyl sh) rw + oxl sw
    uint32_t out;  // byte offset of the thread's four channels inside the output image
    bool live;     // the output pixel exists (inside the workgroup's own rectangle and the map: DwPatchGeom::lbh, lbw)
};

// What the depthwise phase needs beside the patch and the constants, none of it dependent on loaded data: dw_patch_prepare.
struct DwPrep {
    int8_t *out_img;  // the output image (wave-uniform)
    int nout;         // outputs of the rectangle
    int po;           // the thread's first output
    DwOutPos first;   // ... and where it lives
};

__device__ __forceinline__ DwOutPos dw_patch_locate(const ConvArgs &d, const DwPatchGeom &g, int cg, int po)
{
    const int oyl = (int)(((uint32_t)po * g.bw_magic) >> 20);
    const int oxl = po - oyl * g.bw;
    const int oy = g.oy0 + oyl, ox = g.ox0 + oxl;
    DwOutPos p;
    p.lds = (uint32_t)(cg * g.pitch + (oyl * d.sh) * g.rw + oxl * d.sw);
    // (inside an image 32 bits address every byte: the callers admit images below 2 GiB)
    p.out = (uint32_t)((oy * d.Wo + ox) * d.C + g.ch0 + cg * 4);
    p.live = oyl < g.lbh && oxl < g.lbw;
    return p;
}

// The "prepare" half of the depthwise phase.  The callers run it in the shadow of the producer phase's global loads -- after the last
// of them has been issued, before the first wait for them -- where the wave would otherwise idle for a memory latency; left to the
// compiler, this arithmetic (the image base, a magic division, the plane and row bases, the output offset: ~60 instructions of a wave
// that issues one per ~5.8 cycles) and the kernel-argument fetches in front of it stand behind the last barrier, where nothing
// overlaps them.  The image base takes the n ? ... : 0 form: at batch 1 no 64-bit product.
// The result is pinned where it is computed (an empty asm "uses" it): the compiler otherwise sinks every piece into the block
// of its first use, i.e. back behind the barriers.
__device__ __forceinline__ DwPrep dw_patch_prepare(const ConvArgs &d, const DwPatchGeom &g, int tid)
{
    DwPrep p;
    p.out_img = static_cast<int8_t *>(d.out) + (g.n ? (int64_t)g.n * d.Ho * d.Wo * d.C : (int64_t)0);
    p.nout = g.bh * g.bw;
    p.po = tid >> 3;
    p.first = dw_patch_locate(d, g, tid & 7, p.po);
    const uint32_t live = p.first.live ? 1u : 0u;
    asm volatile("" ::"s"(p.out_img), "s"(p.nout), "v"(p.po), "v"(p.first.lds), "v"(p.first.out), "v"(live));
    p.first.live = live != 0;
    return p;
}

// The "run" half.  thread = (output pixel, 4 channels): nine dwords from the patch (the padding value for taps outside the
// image), byte transposes + v_dot4_i32_i8 against the plan's dot4-packed weights, requantise, one dword
// store.  `threads` = workgroup size (a multiple of 8).  The position of an output is computed one iteration ahead (the first: by
// dw_patch_prepare), so that no address arithmetic stands between the barrier and the first patch read.  Restates
// shl_ref_depthwise_conv2d_quant (source/reference/convolution.c:416-460) + relu variants.
template <int EPI = -1>  // the depthwise layer's epilogue flavour (common.h), -1: chosen at run time
__device__ __forceinline__ void depthwise_from_patch(const ConvArgs &d, const uint32_t *patch, const DwPatchGeom &g,
                                                     const DwThreadConsts &k, const DwPrep &prep, int tid, int threads)
{
    const int cg = tid & 7;
    const uint4 w0 = k.w0, w1 = k.w1, w2 = k.w2;
    const int4 d_ai = k.ai;
    const float4 d_mu = k.mu, d_bi = k.bi;
    const uint32_t wk[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
    const int nout = prep.nout;
    int8_t *const out_img = prep.out_img;
    DwOutPos pos = prep.first;
    for (int po = prep.po; po < nout;) {
        const DwOutPos cur = pos;
        if (cur.live) {
            uint32_t iv[9];
            const uint32_t *p00 = patch + cur.lds;  // tap (0, 0)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) iv[ky * 3 + kx] = p00[ky * g.rw + kx];
            const uint32_t r0[4] = {iv[0], iv[1], iv[2], iv[3]}, r1[4] = {iv[4], iv[5], iv[6], iv[7]};
            uint32_t t0[4], t1[4];
            transpose4x4_bytes(r0, t0);  // t0[ch] = taps 0..3 of channel ch
            transpose4x4_bytes(r1, t1);  // taps 4..7
            int a4[4] = {d_ai.x, d_ai.y, d_ai.z, d_ai.w};
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const uint32_t t2 = __builtin_amdgcn_ubfe(iv[8], 8 * ch, 8);  // tap 8 in byte 0, zeros above
                a4[ch] = __builtin_amdgcn_sdot4((int)t0[ch], (int)wk[3 * ch + 0], a4[ch], false);
                a4[ch] = __builtin_amdgcn_sdot4((int)t1[ch], (int)wk[3 * ch + 1], a4[ch], false);
                a4[ch] = __builtin_amdgcn_sdot4((int)t2, (int)wk[3 * ch + 2], a4[ch], false);
            }
            // (the image's base is wave-uniform 64-bit arithmetic on the scalar unit)
            *reinterpret_cast<uint32_t *>(out_img + cur.out) = requant4_i8_sel<EPI>(a4[0], a4[1], a4[2], a4[3], d_mu, d_bi, d);
        }
        po += threads >> 3;
        pos = dw_patch_locate(d, g, cg, po);  // the next output's position, behind the store (the last iteration computes one in vain)
    }
}

}  // namespace shl

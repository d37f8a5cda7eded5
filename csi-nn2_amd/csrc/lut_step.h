// lut_step.h -- the 256-entry table of an int8 activation (sigmoid / hard_sigmoid / silu / leaky_relu, and a swish or hard-swish
// gate: mul(x, act(x)) depends on x's byte alone), for the two places that look it up: the table kernels (eltwise.hip) and the
// stores of a convolution with the activation folded into its launch (conv_igemm.hip; dwconv.hip and dwconv_mfma.hip for a
// depthwise layer).  One definition of the table and of the
// lookup, so that the fused launch equals the layers by construction: its input is the byte the convolution's own
// requantisation produced -- folded relu / relu6 and saturation included.
#pragma once
#include <type_traits>

#include "common.h"
#include "residual_step.h"

namespace shl {

struct Lut256 {
    uint32_t w[64];  // entry of byte value b (as uint8_t) = byte b & 3 of w[b >> 2]
};

// four packed bytes through the table `lut` (256 bytes in LDS)
__device__ __forceinline__ uint32_t lut4(const uint8_t *lut, uint32_t v)
{
    const uint32_t b0 = lut[v & 0xFFu], b1 = lut[(v >> 8) & 0xFFu], b2 = lut[(v >> 16) & 0xFFu], b3 = lut[v >> 24];
    return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

// EPI of the implicit-GEMM kernels carries the table post-op as one more bit above EPI_RESIDUAL.  The two post-ops are not
// combined: no instantiation has both bits
constexpr int EPI_LUT = 16;

// the kernel argument of a fused launch: the convolution's own block and, behind it, the table BY VALUE (nothing to allocate or
// keep alive, capturable), as the table kernels take it
struct LutConvArgs : ConvArgs {
    Lut256 tab;
};
static_assert(sizeof(LutConvArgs) == sizeof(ConvArgs) + 256 && sizeof(ConvArgs) % 4 == 0, "the table sits behind the block");

template <int EPI>
struct IgemmArgs {
    static_assert((EPI & EPI_LUT) == 0 || (EPI & EPI_RESIDUAL) == 0, "a table post-op and a residual tail in one launch");
    using type = typename std::conditional<(EPI & EPI_LUT) != 0, LutConvArgs,
                                           typename std::conditional<(EPI & EPI_RESIDUAL) != 0, ResidualConvArgs, ConvArgs>::type>::type;
};

// The table of a kernel whose one argument is a LutConvArgs, copied where the epilogue begins from the kernel argument segment
// into the calling wave's own 256-byte slice `slice` of LDS: lane t takes dword t.  As fields of the by-value argument the 64
// dwords would be fetched at the kernel's entry and stay live across the K loop (residual_step.h:late_tail met that with 17).
// Call it with all 64 lanes active; the wave's own LDS wait orders the copy before its lookups, so no barrier is needed and
// no other wave's LDS is touched.  Returns the slice as the bytes lut4 indexes.
__device__ __forceinline__ const uint8_t *late_lut(uint32_t *slice)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) uint32_t *kernarg_words;
    kernarg_words kp = (kernarg_words)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));  // opaque from here on: the load below cannot move above this point
    slice[threadIdx.x & 63] = kp[sizeof(ConvArgs) / 4 + (threadIdx.x & 63)];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    return reinterpret_cast<const uint8_t *>(slice);
}

// conv_igemm.hip: the fused launch on one of the two families that carry the post-op ("wave" | "tile")
int launch_conv_igemm_lut(const LutConvArgs &a, const char *family, hipStream_t s);

// dwconv.hip, dwconv_mfma.hip: the fused launch of a depthwise plan (int8, NHWC, depth multiplier 1) on the kernel launch_dwconv
// picks for the same arguments, and which one that is (DW_LUT_* of lut_validate.h)
int launch_dwconv_lut(const LutConvArgs &a, hipStream_t s);
int launch_dwconv_mfma_lut(const LutConvArgs &a, hipStream_t s);
int dwconv_i8_kernel(const ConvArgs &a);

}  // namespace shl

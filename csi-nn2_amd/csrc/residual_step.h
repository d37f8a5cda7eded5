// residual_step.h -- the tail of a skip connection, conv2d -> add(conv_out, skip) -> [relu | relu6], applied inside the
// convolution's launch (conv_igemm.hip): the post-op record, the kernel argument that carries it and the function the stores
// call.  Its input is the byte the convolution's own requantisation produced -- folded activation and saturation included --
// and it runs the add's and the relu's element functions (add_step.h, relu_step.h) on it, so the launch equals the layers
// bit for bit for every record, zero point and scale.
#pragma once
#include <type_traits>

#include "add_step.h"
#include "relu_step.h"

namespace shl {

struct ResidualRec {
    AddRec add;          // the add layer's records, operands in the LAYER's order
    int32_t conv_first;  // the convolution's byte is the add's first operand (else its second)
    int32_t act;         // 0: the sum is the result, 1: relu behind it, 2: relu6
    ReluRec relu;        // the activation layer's input (= the sum's) and output records
};

// skip: scale / zero point of the other operand; sum: the add's output record; out: the activation's output record
static inline ResidualRec residual_rec(int conv_first, float conv_scale, int32_t conv_zp, float skip_scale, int32_t skip_zp,
                                       float sum_scale, int32_t sum_zp, int act, float out_scale, int32_t out_zp)
{
    ResidualRec r;
    r.add = conv_first ? add_rec(conv_scale, conv_zp, skip_scale, skip_zp, sum_scale, sum_zp)
                       : add_rec(skip_scale, skip_zp, conv_scale, conv_zp, sum_scale, sum_zp);
    r.conv_first = conv_first ? 1 : 0;
    r.act = act;
    r.relu = relu_rec(sum_scale, sum_zp, out_scale, out_zp, act == 2);
    return r;
}

// the kernel argument of a fused launch: the convolution's own block, the skip tensor (the output's shape and layout, so an
// output offset addresses it) and the record
struct ResidualTail {
    const void *skip;
    ResidualRec post;
};
struct ResidualConvArgs : ConvArgs {
    ResidualTail tail;
};
static_assert(sizeof(ResidualConvArgs) == sizeof(ConvArgs) + sizeof(ResidualTail) && sizeof(ConvArgs) % 8 == 0, "the tail sits behind the block");

// The tail of a kernel whose one argument is a ResidualConvArgs, read from the kernel argument segment where the epilogue
// begins: as fields of the by-value argument its seventeen scalars are fetched with the other arguments, at the kernel's
// entry, and stay live across the K loop -- the tile kernels, at the limit of their scalar registers there, spilled them
__device__ __forceinline__ ResidualTail late_tail(const ResidualConvArgs &a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) char *kernarg_ptr;
    kernarg_ptr kp = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));  // opaque from here on: the loads below cannot move above this point
    ResidualTail r;
    __builtin_memcpy(&r, kp + sizeof(ConvArgs), sizeof(r));
    return r;
#else
    return a.tail;  // (the host pass only parses this)
#endif
}

// EPI of the implicit-GEMM kernels carries the post-op as one more bit above the requantisation's code (common.h:epi_code):
// the instantiations without it are the ones there were.  (lut_step.h adds one more bit and holds IgemmArgs<EPI>, which picks
// the kernel's argument type from the two.)
constexpr int EPI_RESIDUAL = 8;

// four outputs at once: the bytes requant4_i8_* packed, the four skip bytes of the same offsets
__device__ __forceinline__ uint32_t residual4_i8(uint32_t conv4, uint32_t skip4, const ResidualRec &m)
{
    uint32_t r = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int qc = (int8_t)(conv4 >> (8 * e)), qs = (int8_t)(skip4 >> (8 * e));
        int q = add_i8_step(m.conv_first ? qc : qs, m.conv_first ? qs : qc, m.add);
        if (m.act) q = relu_i8_step(q, m.relu);
        r |= (uint32_t)(q & 0xFF) << (8 * e);
    }
    return r;
}

// binary16: the four halves finish4_f16 produced (the convolution's folded relu / relu6 and its rounding included) and the four
// skip halves of the same offsets, through the same-shape add's and the relu's element functions (add_step.h:add_same_f16_step --
// not the broadcasting add's --, relu_step.h:relu_f16_step).  The records are not read: a binary16 tensor of a fused tail has
// scale 1.  conv_first is not decorative here: the hardware's addition picks between two NaNs by operand position, so the
// operands go in the LAYER's order
__device__ __forceinline__ uint2 residual4_f16(uint2 conv4, uint2 skip4, int conv_first, int act)
{
    const uint32_t c[4] = {conv4.x & 0xFFFFu, conv4.x >> 16, conv4.y & 0xFFFFu, conv4.y >> 16};
    const uint32_t k[4] = {skip4.x & 0xFFFFu, skip4.x >> 16, skip4.y & 0xFFFFu, skip4.y >> 16};
    uint32_t h[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint16_t v = add_same_f16_step((uint16_t)(conv_first ? c[e] : k[e]), (uint16_t)(conv_first ? k[e] : c[e]));
        if (act) v = relu_f16_step(v, act == 2);
        h[e] = v;
    }
    return make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
}

// conv_igemm.hip: the fused launch on one of the two families that carry the post-op ("wave" | "tile"), and the size rule
// that picks between them (igemm_variant's, without the A/B switches of the unfused launch).  _f16: a binary16 problem, of
// whose tail only conv_first and act are read
int launch_conv_igemm_residual(const ResidualConvArgs &a, const char *family, hipStream_t s);
int launch_conv_igemm_residual_f16(const ResidualConvArgs &a, const char *family, hipStream_t s);
const char *igemm_size_rule(int64_t M, int64_t Co, int64_t kbytes);

}  // namespace shl

// shuffle.hip -- shuffle_channel of an int8 / binary16 tensor (CSINN_OP_SHUFFLE_CHANNEL): the end of every ShuffleNet unit.
//
// Restates shl_ref_shuffle_channel_quant (source/reference/shuffle_channel.c): the input is converted to float32, the
// channels are permuted -- with gc = C / group, out[.., j * group + k] = in[.., k * gc + j] for j < gc, k < group -- and the
// result is converted with the output's record.  NHWC permutes inside every pixel; NCHW goes through two transposes in the
// reference, which is the same permutation of whole planes.  The common view is [outer][C][inner] (NHWC: outer = N H W,
// inner = 1; NCHW: outer = N, inner = H W).  Per element (requant_move.h):
//   int8      q_out = sat8(rint(((q - zp_in) * s_in) / s_out) + zp_out); a byte copy when the records are equal and the
//             round trip was checked to be the identity on all 256 values (requant_is_identity, pool2d.hip)
//   binary16  float32_to_float16_base(float16_to_float32_base(h))
// Nothing is summed: results are bit-identical to the reference for any records.
//
// Arguments travel by value, calls enqueue only.  Three forms, chosen by shuffle_form() below, which also names them:
//   plane     inner in bytes a multiple of 16 (W = 16 bytes per thread) or of 4 (W = 4): pieces of a plane are copied plane
//             to plane, indexed in OUTPUT order -- stores fully coalesced, loads coalesced within a plane.
//   pixel     inner == 1 and C in bytes a multiple of 16 or of 4, at most PIXEL_LDS_BYTES: a workgroup takes a run of
//             consecutive pixels -- one contiguous stretch of memory, as much as its 256 lanes move in one pass, at least
//             one pixel --, loads it coalesced into LDS, W bytes per lane, and
//             every lane then assembles W output bytes from LDS in permuted order (byte / half reads; walking k, j instead
//             of dividing per element) and stores them coalesced.  ShuffleNetV2's 116 / 232 / 464 int8 channels are
//             multiples of 4, not of 16: they take W = 4.
//   generic   one element per thread, any shape and alignment: the literal formula.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "requant_move.h"

namespace shl {

enum { SHUFFLE_PLANE = 0, SHUFFLE_PIXEL = 1, SHUFFLE_GENERIC = 2 };

constexpr int PIXEL_LDS_BYTES = 8192;  // the tile: the longest pixel the pixel form takes

struct ShuffleArgs {
    const void *in;
    void *out;
    int64_t outer, c, inner;  // inner: in pieces of W bytes (plane), elements (generic); unused (pixel)
    int64_t items;            // threads that have work (plane, generic)
    int32_t group, gc;
    int32_t row_bytes;  // pixel: C in bytes
    int32_t run;        // pixel: pixels per workgroup
    MoveRec rec;
    int32_t small;  // the tensor has fewer than 2^32 elements: every index fits 32 bits
};

// the input plane that output plane `plane` = (image, output channel) shows
__device__ __forceinline__ int64_t shuffle_source(int64_t plane, const ShuffleArgs &a)
{
    int64_t oc, k;
    const int64_t n = move_divmod(plane, a.c, a.small != 0, oc);
    const int64_t j = move_divmod(oc, a.group, a.small != 0, k);
    return n * a.c + k * a.gc + j;
}

template <typename W, bool F16>
__global__ __launch_bounds__(256) void shuffle_plane_kernel(ShuffleArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (image, output plane, piece), piece fastest
    if (i >= a.items) return;
    int64_t piece;
    const int64_t plane = move_divmod(i, a.inner, a.small != 0, piece);
    const W v = static_cast<const W *>(a.in)[shuffle_source(plane, a) * a.inner + piece];
    static_cast<W *>(a.out)[i] = move_piece<W, F16>(v, a.rec);
}

template <typename W, bool F16>
__global__ __launch_bounds__(256) void shuffle_pixel_kernel(ShuffleArgs a)
{
    __shared__ W tile[PIXEL_LDS_BYTES / sizeof(W)];
    using E = typename std::conditional<F16, uint16_t, uint8_t>::type;
    constexpr int PER = sizeof(W) / sizeof(E);  // elements a lane assembles
    const int64_t first = (int64_t)blockIdx.x * a.run;  // first pixel of this workgroup's run
    const int64_t left = a.outer - first;
    const int pixels = left < a.run ? (int)left : a.run;
    const int pieces = pixels * a.row_bytes / (int)sizeof(W);  // <= PIXEL_LDS_BYTES / sizeof(W)
    const int64_t at = first * a.row_bytes / (int)sizeof(W);  // the run is one contiguous stretch of both tensors
    const W *src = static_cast<const W *>(a.in) + at;
    W *dst = static_cast<W *>(a.out) + at;
    for (int t = threadIdx.x; t < pieces; t += 256) tile[t] = src[t];
    __syncthreads();
    const E *bytes = reinterpret_cast<const E *>(tile);
    const int row = a.row_bytes / (int)sizeof(E);  // C
    for (int t = threadIdx.x; t < pieces; t += 256) {
        const int e0 = t * PER;                // first output element of this piece, inside the run
        const int pix = e0 / row, oc = e0 - pix * row;  // a piece never straddles two pixels: C in bytes % sizeof(W) == 0
        int j = oc / a.group, k = oc - j * a.group;
        const E *px = bytes + pix * row;
        uint32_t w[sizeof(W) / 4];
#pragma unroll
        for (int q = 0; q < (int)(sizeof(W) / 4); ++q) {
            uint32_t word = 0;
#pragma unroll
            for (int b = 0; b < 4 / (int)sizeof(E); ++b) {
                word |= (uint32_t)px[k * a.gc + j] << (8 * (int)sizeof(E) * b);
                if (++k == a.group) k = 0, ++j;
            }
            w[q] = move_word<F16>(word, a.rec);
        }
        W v;
        if constexpr (sizeof(W) == 16) v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
        else v = w[0];
        dst[t] = v;
    }
}

template <bool F16>
__global__ __launch_bounds__(256) void shuffle_generic_kernel(ShuffleArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (image, output channel, inner element), element fastest
    if (i >= a.items) return;
    int64_t e;
    const int64_t plane = move_divmod(i, a.inner, a.small != 0, e);
    const int64_t src = shuffle_source(plane, a) * a.inner + e;
    if constexpr (F16) {
        static_cast<uint16_t *>(a.out)[i] = float_to_f16_bits_ref(f16_bits_to_float(static_cast<const uint16_t *>(a.in)[src]));
    } else {
        static_cast<int8_t *>(a.out)[i] = (int8_t)move_rq<false>(static_cast<const int8_t *>(a.in)[src], a.rec);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------
// NULL when the arguments describe a shuffle_channel, else what is wrong with them; *elems: elements of the tensor
static const char *shuffle_invalid(const void *in_dev, const void *out_dev, const shl_mi355x_shuffle_desc *d, int64_t *elems)
{
    if (!d || !in_dev || !out_dev) return "NULL argument";
    if (d->dtype != SHL_MI355X_I8 && d->dtype != SHL_MI355X_F16) return "dtype is neither int8 nor binary16";
    if (d->outer < 0 || d->c < 1 || d->inner < 1) return "outer < 0, c < 1 or inner < 1";
    if (d->group < 1) return "group < 1";
    if (d->c % d->group != 0) return "c is no multiple of group";
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    int64_t n, bytes;
    if (__builtin_mul_overflow(d->outer, d->c, &n) || __builtin_mul_overflow(n, d->inner, &n) ||
        __builtin_mul_overflow(n, es, &bytes))
        return "tensor too large";
    if (ranges_overlap(in_dev, bytes, out_dev, bytes)) return "the output overlaps the input";
    *elems = n;
    return NULL;
}

// The one place that chooses the form and its width in bytes (launch and name).  SHL_MI355X_SHUFFLE_FORM=generic | plane |
// pixel forces a form (A/B runs, tests); one the arguments do not admit gives generic; read per call.
static int shuffle_form(const void *in_dev, const void *out_dev, const shl_mi355x_shuffle_desc *d, int *width)
{
    const char *force = getenv("SHL_MI355X_SHUFFLE_FORM");
    const bool only_plane = force && strcmp(force, "plane") == 0, only_pixel = force && strcmp(force, "pixel") == 0;
    const bool want_plane = !only_pixel, want_pixel = !only_plane;  // (an unknown value means nothing, as for concat)
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    const uintptr_t both = (uintptr_t)in_dev | (uintptr_t)out_dev;
    *width = 1;
    if (force && strcmp(force, "generic") == 0) return SHUFFLE_GENERIC;
    // the unit every piece, plane / pixel and pointer must be a multiple of
    const int64_t unit = d->inner > 1 ? d->inner * es : d->c * es;
    const int w = unit % 16 == 0 && (both & 15) == 0 ? 16 : unit % 4 == 0 && (both & 3) == 0 ? 4 : 0;
    if (w == 0) return SHUFFLE_GENERIC;
    if (d->inner > 1) {
        if (!want_plane) return SHUFFLE_GENERIC;
        *width = w;
        return SHUFFLE_PLANE;
    }
    if (!want_pixel || d->c * es > PIXEL_LDS_BYTES || d->c > 0x7FFFFFFF) return SHUFFLE_GENERIC;
    *width = w;
    return SHUFFLE_PIXEL;
}

static const char *shuffle_name(int form, int width)
{
    if (form == SHUFFLE_PLANE) return width == 16 ? "shuffle_plane_16" : "shuffle_plane_4";
    if (form == SHUFFLE_PIXEL) return width == 16 ? "shuffle_pixel_16" : "shuffle_pixel_4";
    return "shuffle_generic";
}

}  // namespace shl

extern "C" const char *shl_mi355x_shuffle_channel_kernel_name(const void *in_dev, const void *out_dev,
                                                              const struct shl_mi355x_shuffle_desc *d)
{
    int64_t elems;
    if (shl::shuffle_invalid(in_dev, out_dev, d, &elems)) return "";
    int width;
    const int form = shl::shuffle_form(in_dev, out_dev, d, &width);
    return shl::shuffle_name(form, width);
}

extern "C" int shl_mi355x_shuffle_channel(const void *in_dev, void *out_dev, const struct shl_mi355x_shuffle_desc *d, void *stream)
{
    using namespace shl;
    int64_t elems;
    const char *why = shuffle_invalid(in_dev, out_dev, d, &elems);
    if (why) {
        set_error("shuffle_channel: %s", why);
        return SHL_MI355X_EINVAL;
    }
    if (elems == 0) return SHL_MI355X_OK;
    const bool f16 = d->dtype == SHL_MI355X_F16;
    const int64_t es = f16 ? 2 : 1;
    int width;
    const int form = shuffle_form(in_dev, out_dev, d, &width);
    ShuffleArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in_dev, a.out = out_dev;
    a.outer = d->outer, a.c = d->c;
    a.group = d->group, a.gc = (int32_t)(d->c / d->group);
    a.rec = move_rec(d->in_scale, d->in_zp, d->out_scale, d->out_zp, !f16 && form != SHUFFLE_GENERIC);
    a.small = elems < (1ll << 32);
    int64_t groups;
    if (form == SHUFFLE_PIXEL) {
        a.row_bytes = (int32_t)(d->c * es);
        // a run is what the workgroup moves in ONE pass (256 lanes x `width` bytes): small tensors still spread over the
        // device, large ones have no lane walk the tile more than once.  A pixel longer than that is a run of its own,
        // walked in several passes (C in bytes <= PIXEL_LDS_BYTES: shuffle_form)
        const int pass = 256 * width / a.row_bytes;
        a.run = pass > 0 ? pass : 1;
        groups = (d->outer + a.run - 1) / a.run;
    } else {
        a.inner = form == SHUFFLE_PLANE ? d->inner * es / width : d->inner;
        a.items = d->outer * d->c * a.inner;
        groups = (a.items + 255) / 256;
    }
    if (grid_refused("shuffle_channel", groups)) return SHL_MI355X_ENOTSUP;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)groups), block(256);
    void (*kernel)(ShuffleArgs);  // (a template-id with a comma cannot be a macro argument)
    if (form == SHUFFLE_PLANE) {
        if (width == 16) kernel = f16 ? shuffle_plane_kernel<uint4, true> : shuffle_plane_kernel<uint4, false>;
        else kernel = f16 ? shuffle_plane_kernel<uint32_t, true> : shuffle_plane_kernel<uint32_t, false>;
    } else if (form == SHUFFLE_PIXEL) {
        if (width == 16) kernel = f16 ? shuffle_pixel_kernel<uint4, true> : shuffle_pixel_kernel<uint4, false>;
        else kernel = f16 ? shuffle_pixel_kernel<uint32_t, true> : shuffle_pixel_kernel<uint32_t, false>;
    } else {
        kernel = f16 ? shuffle_generic_kernel<true> : shuffle_generic_kernel<false>;
    }
    hipLaunchKernelGGL(kernel, grid, block, 0, s, a);
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

// transpose.hip -- transpose of an int8 / binary16 tensor of any rank up to 8 under any permutation (CSINN_OP_TRANSPOSE),
// and the flat requantised move that reshape and flatten are (CSINN_OP_RESHAPE, CSINN_OP_FLATTEN).
//
// Restates shl_ref_transpose behind shl_ref_siso_callback_base (source/reference/transpose.c:73-100): the input is
// converted to float32 with its record, out[o_0, .., o_r-1] = in[i], i[perm[k]] = o_k, and the float32 result is converted
// with the output's record.  Per element (requant_move.h):
//   int8      q_out = sat8(rint(((q - zp_in) * s_in) / s_out) + zp_out); a byte copy when the records are equal and the
//             round trip was checked to be the identity on all 256 values (requant_is_identity, pool2d.hip)
//   binary16  float32_to_float16_base(float16_to_float32_base(h))
// Nothing is summed: results are bit-identical to the reference for any records.
//
// The host canonicalises the layer (canonicalise() below): dims of extent 1 are dropped, and two dims that follow each
// other in the output and are contiguous in the input become one.  What is left is a list of dims in OUTPUT order, each
// with its extent and its stride in the input.  Arguments travel by value, calls enqueue only.  Four forms, chosen by
// canon_form() below, which also names them:
//   flat      one canonical dim: a flat move.  16 bytes per thread; the last thread finishes a tail of fewer than 16 bytes
//             element by element.  Needs both pointers 16-byte aligned.
//   rows      the innermost canonical dim is the input's innermost too, and a run of it is a multiple of 16 bytes (W = 16) or
//             of 4 (W = 4), pointers aligned alike: a thread moves one piece, indexed in output order -- stores fully
//             coalesced, loads coalesced within a run; the outer coordinates are taken apart with move_divmod.
//   tile      the output's innermost dim A is not the input's innermost dim B: a workgroup moves a 64 x 64-element tile of
//             the (A, B) plane through LDS -- global reads run along B (contiguous in the input), global writes along A
//             (contiguous in the output), so both sides are coalesced; every other dim is a batch coordinate taken from the
//             workgroup's index.  Extents are ragged (7 x 7 maps, 85-channel heads): every access is predicated on its
//             coordinates, no access leaves the tensor.
//             Widths, chosen per SIDE.  A side whose extent in bytes is a multiple of 4 and whose pointer is 4-byte aligned
//             moves one dword per lane (a wave covers 256 contiguous bytes per access): loads along B, stores along A.
//             Nothing wider: an 8- or 16-byte access along A would need 8 / 16 byte gathers per lane from LDS in phase 2
//             or as many scattered byte writes in phase 1, and the shapes this form exists for (NCHW <-> NHWC of 49-byte
//             planes, 85- and 197-long dims) rarely give a side an aligned 16 bytes.  The other side moves one element per
//             lane -- a wave still covers one contiguous run of up to 64 / 128 bytes.  Most ragged layers have ONE ragged
//             side only (49-byte planes against 2048 channels, 85 values against 400 pixels).  Names: tile_4 (dwords on
//             both sides), tile_4_1 (dword loads, element stores), tile_1_4 (element loads, dword stores), tile_1.
//             LDS.  The tile is kept in OUTPUT order, tile[b][a], so phase 2 reads whole dwords; phase 1 scatters elements.
//             Pitch: 68 bytes (int8: 17 dwords) / 66 halves (binary16: 33 dwords), an odd number of dwords.  ds_write and
//             ds_read_b32 bank a dword at (a / 4) % 32 within a 32-lane half: in _1 the lanes of a half write 32
//             consecutive b -- rows 17 b / 33 b apart, 32 distinct banks -- and read consecutive dwords of one row; in
//             _4 int8 the sixteen lanes of a row write bytes of rows 4 b' + j, 68 b' mod 32 takes 8 values: a 2-way
//             conflict on the byte writes (four lanes write bytes of ONE dword), accepted -- the form is bound by HBM.
//   generic   one output element per thread, every coordinate by division: the literal formula.  Takes any layer.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "requant_move.h"

namespace shl {

enum { TR_FLAT = 0, TR_ROWS = 1, TR_TILE = 2, TR_GENERIC = 3 };

constexpr int TR_DIMS = SHL_MI355X_MAX_DIM;
constexpr int TR_TILE_E = 64;  // elements per tile side

struct TrArgs {
    const void *in;
    void *out;
    // rows / generic: the canonical dims in output order, RIGHT-aligned (the innermost is [TR_DIMS - 1], the outermost
    // [first]); extents and input strides in the form's unit (pieces of W bytes / elements)
    int64_t ext[TR_DIMS], is[TR_DIMS];
    int64_t items;  // threads that have work (flat: pieces of 16 bytes, the tail's included)
    int64_t bytes;  // flat: of the tensor
    // tile: extents of A and B, A's stride in the input and B's in the output, tiles along each, the batch dims
    int64_t sa_in, sb_out;
    int64_t bis[TR_DIMS - 2], bos[TR_DIMS - 2];
    int32_t bext[TR_DIMS - 2];
    int32_t ea, eb, ta, tb, nb;
    int32_t first;
    MoveRec rec;
    int32_t small;  // the tensor has fewer than 2^32 elements: every index fits 32 bits
};

template <bool F16>
__global__ __launch_bounds__(256) void transpose_flat_kernel(TrArgs a)
{
    using E = typename std::conditional<F16, uint16_t, uint8_t>::type;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // piece of 16 bytes
    if (i >= a.items) return;
    const int64_t at = i * 16;
    if (at + 16 <= a.bytes) {
        static_cast<uint4 *>(a.out)[i] = move_piece<uint4, F16>(static_cast<const uint4 *>(a.in)[i], a.rec);
        return;
    }
    // the tail: fewer than 16 bytes, whole elements
    const E *src = reinterpret_cast<const E *>(static_cast<const uint8_t *>(a.in) + at);
    E *dst = reinterpret_cast<E *>(static_cast<uint8_t *>(a.out) + at);
    const int left = (int)((a.bytes - at) / (int64_t)sizeof(E));
    for (int e = 0; e < left; ++e) dst[e] = (E)move_elem<F16>(src[e], a.rec);
}

// rows (W = uint4 / uint32_t, LIT = false) and generic (W = the element, LIT = true): thread i owns output unit i and finds
// its source by taking i apart over the canonical dims, innermost first
template <typename W, bool F16, bool LIT>
__global__ __launch_bounds__(256) void transpose_walk_kernel(TrArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.items) return;
    int64_t rem = i, src = 0;
#pragma unroll
    for (int k = TR_DIMS - 1; k >= 0; --k) {
        if (k >= a.first) {  // (uniform)
            int64_t c;
            rem = move_divmod(rem, a.ext[k], a.small != 0, c);
            src += c * a.is[k];
        }
    }
    if constexpr (LIT) static_cast<W *>(a.out)[i] = (W)move_literal<F16>(static_cast<const W *>(a.in)[src], a.rec);
    else static_cast<W *>(a.out)[i] = move_piece<W, F16>(static_cast<const W *>(a.in)[src], a.rec);
}

template <bool F16, bool VIN, bool VOUT>
__global__ __launch_bounds__(256) void transpose_tile_kernel(TrArgs a)
{
    using E = typename std::conditional<F16, uint16_t, uint8_t>::type;
    constexpr int T = TR_TILE_E;
    constexpr int PA = F16 ? T + 2 : T + 4;  // pitch in elements: 33 / 17 dwords
    __shared__ __attribute__((aligned(16))) E tile[T * PA];  // [b][a]
    uint32_t blk = blockIdx.x;
    const int a0 = (int)(blk % (uint32_t)a.ta) * T;
    blk /= (uint32_t)a.ta;
    const int b0 = (int)(blk % (uint32_t)a.tb) * T;
    blk /= (uint32_t)a.tb;
    int64_t in_base = 0, out_base = 0;
#pragma unroll
    for (int k = TR_DIMS - 3; k >= 0; --k) {
        if (k < a.nb) {  // (uniform)
            const uint32_t c = blk % (uint32_t)a.bext[k];
            blk /= (uint32_t)a.bext[k];
            in_base += (int64_t)c * a.bis[k], out_base += (int64_t)c * a.bos[k];
        }
    }
    // phase 1: rows of the input (a fixed, b running)
    constexpr int EPV = VIN ? 4 / (int)sizeof(E) : 1;  // elements per global load
    constexpr int V = T / EPV;                         // loads per tile row
    for (int t = threadIdx.x; t < T * V; t += 256) {
        const int ar = t / V, b = (t - ar * V) * EPV;
        const int ga = a0 + ar, gb = b0 + b;
        if (ga < a.ea && gb < a.eb) {  // (VIN: eb is a multiple of EPV, so is gb: the whole access is inside)
            const int64_t at = in_base + (int64_t)ga * a.sa_in + gb;
            if constexpr (VIN) {
                const uint32_t w = move_word<F16>(static_cast<const uint32_t *>(a.in)[at / EPV], a.rec);
#pragma unroll
                for (int j = 0; j < EPV; ++j) tile[(b + j) * PA + ar] = (E)(w >> (8 * (int)sizeof(E) * j));
            } else {
                tile[b * PA + ar] = (E)move_elem<F16>(static_cast<const E *>(a.in)[at], a.rec);
            }
        }
    }
    __syncthreads();
    // phase 2: rows of the output (b fixed, a running)
    constexpr int EPO = VOUT ? 4 / (int)sizeof(E) : 1;  // elements per global store
    constexpr int VO = T / EPO;
    for (int t = threadIdx.x; t < T * VO; t += 256) {
        const int b = t / VO, ar = (t - b * VO) * EPO;
        const int ga = a0 + ar, gb = b0 + b;
        if (ga < a.ea && gb < a.eb) {  // (VOUT: ea is a multiple of EPO: every element of the dword was written in phase 1)
            const int64_t at = out_base + (int64_t)gb * a.sb_out + ga;
            if constexpr (VOUT) static_cast<uint32_t *>(a.out)[at / EPO] = *reinterpret_cast<const uint32_t *>(&tile[b * PA + ar]);
            else static_cast<E *>(a.out)[at] = tile[b * PA + ar];
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------
// the layer after canonicalisation: dims in OUTPUT order with their extents, strides in the input and in the output
// (elements).  rank >= 1; elems == 0: nothing to do
struct Canon {
    int rank;
    int64_t ext[TR_DIMS], is[TR_DIMS], os[TR_DIMS];
    int64_t elems;
};

// NULL when the descriptor describes a transpose, else what is wrong with it
static const char *transpose_invalid(const shl_mi355x_transpose_desc *d)
{
    if (!d) return "NULL argument";
    if (d->dtype != SHL_MI355X_I8 && d->dtype != SHL_MI355X_F16) return "dtype is neither int8 nor binary16";
    if (d->rank < 1 || d->rank > TR_DIMS) return "rank outside 1 .. 8";
    unsigned seen = 0;
    int64_t n = 1;
    for (int k = 0; k < d->rank; ++k) {
        if (d->perm[k] < 0 || d->perm[k] >= d->rank) return "a permutation entry out of range";
        if (seen & (1u << d->perm[k])) return "a repeated permutation entry";
        seen |= 1u << d->perm[k];
        if (d->dim[k] < 0) return "a negative dim";
        if (__builtin_mul_overflow(n, (int64_t)d->dim[k], &n)) return "tensor too large";
    }
    if (n > INT64_MAX / 2) return "tensor too large";
    return NULL;
}

static void canonicalise(const shl_mi355x_transpose_desc *d, Canon *c)
{
    int64_t stride[TR_DIMS];
    int64_t n = 1;
    for (int j = d->rank - 1; j >= 0; --j) stride[j] = n, n *= d->dim[j];
    c->elems = n;
    c->rank = 0;
    for (int k = 0; k < d->rank; ++k) {
        const int j = d->perm[k];
        if (d->dim[j] == 1) continue;  // (a dim of extent 1 has no coordinate to speak of)
        if (c->rank > 0 && c->is[c->rank - 1] == d->dim[j] * stride[j]) {
            // contiguous in the input behind its neighbour in the output: one dim
            c->ext[c->rank - 1] *= d->dim[j], c->is[c->rank - 1] = stride[j];
            continue;
        }
        c->ext[c->rank] = d->dim[j], c->is[c->rank] = stride[j], c->rank++;
    }
    if (c->rank == 0) c->ext[0] = 1, c->is[0] = 1, c->rank = 1;
    n = 1;
    for (int k = c->rank - 1; k >= 0; --k) c->os[k] = n, n *= c->ext[k];
}

static void canon_flat(int64_t elems, Canon *c)
{
    c->rank = 1, c->ext[0] = elems, c->is[0] = 1, c->os[0] = 1, c->elems = elems;
}

// NULL, or what is wrong with the buffers
static const char *buffers_invalid(const void *in_dev, const void *out_dev, int64_t bytes)
{
    if (!in_dev || !out_dev) return "NULL argument";
    if (ranges_overlap(in_dev, bytes, out_dev, bytes)) return "the output overlaps the input";
    return NULL;
}

// The one place that chooses the form and its width in bytes (launch and name).  SHL_MI355X_TRANSPOSE_FORM=generic | tile |
// rows forces a form (A/B runs, tests); one the arguments do not admit gives generic; read per call.  *kb: the canonical dim
// that is the input's innermost (tile).  *width of the tile form: 4, 41 (dword loads, element stores), 14, 1
static int canon_form(const void *in_dev, const void *out_dev, const Canon *c, int64_t es, int *width, int *kb)
{
    const char *force = getenv("SHL_MI355X_TRANSPOSE_FORM");
    const uintptr_t both = (uintptr_t)in_dev | (uintptr_t)out_dev;
    const int last = c->rank - 1;
    *width = 1, *kb = -1;
    if (force && strcmp(force, "generic") == 0) return TR_GENERIC;
    const bool only_tile = force && strcmp(force, "tile") == 0, only_rows = force && strcmp(force, "rows") == 0;
    if (!only_tile && !only_rows && c->rank == 1 && (both & 15) == 0) return TR_FLAT;
    if (c->is[last] == 1) {  // the innermost dim stays innermost
        const int64_t run = c->ext[last] * es;
        const int w = run % 16 == 0 && (both & 15) == 0 ? 16 : run % 4 == 0 && (both & 3) == 0 ? 4 : 0;
        if (only_tile || w == 0) return TR_GENERIC;
        *width = w;
        return TR_ROWS;
    }
    if (only_rows) return TR_GENERIC;
    for (int k = 0; k < last; ++k)
        if (c->is[k] == 1) *kb = k;
    if (*kb < 0 || c->ext[last] > 0x7FFFFFFF || c->ext[*kb] > 0x7FFFFFFF) return TR_GENERIC;
    for (int k = 0; k < last; ++k)
        if (k != *kb && c->ext[k] > 0x7FFFFFFF) return TR_GENERIC;
    const bool vin = (c->ext[*kb] * es) % 4 == 0 && ((uintptr_t)in_dev & 3) == 0;
    const bool vout = (c->ext[last] * es) % 4 == 0 && ((uintptr_t)out_dev & 3) == 0;
    *width = vin && vout ? 4 : vin ? 41 : vout ? 14 : 1;
    return TR_TILE;
}

static const char *canon_name(int form, int width)
{
    if (form == TR_FLAT) return "transpose_flat";
    if (form == TR_ROWS) return width == 16 ? "transpose_rows_16" : "transpose_rows_4";
    if (form == TR_TILE)
        return width == 4 ? "transpose_tile_4" : width == 41 ? "transpose_tile_4_1" : width == 14 ? "transpose_tile_1_4" : "transpose_tile_1";
    return "transpose_generic";
}

static int canon_launch(const char *op, const void *in_dev, void *out_dev, const Canon *c, int dtype, float in_scale,
                        int32_t in_zp, float out_scale, int32_t out_zp, hipStream_t s)
{
    const bool f16 = dtype == SHL_MI355X_F16;
    const int64_t es = f16 ? 2 : 1;
    int width, kb;
    const int form = canon_form(in_dev, out_dev, c, es, &width, &kb);
    const int last = c->rank - 1;
    TrArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in_dev, a.out = out_dev;
    a.rec = move_rec(in_scale, in_zp, out_scale, out_zp, !f16 && form != TR_GENERIC);
    a.small = c->elems < (1ll << 32);
    int64_t groups;
    void (*kernel)(TrArgs);  // (a template-id with a comma cannot be a macro argument)
    if (form == TR_FLAT) {
        a.bytes = c->elems * es;
        a.items = (a.bytes + 15) / 16;
        groups = (a.items + 255) / 256;
        kernel = f16 ? transpose_flat_kernel<true> : transpose_flat_kernel<false>;
    } else if (form == TR_TILE) {
        a.ea = (int32_t)c->ext[last], a.eb = (int32_t)c->ext[kb];
        a.sa_in = c->is[last], a.sb_out = c->os[kb];
        a.ta = (a.ea + TR_TILE_E - 1) / TR_TILE_E, a.tb = (a.eb + TR_TILE_E - 1) / TR_TILE_E;
        groups = (int64_t)a.ta * a.tb;
        for (int k = 0; k < last; ++k) {
            if (k == kb) continue;
            a.bext[a.nb] = (int32_t)c->ext[k], a.bis[a.nb] = c->is[k], a.bos[a.nb] = c->os[k], a.nb++;
            if (__builtin_mul_overflow(groups, c->ext[k], &groups)) groups = INT64_MAX;
        }
        if (width == 4) kernel = f16 ? transpose_tile_kernel<true, true, true> : transpose_tile_kernel<false, true, true>;
        else if (width == 41) kernel = f16 ? transpose_tile_kernel<true, true, false> : transpose_tile_kernel<false, true, false>;
        else if (width == 14) kernel = f16 ? transpose_tile_kernel<true, false, true> : transpose_tile_kernel<false, false, true>;
        else kernel = f16 ? transpose_tile_kernel<true, false, false> : transpose_tile_kernel<false, false, false>;
    } else {
        // rows: the unit is a piece of `width` bytes -- the innermost extent and every other dim's input stride (a multiple
        // of the innermost extent) are counted in pieces; generic: the unit is the element
        const int64_t per = form == TR_ROWS ? width / es : 1;  // elements per unit
        a.first = TR_DIMS - c->rank;
        for (int k = 0; k < c->rank; ++k) {
            a.ext[a.first + k] = k == last ? c->ext[k] / per : c->ext[k];
            a.is[a.first + k] = k == last ? c->is[k] : c->is[k] / per;
        }
        a.items = c->elems / per;
        groups = (a.items + 255) / 256;
        if (form == TR_ROWS) {
            if (width == 16) kernel = f16 ? transpose_walk_kernel<uint4, true, false> : transpose_walk_kernel<uint4, false, false>;
            else kernel = f16 ? transpose_walk_kernel<uint32_t, true, false> : transpose_walk_kernel<uint32_t, false, false>;
        } else {
            kernel = f16 ? transpose_walk_kernel<uint16_t, true, true> : transpose_walk_kernel<uint8_t, false, true>;
        }
    }
    if (grid_refused(op, groups)) return SHL_MI355X_ENOTSUP;
    const dim3 grid((unsigned)groups), block(256);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, a);
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

static const char *move_invalid(const shl_mi355x_move_desc *d, int64_t elems)
{
    if (!d) return "NULL argument";
    if (d->dtype != SHL_MI355X_I8 && d->dtype != SHL_MI355X_F16) return "dtype is neither int8 nor binary16";
    if (elems < 0 || elems > INT64_MAX / 2) return "element count negative or too large";
    return NULL;
}

}  // namespace shl

extern "C" const char *shl_mi355x_transpose_kernel_name(const void *in_dev, const void *out_dev,
                                                        const struct shl_mi355x_transpose_desc *d)
{
    using namespace shl;
    if (transpose_invalid(d)) return "";
    Canon c;
    canonicalise(d, &c);
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    if (buffers_invalid(in_dev, out_dev, c.elems * es)) return "";
    int width, kb;
    const int form = canon_form(in_dev, out_dev, &c, es, &width, &kb);
    return canon_name(form, width);
}

extern "C" int shl_mi355x_transpose(const void *in_dev, void *out_dev, const struct shl_mi355x_transpose_desc *d, void *stream)
{
    using namespace shl;
    const char *why = transpose_invalid(d);
    Canon c;
    if (!why) {
        canonicalise(d, &c);
        why = buffers_invalid(in_dev, out_dev, c.elems * (d->dtype == SHL_MI355X_F16 ? 2 : 1));
    }
    if (why) {
        set_error("transpose: %s", why);
        return SHL_MI355X_EINVAL;
    }
    if (c.elems == 0) return SHL_MI355X_OK;
    return canon_launch("transpose", in_dev, out_dev, &c, d->dtype, d->in_scale, d->in_zp, d->out_scale, d->out_zp,
                        (hipStream_t)stream);
}

extern "C" const char *shl_mi355x_move_kernel_name(const void *in_dev, const void *out_dev, int64_t elems,
                                                   const struct shl_mi355x_move_desc *d)
{
    using namespace shl;
    if (move_invalid(d, elems)) return "";
    const int64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    if (buffers_invalid(in_dev, out_dev, elems * es)) return "";
    Canon c;
    canon_flat(elems, &c);
    int width, kb;
    const int form = canon_form(in_dev, out_dev, &c, es, &width, &kb);
    return canon_name(form, width);
}

extern "C" int shl_mi355x_move(const void *in_dev, void *out_dev, int64_t elems, const struct shl_mi355x_move_desc *d, void *stream)
{
    using namespace shl;
    const char *why = move_invalid(d, elems);
    if (!why) why = buffers_invalid(in_dev, out_dev, elems * (d->dtype == SHL_MI355X_F16 ? 2 : 1));
    if (why) {
        set_error("move: %s", why);
        return SHL_MI355X_EINVAL;
    }
    if (elems == 0) return SHL_MI355X_OK;
    Canon c;
    canon_flat(elems, &c);
    return canon_launch("move", in_dev, out_dev, &c, d->dtype, d->in_scale, d->in_zp, d->out_scale, d->out_zp, (hipStream_t)stream);
}

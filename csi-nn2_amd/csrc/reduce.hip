// reduce.hip -- reductions of an int8 / binary16 tensor: sum, mean, max and min over any set of dims.  One entry point serves
// CSINN_OP_MEAN / _SUM / _MAX / _MIN (the stride family), CSINN_OP_REDUCE_MEAN / _SUM / _MAX / _MIN (the axis family) and
// CSINN_OP_GLOBAL_MAXPOOL2D.
//
// Restates, behind shl_ref_siso_callback_base (the whole input converted to float32 with its record, the float32 function,
// the result converted with the output's record):
//   shl_ref_{mean,sum,max,min}_stride_f32 (source/reference/mean.c:21-53, sum.c, max.c, min.c): output o reads
//       in[index(o, out_strides, out_extents) + index(i, inner_strides, inner_extents)] for i = 0 .. inner_size - 1 IN THAT
//       ORDER (shl_ref_get_reduction_index, utils.c:366-381: a mixed-radix number, the first group the outermost digit);
//       sum / mean start from 0 and add, mean ends with ONE division by (float)inner_size; max starts from -FLT_MAX, min from
//       +FLT_MAX
//   shl_ref_reduce_{mean,sum,max,min}_f32 (reduce_mean.c ..): outer x cnt x inner in the same fixed order; max / min start
//       from the FIRST element
//   shl_ref_global_maxpool2d_f32 (global_maxpool.c, maxpool.c:47-53): max from -FLT_MAX over the map, row by row
// The float32 additions are a dependent chain in the reference's order (__fadd_rn, nothing contracted, no tree): a sum
// is bit-identical only if it is the same chain.  max / min are the C library's fmax / fmin as the reference's build uses
// them: a NaN operand loses, two NaNs give the first, of two equal operands (+0 and -0) the SECOND is returned; here they
// are the same sequential walk (rd_step), so every class of row takes it.
// Per element: int8 x = (q - zp_in) * s_in (__fsub_rn, __fmul_rn), binary16 exact.  Per output: int8
// sat8(rint(x / s_out) + zp_out), the division through div_by_scale where the records admit it (reduce_fma_ok) and
// __fdiv_rn otherwise; binary16 float32_to_float16_base.
//
// The host canonicalises both group lists (extent-1 groups dropped, adjacent groups merged when the outer one's stride is the
// inner one's extent times its stride) and chooses ONE of three forms (rd_form, also behind the kernel-name function):
//   reduce_rows     the innermost inner group has stride 1 (NCHW mean / max over H and W, a last-axis reduce_*, axis = -1):
//                   a workgroup owns `rows` output rows.  Per pass all 256 lanes stage one window of every row into LDS as RAW
//                   elements -- windows lie on the 16-byte grid of global memory, a piece wholly inside the row is one
//                   16-byte load, a piece the row's head or tail shares with its neighbours takes element loads -- then lane r
//                   adds row r's window in index order, piece by piece: the four dword reads of the next piece are issued
//                   before the 16 / 8 steps of this one (one LDS read per element left the chain waiting on LDS: 42 -> 15 ns
//                   per int8 element of a long sum, profiles/reduce_notes.md).  A window is np pieces (a power of two up to 16: 256 bytes, the
//                   staging chunk); short rows take fewer pieces and more rows per pass (np = 16: 64 rows, 8: 128, <= 4:
//                   256).  A row's pitch is 4 np + 1 dwords, odd: the lanes' walks meet 64 different banks.
//   reduce_cols     the innermost outer group has stride 1 (NHWC mean over H and W, reduce_sum over a non-last axis, NHWC
//                   global_maxpool2d): one output per thread, adjacent threads read adjacent elements, so every step's load
//                   is coalesced; the loads are issued eight at a time ahead of the eight additions that consume them, so
//                   the chain waits on arithmetic, not on memory.  The inner offsets are the same for every lane (scalar).
//   reduce_generic  one output per thread, every inner index taken apart by division: the literal formula; any groups.
// SHL_MI355X_REDUCE_FORM=generic forces the literal form.  A single very long row is one lane's chain in every form.
#include <float.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "reduce_canon.h"  // the host side: validation, canonicalisation, the form rule (a stand-alone program compiles it too)
#include "common.h"

namespace shl {

enum { RD_ADD = 0, RD_MAX = 1, RD_MIN = 2 };  // the chain's step: sum and mean share one

constexpr int RD_PIECES = SHL_MI355X_REDUCE_CHUNK_BYTES / 16;  // pieces of 16 bytes in a full window
constexpr int RD_LDS_DWORDS = 256 * (4 * 4 + 1);               // the largest of rows * (4 np + 1): 256 rows of 4 pieces
static_assert(64 * (4 * RD_PIECES + 1) <= RD_LDS_DWORDS && 128 * (4 * 8 + 1) <= RD_LDS_DWORDS, "every (rows, np) pair fits");

struct RdArgs {
    const void *in;
    void *out;
    // canonical groups, RIGHT-aligned (the innermost is [RD_G - 1]); an unused slot has extent 1 and stride 0
    int32_t oext[RD_G], ostr[RD_G], iext[RD_G], istr[RD_G];
    int32_t out_count, inner_size;
    int32_t kind, init, div_fma;
    float si, zi, so, zo, inv_so;
    // rows: elements of a run (the innermost inner group), runs per output, pieces per window, rows per workgroup, windows
    // per run
    int32_t run, segs, np, rows, passes;
};

template <bool F16>
__device__ __forceinline__ float rd_cvt(uint32_t raw, const RdArgs &a)
{
    if constexpr (F16) return f16_bits_to_float((uint16_t)raw);
    else return __fmul_rn(__fsub_rn((float)(int8_t)raw, a.zi), a.si);  // int8_to_float_base
}

template <bool F16>
__device__ __forceinline__ uint32_t rd_load(const void *in, int64_t at)
{
    if constexpr (F16) return static_cast<const uint16_t *>(in)[at];
    else return static_cast<const uint8_t *>(in)[at];
}

// one step of the chain.  max / min: fmax(acc, v) / fmin(acc, v) of the C library the reference is built against.  A
// binary16 sum can meet NaNs, and float32_to_float16_base keeps a NaN's sign: the reference's addition (x86, acc += v) hands
// on acc's NaN, else v's, and makes the default NaN -- whose sign bit is set there -- from inf + -inf.  The selects below
// restate that choice instead of trusting this machine's; int8 sums meet no NaN
template <int K, bool F16>
__device__ __forceinline__ float rd_step(float acc, float v)
{
    if constexpr (K == RD_ADD) {
        const float r = __fadd_rn(acc, v);
        if constexpr (F16) return r == r ? r : (acc != acc ? acc : (v != v ? v : __uint_as_float(0xFFC00000u)));
        else return r;
    } else if constexpr (K == RD_MAX) {
        return v != v ? acc : (acc != acc ? v : (acc > v ? acc : v));
    } else {
        return v != v ? acc : (acc != acc ? v : (acc < v ? acc : v));
    }
}

// the chain's start.  First-element rule: the element is then stepped over once more, which changes nothing (fmax(x, x) is
// x, of two NaNs the first stays)
template <int K, bool F16>
__device__ __forceinline__ float rd_start(const RdArgs &a, int64_t base)
{
    if constexpr (K == RD_ADD) return 0.0f;
    if (a.init == SHL_MI355X_REDUCE_INIT_FIRST) return rd_cvt<F16>(rd_load<F16>(a.in, base), a);
    return K == RD_MAX ? -FLT_MAX : FLT_MAX;
}

template <bool F16>
__device__ __forceinline__ void rd_store(const RdArgs &a, int64_t o, float acc)
{
    if constexpr (F16) {
        if (acc != acc) {  // a NaN keeps its sign through the mean's division and the conversion
            static_cast<uint16_t *>(a.out)[o] = (__float_as_uint(acc) >> 31) ? 0xFFFFu : 0x7FFFu;
            return;
        }
    }
    if (a.kind == SHL_MI355X_REDUCE_MEAN) acc = __fdiv_rn(acc, (float)a.inner_size);
    if constexpr (F16) {
        static_cast<uint16_t *>(a.out)[o] = float_to_f16_bits_ref(acc);
    } else {
        const float d = a.div_fma ? div_by_scale(acc, a.so, a.inv_so) : __fdiv_rn(acc, a.so);
        static_cast<int8_t *>(a.out)[o] = (int8_t)sat8_from_float(__fadd_rn(rintf(d), a.zo));  // float_to_int8_base
    }
}

// shl_ref_get_reduction_index over the canonical groups
__device__ __forceinline__ int64_t rd_index(uint32_t k, const int32_t *ext, const int32_t *str)
{
    int64_t at = 0;
#pragma unroll
    for (int g = RD_G - 1; g >= 0; --g) {
        const uint32_t q = k / (uint32_t)ext[g];
        at += (int64_t)(k - q * (uint32_t)ext[g]) * str[g];
        k = q;
    }
    return at;
}

// the inner offset of consecutive inner indices without a division: counters over the canonical inner groups from slot
// `LAST` outwards (the same for every lane)
template <int LAST>
struct RdWalk {
    int32_t c[RD_G];
    int64_t off;
    __device__ __forceinline__ void reset()
    {
#pragma unroll
        for (int g = 0; g < RD_G; ++g) c[g] = 0;
        off = 0;
    }
    __device__ __forceinline__ void advance(const RdArgs &a)
    {
        off += a.istr[LAST];
#pragma unroll
        for (int g = LAST; g >= 1; --g) {
            if (++c[g] < a.iext[g]) return;
            c[g] = 0;
            off += (int64_t)a.istr[g - 1] - (int64_t)a.iext[g] * a.istr[g];
        }
    }
};

template <int K, bool F16>
__global__ __launch_bounds__(256) void reduce_generic_kernel(RdArgs a)
{
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= a.out_count) return;
    const int64_t base = rd_index((uint32_t)o, a.oext, a.ostr);
    float acc = rd_start<K, F16>(a, base);
    for (int32_t i = 0; i < a.inner_size; ++i)
        acc = rd_step<K, F16>(acc, rd_cvt<F16>(rd_load<F16>(a.in, base + rd_index((uint32_t)i, a.iext, a.istr)), a));
    rd_store<F16>(a, o, acc);
}

template <int K, bool F16>
__global__ __launch_bounds__(256) void reduce_cols_kernel(RdArgs a)
{
    constexpr int B = 8;  // loads in flight ahead of the additions
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= a.out_count) return;
    const int64_t base = rd_index((uint32_t)o, a.oext, a.ostr);
    float acc = rd_start<K, F16>(a, base);
    RdWalk<RD_G - 1> w;
    w.reset();
    int32_t i = 0;
    for (; i + B <= a.inner_size; i += B) {
        uint32_t raw[B];
#pragma unroll
        for (int j = 0; j < B; ++j) {
            raw[j] = rd_load<F16>(a.in, base + w.off);
            w.advance(a);
        }
#pragma unroll
        for (int j = 0; j < B; ++j) acc = rd_step<K, F16>(acc, rd_cvt<F16>(raw[j], a));
    }
    for (; i < a.inner_size; ++i) {
        acc = rd_step<K, F16>(acc, rd_cvt<F16>(rd_load<F16>(a.in, base + w.off), a));
        w.advance(a);
    }
    rd_store<F16>(a, o, acc);
}

template <int K, bool F16>
__global__ __launch_bounds__(256) void reduce_rows_kernel(RdArgs a)
{
    using E = typename std::conditional<F16, uint16_t, uint8_t>::type;
    constexpr int ES = (int)sizeof(E);
    __shared__ __attribute__((aligned(16))) uint32_t win[RD_LDS_DWORDS];
    __shared__ int32_t row_base[256];
    const int tid = (int)threadIdx.x;
    const int np = a.np, pitch = 4 * np + 1;  // dwords
    const int64_t row0 = (int64_t)blockIdx.x * a.rows;
    const int nrows = (int)(a.out_count - row0 < (int64_t)a.rows ? a.out_count - row0 : (int64_t)a.rows);  // <= 256
    const bool own = tid < nrows;
    const int64_t my_base = own ? rd_index((uint32_t)(row0 + tid), a.oext, a.ostr) : 0;
    if (own) row_base[tid] = (int32_t)my_base;  // (an index into fewer than 2^31 elements)
    float acc = own ? rd_start<K, F16>(a, my_base) : 0.0f;
    const uintptr_t in0 = (uintptr_t)a.in;
    const int64_t run_bytes = (int64_t)a.run * ES, window = (int64_t)np * 16;
    RdWalk<RD_G - 2> seg;  // over the inner groups outside the run
    seg.reset();
    for (int32_t s = 0; s < a.segs; ++s) {
        for (int32_t pass = 0; pass < a.passes; ++pass) {
            __syncthreads();  // the previous window was consumed (first pass: row_base is written)
            for (int it = tid; it < nrows * np; it += 256) {
                const int r = it / np, p = it - r * np;
                const uintptr_t first = in0 + (uintptr_t)(((int64_t)row_base[r] + seg.off) * ES);  // the run's first byte
                const uintptr_t end = first + (uintptr_t)run_bytes;
                const uintptr_t g = (first & ~(uintptr_t)15) + (uintptr_t)(pass * window + p * 16);
                uint32_t *dst = &win[r * pitch + p * 4];
                if (g >= first && g + 16 <= end) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(g);
                    dst[0] = v.x, dst[1] = v.y, dst[2] = v.z, dst[3] = v.w;
                } else if (g + 16 > first && g < end) {  // the run's head or tail: only its own elements are read
                    E *d = reinterpret_cast<E *>(dst);
                    for (int e = 0; e < 16 / ES; ++e) {
                        const uintptr_t at = g + (uintptr_t)(e * ES);
                        if (at >= first && at < end) d[e] = *reinterpret_cast<const E *>(at);
                    }
                }
            }
            __syncthreads();
            if (own) {
                // the row's bytes inside this window, [from, to) from the window's start; walked in the 16-byte pieces they
                // were staged in: four dword reads ahead of the piece's 16 / 8 steps, the next piece's reads issued before
                // this one's chain, so that the chain waits on arithmetic and not on LDS; a piece the row only partly
                // covers (its head, its tail) steps over its own elements only
                const int64_t lo = (int64_t)((in0 + (uintptr_t)((my_base + seg.off) * ES)) & 15);  // of the run in its first window
                const int64_t w0 = pass * window;
                const int from = (int)((lo > w0 ? lo : w0) - w0);
                const int to = (int)((lo + run_bytes < w0 + window ? lo + run_bytes : w0 + window) - w0);
                const uint32_t *row = &win[tid * pitch];
                int p = from & ~15;
                uint32_t cur[4] = {0u, 0u, 0u, 0u}, nxt[4] = {0u, 0u, 0u, 0u};
                if (p < to) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) cur[j] = row[p / 4 + j];
                }
                for (; p < to; p += 16) {
                    if (p + 16 < to) {  // (p + 32 <= the window: `to` is at most the window, p a multiple of 16)
#pragma unroll
                        for (int j = 0; j < 4; ++j) nxt[j] = row[p / 4 + 4 + j];
                    }
                    if (p >= from && p + 16 <= to) {
#pragma unroll
                        for (int e = 0; e < 16 / ES; ++e)
                            acc = rd_step<K, F16>(acc, rd_cvt<F16>(cur[e * ES / 4] >> (8 * (e * ES % 4)), a));
                    } else {
#pragma unroll
                        for (int e = 0; e < 16 / ES; ++e) {
                            const int b = p + e * ES;
                            if (b >= from && b < to) acc = rd_step<K, F16>(acc, rd_cvt<F16>(cur[e * ES / 4] >> (8 * (e * ES % 4)), a));
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
                }
            }
        }
        seg.advance(a);
    }
    if (own) rd_store<F16>(a, row0 + tid, acc);
}

// ---- host side (validation, canonicalisation and the form rule are in reduce_canon.h) ----------------------------------
static int reduce_launch(const void *in_dev, void *out_dev, const shl_mi355x_reduce_desc *d, const RdCanon *c, hipStream_t s)
{
    const bool f16 = d->dtype == SHL_MI355X_F16;
    const int form = rd_form(c);
    RdArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in_dev, a.out = out_dev;
    for (int g = 0; g < RD_G; ++g) a.oext[g] = a.iext[g] = 1;
    for (int g = 0; g < c->n_out; ++g) a.oext[RD_G - c->n_out + g] = (int32_t)c->oext[g], a.ostr[RD_G - c->n_out + g] = (int32_t)c->ostr[g];
    for (int g = 0; g < c->n_in; ++g) a.iext[RD_G - c->n_in + g] = (int32_t)c->iext[g], a.istr[RD_G - c->n_in + g] = (int32_t)c->istr[g];
    a.out_count = (int32_t)c->out_count, a.inner_size = (int32_t)c->inner_size;
    a.kind = d->kind, a.init = d->init;
    a.si = d->in_scale, a.zi = (float)d->in_zp;
    a.so = d->out_scale, a.zo = (float)d->out_zp, a.inv_so = 1.0f / d->out_scale;
    a.div_fma = !f16 && reduce_fma_ok(d, c);
    int64_t groups = (c->out_count + 255) / 256;
    if (form == RD_ROWS) {
        RdRows r;
        rd_rows_plan(c, f16 ? 2 : 1, &r);
        a.run = r.run, a.segs = r.segs, a.np = r.np, a.rows = r.rows, a.passes = r.passes;
        groups = (c->out_count + r.rows - 1) / r.rows;
    }
    const int k = d->kind == SHL_MI355X_REDUCE_MAX ? RD_MAX : d->kind == SHL_MI355X_REDUCE_MIN ? RD_MIN : RD_ADD;
    void (*kernel)(RdArgs);
#define RD_PICK(NAME)                                                                                  \
    (k == RD_ADD ? (f16 ? NAME<RD_ADD, true> : NAME<RD_ADD, false>)                                    \
                 : k == RD_MAX ? (f16 ? NAME<RD_MAX, true> : NAME<RD_MAX, false>) : (f16 ? NAME<RD_MIN, true> : NAME<RD_MIN, false>))
    if (form == RD_ROWS) kernel = RD_PICK(reduce_rows_kernel);
    else if (form == RD_COLS) kernel = RD_PICK(reduce_cols_kernel);
    else kernel = RD_PICK(reduce_generic_kernel);
#undef RD_PICK
    const dim3 grid((unsigned)groups), block(256);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, a);
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

}  // namespace shl

extern "C" const char *shl_mi355x_reduce_kernel_name(const void *in_dev, const void *out_dev, const struct shl_mi355x_reduce_desc *d)
{
    using namespace shl;
    RdCanon c;
    if (rd_canonicalise(in_dev, out_dev, d, &c)) return "";
    return rd_form_name(rd_form(&c));
}

extern "C" int shl_mi355x_reduce(const void *in_dev, void *out_dev, const struct shl_mi355x_reduce_desc *d, void *stream)
{
    using namespace shl;
    RdCanon c;
    const char *why = rd_canonicalise(in_dev, out_dev, d, &c);
    if (why) {
        set_error("reduce: %s", why);
        return SHL_MI355X_EINVAL;
    }
    if (c.out_count == 0) return SHL_MI355X_OK;
    return reduce_launch(in_dev, out_dev, d, &c, (hipStream_t)stream);
}

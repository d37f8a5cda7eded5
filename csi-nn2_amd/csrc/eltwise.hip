// eltwise.hip -- sigmoid / hard_sigmoid / silu / leaky_relu (CSINN_OP_SIGMOID, _HARD_SIGMOID, _SILU, _LEAKY_RELU) and the
// broadcasting product (CSINN_OP_MUL) on int8 / binary16 tensors.
//
// The four activations run inside shl_ref_siso_callback_base (source/reference/utils.c:609-621): dequantise, a pure
// per-element function in float / double (sigmoid.c:33, silu.c:33, hard_sigmoid.c:31-37, leaky_relu.c:33), requantise.
//   int8      the output byte depends on the input byte and the two records only: the backend builds the 256 results on
//             the host (source/mi355x_opt/eltwise.c) and the kernel here looks them up.  The table travels BY VALUE in
//             the kernel arguments (256 bytes: nothing to allocate or keep alive, capturable) and sits in LDS while the
//             workgroup runs; no transcendental, no division on the device.  unary_lut_i8_vec_kernel: 16 bytes per lane
//             per access + a one-byte tail; unary_lut_i8_byte_kernel: one byte per thread, for pointers off the 16-byte
//             grid (a DMABUF tensor can start anywhere).
//   binary16  unary_f16_kernel<KIND>: f16 -> f32 exactly, the reference's formula in the reference's precision (double
//             exp, __dadd_rn / __ddiv_rn: nothing contracted but hard_sigmoid's 0.2 x + 0.5, which the reference's build
//             fuses), ONE rounding to float, the reference's
//             float -> binary16 rounding.  A NaN comes out as the x86 operations propagate it: with its sign (sigmoid:
//             the sign flipped, it went through exp(-x)), every payload 0x7FFF.  Compute-bound on large maps by design.
//
// mul (source/reference/mul.c:21-40 inside shl_ref_diso_callback_base): both operands dequantised, ONE fp32 product,
// requantised (int8: div_by_scale where the records admit it) / rounded to binary16.  `a` has the output's shape; `b`
// is broadcast to it following shl_ref_broadcast_to_shape_f32 (utils.c:692-785).  The output's dims arrive collapsed to
// at most four groups with b's stride per group (0: b is broadcast along it).  Forms, chosen by mul_form() below, which
// also names them:
//   vec       16 bytes per lane in output order when b is same-shape, a scalar, or varies only along an unbroadcast
//             innermost group of whole 16-byte pieces (NHWC [N,1,1,C], [C], [1,1,1,C] with C % 16 == 0, binary16 % 8):
//             b is fetched 16 bytes at a time as well
//   row       the innermost group is broadcast (NCHW [N,C,1,1] / [1,C,1,1]): 16 bytes of a / out per lane on the flat
//             tensor, one b value per run of H*W elements, fetched again where a run ends inside the piece
//   generic   one output per thread, any groups and alignment (SHL_MI355X_MUL_FORM=generic forces it)
// vec and row need a and out (vec: b too, unless it is a scalar) on the 16-byte grid; elements behind the last whole
// piece take the one-output path inside the same launch.
//
// The broadcasting add (CSINN_OP_ADD with operands of different shapes: source/reference/add.c:21-41, the same
// shl_ref_diso_callback_base and the same broadcast) is these three kernels instantiated with the sum as the element
// function: add_vec / add_row / add_generic, the same form rule (SHL_MI355X_ADD_FORM=generic forces the last), the same
// descriptor.  [.., N] + [N] with N in whole pieces -- a linear layer's bias -- is the vec form.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "add_step.h"
#include "common.h"
#include "lut_step.h"
#include "mul_step.h"

namespace shl {

// ------------------------------------------------------------------------------------------ int8 unary by table
// (Lut256 and lut4: lut_step.h, which the convolution's fused stores call as well)
// the table is the FIRST kernel argument: lane t copies dword t of the argument block to LDS (indexing the by-value
// struct with a lane id would send it through scratch)
__device__ __forceinline__ void lut_to_lds(uint32_t *lds)
{
    typedef const __attribute__((address_space(4))) uint32_t *kernarg_words;
    if (threadIdx.x < 64) lds[threadIdx.x] = ((kernarg_words)__builtin_amdgcn_kernarg_segment_ptr())[threadIdx.x];
    __syncthreads();
}

__global__ __launch_bounds__(256) void unary_lut_i8_vec_kernel(Lut256 tab, const int8_t *in, int8_t *out, size_t count)
{
    __shared__ uint32_t lds[64];
    lut_to_lds(lds);
    const uint8_t *lut = reinterpret_cast<const uint8_t *>(lds);
    const size_t nvec = count / 16;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        uint4 v = reinterpret_cast<const uint4 *>(in)[i];
        v.x = lut4(lut, v.x), v.y = lut4(lut, v.y), v.z = lut4(lut, v.z), v.w = lut4(lut, v.w);
        reinterpret_cast<uint4 *>(out)[i] = v;
    }
    // ragged tail: count % 16 bytes
    for (size_t i = nvec * 16 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
        out[i] = (int8_t)lut[(uint8_t)in[i]];
}

__global__ __launch_bounds__(256) void unary_lut_i8_byte_kernel(Lut256 tab, const int8_t *in, int8_t *out, size_t count)
{
    __shared__ uint32_t lds[64];
    lut_to_lds(lds);
    const uint8_t *lut = reinterpret_cast<const uint8_t *>(lds);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) out[i] = (int8_t)lut[(uint8_t)in[i]];
}

// ------------------------------------------------------------------------------------------ binary16 unary
template <int KIND>
__device__ __forceinline__ uint16_t unary_f16_one(uint16_t h, float alpha)
{
    const float v = f16_bits_to_float(h);
    if ((h & 0x7FFFu) > 0x7C00u) {
        // a NaN leaves every one of these formulas as a NaN and float32_to_float16_base keeps only its sign; sigmoid's
        // went through exp(-x), which hands the negated argument back
        return (uint16_t)(0x7FFFu | ((KIND == SHL_MI355X_UNARY_SIGMOID ? ~h : h) & 0x8000u));
    }
    float r;
    if constexpr (KIND == SHL_MI355X_UNARY_SIGMOID) {
        r = __double2float_rn(__ddiv_rn(1.0, __dadd_rn(1.0, exp((double)(-v)))));  // sigmoid.c:33
    } else if constexpr (KIND == SHL_MI355X_UNARY_SILU) {
        r = __double2float_rn(__ddiv_rn((double)v, __dadd_rn(1.0, exp((double)(-v)))));  // silu.c:33
    } else if constexpr (KIND == SHL_MI355X_UNARY_HARD_SIGMOID) {
        // hard_sigmoid.c:31-37: double comparisons, double 0.2 x + 0.5 -- which the reference's build (-O3 -mfma) contracts
        // into ONE fused multiply-add: at x = -2.5 the result is -2.8e-17, a negative zero in binary16, where the two
        // roundings give +0 (the genuine library's output over all 65 536 patterns decides, tests/golden/eltwise_cases.npz)
        const double x = (double)v;
        r = x < -2.5 ? 0.0f : x > 2.5 ? 1.0f : __double2float_rn(__fma_rn(0.2, x, 0.5));
    } else {
        r = v > 0.0f ? v : __fmul_rn(v, alpha);  // leaky_relu.c:33
    }
    return float_to_f16_bits_ref(r);
}

template <int KIND>
__global__ __launch_bounds__(256) void unary_f16_kernel(const uint16_t *in, uint16_t *out, size_t count, float alpha)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
        out[i] = unary_f16_one<KIND>(in[i], alpha);
}

// ------------------------------------------------------------------------------------------ mul, broadcasting add
enum { OP_MUL = 0, OP_ADD = 1 };  // what the three kernels below compute: they are shared, the element function is not
enum { MUL_VEC = 0, MUL_ROW = 1, MUL_GENERIC = 2 };
enum { B_SAME = 0, B_SCALAR = 1, B_INNER = 2 };  // how the vec form finds b

struct MulArgs {
    const void *a, *b;
    void *out;
    uint64_t count;     // elements of the output
    uint64_t dim[4];    // the output's groups, outermost first, padded in front with 1
    uint64_t bs[4];     // b's stride per group, in elements
    float sa, za, sb, zb, so, zo, inv_so;
    int32_t fma_div;    // div_by_scale is exact for every product (sum) these records can give
    int32_t b_mode;     // vec form: B_*
    int32_t a_second;   // a is the reference's SECOND input (the callback swapped the operands): whose NaN goes through
};

// b's element for output element e.  I: uint32_t when the output has fewer than 2^32 elements
template <typename I>
__device__ __forceinline__ uint64_t mul_b_index(const MulArgs &m, I e)
{
    const I d1 = (I)m.dim[1], d2 = (I)m.dim[2], d3 = (I)m.dim[3];
    const I c3 = e % d3;
    e /= d3;
    const I c2 = e % d2;
    e /= d2;
    const I c1 = e % d1, c0 = e / d1;
    return (uint64_t)c0 * m.bs[0] + (uint64_t)c1 * m.bs[1] + (uint64_t)c2 * m.bs[2] + (uint64_t)c3 * m.bs[3];
}

__device__ __forceinline__ uint64_t mul_b_index(const MulArgs &m, uint64_t e)
{
    return m.count <= 0xFFFFFFFFull ? mul_b_index<uint32_t>(m, (uint32_t)e) : mul_b_index<uint64_t>(m, e);
}

// mul: mul_i8_one / mul_f16_one of mul_step.h, which the fused attention kernel's scale step (attention.hip) applies as well
// add: the element function of add_step.h, which the fused matmul + bias store (matmul.hip) applies as well
__device__ __forceinline__ int add_i8_one(int qa, int qb, const MulArgs &m)
{
    const AddRec r = {m.sa, m.za, m.sb, m.zb, m.so, m.zo, m.inv_so, m.fma_div};
    return add_i8_step(qa, qb, r);
}

__device__ __forceinline__ uint16_t add_f16_one(uint16_t ha, uint16_t hb, const MulArgs &m)
{
    return m.a_second ? add_f16_step(hb, ha) : add_f16_step(ha, hb);  // (the reference's input0, input1)
}

template <bool F16, int OP>
__device__ __forceinline__ auto elem_one(typename std::conditional<F16, uint16_t, int>::type va,
                                         typename std::conditional<F16, uint16_t, int>::type vb, const MulArgs &m)
{
    if constexpr (F16) return OP == OP_ADD ? add_f16_one(va, vb, m) : mul_f16_one(va, vb, m);
    else return OP == OP_ADD ? add_i8_one(va, vb, m) : mul_i8_one(va, vb, m);
}

template <bool F16, int OP>
__device__ __forceinline__ void mul_one(const MulArgs &m, uint64_t e, uint64_t bi)
{
    if constexpr (F16) {
        static_cast<uint16_t *>(m.out)[e] = elem_one<true, OP>(static_cast<const uint16_t *>(m.a)[e], static_cast<const uint16_t *>(m.b)[bi], m);
    } else {
        static_cast<int8_t *>(m.out)[e] = (int8_t)elem_one<false, OP>(static_cast<const int8_t *>(m.a)[e], static_cast<const int8_t *>(m.b)[bi], m);
    }
}

template <bool F16, int OP>
__device__ __forceinline__ uint32_t mul_word(uint32_t wa, uint32_t wb, const MulArgs &m)
{
    if constexpr (F16) {
        return (uint32_t)elem_one<true, OP>((uint16_t)wa, (uint16_t)wb, m) | ((uint32_t)elem_one<true, OP>((uint16_t)(wa >> 16), (uint16_t)(wb >> 16), m) << 16);
    } else {
        return pack4_i8(elem_one<false, OP>((int8_t)wa, (int8_t)wb, m), elem_one<false, OP>((int8_t)(wa >> 8), (int8_t)(wb >> 8), m),
                        elem_one<false, OP>((int8_t)(wa >> 16), (int8_t)(wb >> 16), m), elem_one<false, OP>((int8_t)(wa >> 24), (int8_t)(wb >> 24), m));
    }
}

template <bool F16, int OP = OP_MUL>
__global__ __launch_bounds__(256) void mul_vec_kernel(MulArgs m)
{
    constexpr uint64_t E = F16 ? 8 : 16;  // elements per piece
    const uint64_t nvec = m.count / E;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint4 vb = make_uint4(0, 0, 0, 0);
    if (m.b_mode == B_SCALAR) {
        const uint32_t s = F16 ? static_cast<const uint16_t *>(m.b)[0] * 0x00010001u : static_cast<const uint8_t *>(m.b)[0] * 0x01010101u;
        vb = make_uint4(s, s, s, s);
    }
    for (uint64_t i = t; i < nvec; i += stride) {
        const uint4 va = static_cast<const uint4 *>(m.a)[i];
        if (m.b_mode == B_SAME) vb = static_cast<const uint4 *>(m.b)[i];
        else if (m.b_mode == B_INNER) vb = *reinterpret_cast<const uint4 *>(static_cast<const char *>(m.b) + mul_b_index(m, i * E) * (F16 ? 2 : 1));
        uint4 r;
        r.x = mul_word<F16, OP>(va.x, vb.x, m), r.y = mul_word<F16, OP>(va.y, vb.y, m);
        r.z = mul_word<F16, OP>(va.z, vb.z, m), r.w = mul_word<F16, OP>(va.w, vb.w, m);
        static_cast<uint4 *>(m.out)[i] = r;
    }
    for (uint64_t e = nvec * E + t; e < m.count; e += stride) mul_one<F16, OP>(m, e, mul_b_index(m, e));
}

// the innermost group (run = dim[3]) is broadcast: element e takes b's element of its row e / run
template <bool F16, int OP = OP_MUL>
__global__ __launch_bounds__(256) void mul_row_kernel(MulArgs m)
{
    constexpr int E = F16 ? 8 : 16;
    typedef typename std::conditional<F16, uint16_t, uint8_t>::type T;
    const uint64_t nvec = m.count / E, run = m.dim[3];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = t; i < nvec; i += stride) {
        const uint4 va = static_cast<const uint4 *>(m.a)[i];
        const uint32_t wa[4] = {va.x, va.y, va.z, va.w};
        uint32_t wb[4] = {0, 0, 0, 0};
        const uint64_t e0 = i * E;
        uint64_t left = run - e0 % run;  // elements of the current run from e0 on
        uint32_t bv = static_cast<const T *>(m.b)[mul_b_index(m, e0)];
#pragma unroll
        for (int k = 0; k < E; ++k) {
            if (left == 0) {
                bv = static_cast<const T *>(m.b)[mul_b_index(m, e0 + k)];
                left = run;
            }
            --left;
            wb[k * (F16 ? 2 : 1) / 4] |= bv << (F16 ? 16 * (k & 1) : 8 * (k & 3));
        }
        uint4 r;
        r.x = mul_word<F16, OP>(wa[0], wb[0], m), r.y = mul_word<F16, OP>(wa[1], wb[1], m);
        r.z = mul_word<F16, OP>(wa[2], wb[2], m), r.w = mul_word<F16, OP>(wa[3], wb[3], m);
        static_cast<uint4 *>(m.out)[i] = r;
    }
    for (uint64_t e = nvec * E + t; e < m.count; e += stride) mul_one<F16, OP>(m, e, mul_b_index(m, e));
}

template <bool F16, int OP = OP_MUL>
__global__ __launch_bounds__(256) void mul_generic_kernel(MulArgs m)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m.count; e += stride) mul_one<F16, OP>(m, e, mul_b_index(m, e));
}

// ---- host side ---------------------------------------------------------------------------------------------
static bool overlaps(const void *p, uint64_t pbytes, const void *q, uint64_t qbytes)
{
    const uintptr_t p0 = (uintptr_t)p, p1 = p0 + pbytes, q0 = (uintptr_t)q, q1 = q0 + qbytes;
    return p0 < p1 && q0 < q1 && p0 < q1 && q0 < p1;
}

static unsigned grid_for(uint64_t items)
{
    uint64_t blocks = (items + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 256 * 8) blocks = 256 * 8;
    return (unsigned)blocks;
}

// NULL when `d` and the pointers describe a product, else what is wrong; *count: the output's elements, *b_count: b's
static const char *mul_invalid(const void *a, const void *b, const void *out, const shl_mi355x_mul_desc *d, uint64_t *count,
                               uint64_t *b_count)
{
    if (!d || !a || !b || !out) return "NULL argument";
    if (d->dtype != SHL_MI355X_I8 && d->dtype != SHL_MI355X_F16) return "dtype is neither int8 nor binary16";
    if (d->ngroups < 1 || d->ngroups > 4) return "ngroups outside 1 .. 4";
    int64_t n = 1, last = 0;
    for (int g = 0; g < d->ngroups; ++g) {
        if (d->dim[g] < 0 || d->b_stride[g] < 0) return "negative size";
        if (__builtin_mul_overflow(n, d->dim[g], &n) || n > (int64_t)1 << 60) return "tensor too large";
        if (d->dim[g] > 0) last += (d->dim[g] - 1) * d->b_stride[g];
    }
    const uint64_t es = d->dtype == SHL_MI355X_F16 ? 2 : 1;
    *count = (uint64_t)n;
    *b_count = n > 0 ? (uint64_t)last + 1 : 0;
    if (overlaps(out, *count * es, a, *count * es) || overlaps(out, *count * es, b, *b_count * es)) return "the output overlaps an input";
    return NULL;
}

// The one place that chooses the form (launch and name), for mul and for the broadcasting add; *b_mode: how the vec form
// finds b.  SHL_MI355X_MUL_FORM=generic / SHL_MI355X_ADD_FORM=generic forces the literal form (A/B runs, tests); read per call.
static int mul_form(int op, const void *a, const void *b, const void *out, const shl_mi355x_mul_desc *d, int *b_mode)
{
    const char *force = getenv(op == OP_ADD ? "SHL_MI355X_ADD_FORM" : "SHL_MI355X_MUL_FORM");
    if (force && strcmp(force, "generic") == 0) return MUL_GENERIC;
    if ((((uintptr_t)a | (uintptr_t)out) & 15) != 0) return MUL_GENERIC;
    const int64_t E = d->dtype == SHL_MI355X_F16 ? 8 : 16;
    const int n = d->ngroups;
    bool scalar = true;
    for (int g = 0; g < n; ++g) scalar = scalar && (d->b_stride[g] == 0 || d->dim[g] == 1);
    if (scalar) {
        *b_mode = B_SCALAR;
        return MUL_VEC;
    }
    const bool b_aligned = ((uintptr_t)b & 15) == 0;
    if (n == 1) {  // same shape (stride 1; any other stride is nobody's broadcast: generic)
        *b_mode = B_SAME;
        return d->b_stride[0] == 1 && b_aligned ? MUL_VEC : MUL_GENERIC;
    }
    if (d->b_stride[n - 1] == 0 && d->dim[n - 1] > 1) return MUL_ROW;
    if (d->b_stride[n - 1] == 1 && d->dim[n - 1] % E == 0 && b_aligned) {
        // every piece lies inside one innermost run; the outer strides must keep b's pieces on the 16-byte grid
        for (int g = 0; g < n - 1; ++g)
            if (d->dim[g] > 1 && d->b_stride[g] % E != 0) return MUL_GENERIC;
        *b_mode = B_INNER;
        return MUL_VEC;
    }
    return MUL_GENERIC;
}

static const char *const kMulNames[2][3] = {{"mul_vec", "mul_row", "mul_generic"}, {"add_vec", "add_row", "add_generic"}};

static const char *bcast_kernel_name(int op, const shl_mi355x_mul_desc *d, const void *a, const void *b, const void *out)
{
    uint64_t count, b_count;
    int b_mode = 0;
    if (mul_invalid(a, b, out, d, &count, &b_count)) return "";
    return kMulNames[op][mul_form(op, a, b, out, d, &b_mode)];
}

// validate, choose the form, enqueue: shl_mi355x_mul and shl_mi355x_add_bcast
template <int OP>
static int bcast_launch(const char *what, const void *a_dev, const void *b_dev, void *out_dev, const shl_mi355x_mul_desc *d,
                        void *stream)
{
    uint64_t count, b_count;
    const char *why = mul_invalid(a_dev, b_dev, out_dev, d, &count, &b_count);
    if (why) {
        set_error("%s: %s", what, why);
        return SHL_MI355X_EINVAL;
    }
    if (count == 0) return SHL_MI355X_OK;
    const bool f16 = d->dtype == SHL_MI355X_F16;
    MulArgs m;
    memset(&m, 0, sizeof(m));
    m.a = a_dev, m.b = b_dev, m.out = out_dev, m.count = count;
    for (int g = 0; g < 4; ++g) {
        const int src = g - (4 - d->ngroups);
        m.dim[g] = src >= 0 ? (uint64_t)d->dim[src] : 1;
        m.bs[g] = src >= 0 && d->dim[src] > 1 ? (uint64_t)d->b_stride[src] : 0;
    }
    m.sa = d->a_scale, m.za = (float)d->a_zp, m.sb = d->b_scale, m.zb = (float)d->b_zp;
    m.so = d->out_scale, m.zo = (float)d->out_zp, m.inv_so = 1.0f / d->out_scale;
    // div_by_scale(p, so, RN(1 / so)) == p / so for every product (sum) these records can give (mul_step.h, add_step.h)
    m.fma_div = mul_fma_ok(d->a_scale, d->a_zp, d->b_scale, d->b_zp, d->out_scale);
    if (OP == OP_ADD) m.fma_div = add_rec(d->a_scale, d->a_zp, d->b_scale, d->b_zp, d->out_scale, d->out_zp).fma_div;  // (the sum's bound)
    m.a_second = d->a_is_second ? 1 : 0;
    const int form = mul_form(OP, a_dev, b_dev, out_dev, d, &m.b_mode);
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(256);
    const uint64_t pieces = count / (f16 ? 8 : 16);
    if (form == MUL_VEC)
        hipLaunchKernelGGL((f16 ? mul_vec_kernel<true, OP> : mul_vec_kernel<false, OP>), dim3(grid_for(pieces)), block, 0, s, m);
    else if (form == MUL_ROW)
        hipLaunchKernelGGL((f16 ? mul_row_kernel<true, OP> : mul_row_kernel<false, OP>), dim3(grid_for(pieces)), block, 0, s, m);
    else
        hipLaunchKernelGGL((f16 ? mul_generic_kernel<true, OP> : mul_generic_kernel<false, OP>), dim3(grid_for(count)), block, 0, s, m);
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

}  // namespace shl

extern "C" int shl_mi355x_unary_lut_i8(const int8_t *input_dev, int8_t *output_dev, size_t count, const uint8_t *table,
                                       void *stream)
{
    using namespace shl;
    if (!input_dev || !output_dev || !table) {
        set_error("unary_lut_i8: NULL argument");
        return SHL_MI355X_EINVAL;
    }
    if ((int64_t)count < 0) {
        set_error("unary_lut_i8: negative count");
        return SHL_MI355X_EINVAL;
    }
    if (overlaps(output_dev, count, input_dev, count)) {
        set_error("unary_lut_i8: the output overlaps the input");
        return SHL_MI355X_EINVAL;
    }
    if (count == 0) return SHL_MI355X_OK;
    Lut256 tab;
    memcpy(tab.w, table, 256);
    hipStream_t s = (hipStream_t)stream;
    if ((((uintptr_t)input_dev | (uintptr_t)output_dev) & 15) == 0)
        hipLaunchKernelGGL(unary_lut_i8_vec_kernel, dim3(grid_for(count / 16)), dim3(256), 0, s, tab, input_dev, output_dev, count);
    else
        hipLaunchKernelGGL(unary_lut_i8_byte_kernel, dim3(grid_for(count)), dim3(256), 0, s, tab, input_dev, output_dev, count);
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

extern "C" const char *shl_mi355x_unary_lut_i8_kernel_name(const void *input_dev, const void *output_dev)
{
    return (((uintptr_t)input_dev | (uintptr_t)output_dev) & 15) == 0 ? "unary_lut_i8_vec" : "unary_lut_i8_byte";
}

extern "C" int shl_mi355x_unary_f16(const uint16_t *input_dev, uint16_t *output_dev, size_t count, int32_t kind, float alpha,
                                    void *stream)
{
    using namespace shl;
    if (!input_dev || !output_dev) {
        set_error("unary_f16: NULL argument");
        return SHL_MI355X_EINVAL;
    }
    if (kind < SHL_MI355X_UNARY_SIGMOID || kind > SHL_MI355X_UNARY_LEAKY_RELU) {
        set_error("unary_f16: unknown kind %d", (int)kind);
        return SHL_MI355X_EINVAL;
    }
    if ((int64_t)count < 0 || count > (size_t)1 << 60) {
        set_error("unary_f16: negative count");
        return SHL_MI355X_EINVAL;
    }
    if (overlaps(output_dev, 2 * count, input_dev, 2 * count)) {
        set_error("unary_f16: the output overlaps the input");
        return SHL_MI355X_EINVAL;
    }
    if (count == 0) return SHL_MI355X_OK;
    const dim3 grid(grid_for(count)), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (kind) {
        case SHL_MI355X_UNARY_SIGMOID:
            hipLaunchKernelGGL(unary_f16_kernel<SHL_MI355X_UNARY_SIGMOID>, grid, block, 0, s, input_dev, output_dev, count, alpha);
            break;
        case SHL_MI355X_UNARY_HARD_SIGMOID:
            hipLaunchKernelGGL(unary_f16_kernel<SHL_MI355X_UNARY_HARD_SIGMOID>, grid, block, 0, s, input_dev, output_dev, count, alpha);
            break;
        case SHL_MI355X_UNARY_SILU:
            hipLaunchKernelGGL(unary_f16_kernel<SHL_MI355X_UNARY_SILU>, grid, block, 0, s, input_dev, output_dev, count, alpha);
            break;
        default:
            hipLaunchKernelGGL(unary_f16_kernel<SHL_MI355X_UNARY_LEAKY_RELU>, grid, block, 0, s, input_dev, output_dev, count, alpha);
            break;
    }
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

extern "C" const char *shl_mi355x_mul_kernel_name(const struct shl_mi355x_mul_desc *d, const void *a_dev, const void *b_dev,
                                                  const void *out_dev)
{
    return shl::bcast_kernel_name(shl::OP_MUL, d, a_dev, b_dev, out_dev);
}

extern "C" int shl_mi355x_mul(const void *a_dev, const void *b_dev, void *out_dev, const struct shl_mi355x_mul_desc *d,
                              void *stream)
{
    return shl::bcast_launch<shl::OP_MUL>("mul", a_dev, b_dev, out_dev, d, stream);
}

extern "C" const char *shl_mi355x_add_bcast_kernel_name(const struct shl_mi355x_mul_desc *d, const void *a_dev, const void *b_dev,
                                                        const void *out_dev)
{
    return shl::bcast_kernel_name(shl::OP_ADD, d, a_dev, b_dev, out_dev);
}

extern "C" int shl_mi355x_add_bcast(const void *a_dev, const void *b_dev, void *out_dev, const struct shl_mi355x_mul_desc *d,
                                    void *stream)
{
    return shl::bcast_launch<shl::OP_ADD>("add_bcast", a_dev, b_dev, out_dev, d, stream);
}

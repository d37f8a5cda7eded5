// pool_softmax.hip -- the MobileNet tail between the last convolution and the classifier output:
// global average pooling and softmax on quantised int8 / binary16 tensors.
//
// Both follow the reference's "dequantise -> fp32 op -> requantise" callbacks
// (shl_ref_siso_callback_base, source/reference/utils.c:609-621) literally, including the ORDER of
// the fp32 operations, so that results agree bit for bit with the C reference for any scales:
//   global_avgpool2d  shl_ref_global_avgpool2d_f32 -> shl_ref_avgpool2d_{nhwc,nchw}_f32
//                     (global_averagepool.c:21-44, averagepool.c:21-119): total += x in (y, x)
//                     order in fp32, average = total / count.
//                     One thread per (image, channel) walks its H*W values in that order; NHWC
//                     reads are coalesced across the channel threads.  Tiny next to the convolutions
//                     (MobileNetV1: 50 KB in, 1 KB out).
//   softmax           shl_ref_softmax_f32 (softmax.c:21-66): max over the axis, then
//                     acc(float) += exp(double(x - max)) in index order, then
//                     float(exp(double(x - max)) / acc).  One block per (outer, inner) row: the
//                     max and the exponentials are computed in parallel (order-independent); the
//                     float running sum is reproduced EXACTLY by a wave-parallel scan (see
//                     running_sum_exact in softmax_step.h, which holds every step the fused attention kernel
//                     of attention.hip runs as well).
#include <stdlib.h>

#include "common.h"
#include "softmax_step.h"  // load_dequant / store_requant, softmax_exp, running_sum_exact

namespace shl {

__global__ __launch_bounds__(256) void global_avgpool_kernel(const void *in, void *out, int dtype, int nhwc,
                                                             int64_t nc, int C, int HW, float si, float zi,
                                                             float so, float zo)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (n, c), c fastest
    if (i >= nc) return;
    const int64_t n = i / C;
    const int c = (int)(i - n * C);
    const int64_t base = nhwc ? n * HW * C + c : (n * C + c) * (int64_t)HW;
    const int64_t step = nhwc ? C : 1;
    float total = 0.f;
    for (int p = 0; p < HW; ++p) total = __fadd_rn(total, load_dequant(in, base + p * step, dtype, si, zi));
    const float avg = __fdiv_rn(total, (float)HW);
    store_requant(out, i, avg, dtype, so, zo);  // output is [N, 1, 1, C] / [N, C, 1, 1]: index n*C + c
}

// int8 NHWC with at most 64 pixels (every MobileNet / ResNet tail): ONE channel per thread -- the reference's sum is a
// chain of H*W dependent fp32 additions per channel, so the channels are all the parallelism there is (1 024 threads for
// MobileNetV1; round 4 ran four such chains per thread).  A thread requests ALL the H*W dwords that hold its channel up
// front (one memory round trip; the four threads of a dword share the load) and then adds its byte of each in the
// reference's (y, x) order.
__global__ __launch_bounds__(64) void global_avgpool_nhwc_i8_kernel(const void *in, void *out, int64_t nc, int C, int HW,
                                                                    float si, float zi, float so, float zo)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (n, c), c fastest
    if (i >= nc) return;
    const int64_t n = i / C;
    const int c = (int)(i - n * C);
    const int cgroups = C >> 2;
    const uint32_t *src = static_cast<const uint32_t *>(in) + n * HW * cgroups + (c >> 2);
    const int sh = 8 * (c & 3);
    uint32_t v[64];
#pragma unroll
    for (int p = 0; p < 64; ++p)
        if (p < HW) v[p] = src[(int64_t)p * cgroups];
    float total = 0.f;
#pragma unroll
    for (int p = 0; p < 64; ++p) {
        if (p < HW) {
            const float x = __fmul_rn(__fsub_rn((float)(int8_t)(v[p] >> sh), zi), si);
            total = __fadd_rn(total, x);
        }
    }
    const int q = sat8_from_float(__fadd_rn(rintf(__fdiv_rn(__fdiv_rn(total, (float)HW), so)), zo));
    static_cast<int8_t *>(out)[i] = (int8_t)q;
}

// The literal loop on one lane (SHL_MI355X_SOFTMAX_SEQ=1, shl_mi355x_debug_running_sum): `acc_exp += exp(...)`, a double
// add rounded to float every step.
__device__ __forceinline__ float running_sum_literal(const double *e, int cnt)
{
    float acc = 0.f;
    int j = 0;
    for (; j + 8 <= cnt; j += 8) {  // eight LDS reads in flight, then the dependent chain
        double b[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) b[k] = e[j + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc = (float)((double)acc + b[k]);
    }
    for (; j < cnt; ++j) acc = (float)((double)acc + e[j]);
    return acc;
}

constexpr int SOFTMAX_MAX_CNT = 8192;  // doubles parked in LDS: 64 KiB

// Tests only (shl_mi355x_debug_running_sum): one workgroup parks the caller's terms in LDS the way softmax_kernel does
// (256 zeros behind them) and runs one of the two forms of the running sum on them.
__global__ __launch_bounds__(256) void running_sum_debug_kernel(const double *terms, int cnt, int literal, float *sum)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *e = reinterpret_cast<double *>(smem);  // [cnt + 256]
    const int tid = threadIdx.x;
    for (int j = tid; j < cnt; j += 256) e[j] = terms[j];
    e[cnt + tid] = 0.0;
    __syncthreads();
    if (literal) {
        if (tid == 0) *sum = running_sum_literal(e, cnt);
    } else if (tid < 64) {
        const float acc = running_sum_exact(e, cnt, tid);
        if (tid == 0) *sum = acc;
    }
}

// -DSHL_SM_TRACE=1 (tools/dev): s_memtime of thread 0 of row 0 at the phase boundaries of softmax_kernel
#ifndef SHL_SM_TRACE
#define SHL_SM_TRACE 0
#endif
#if SHL_SM_TRACE
static __device__ unsigned long long g_sm_trace[8];
#define SM_STAMP(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_sm_trace[k] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define SM_STAMP(k) do { } while (0)
#endif

__global__ __launch_bounds__(256) void softmax_kernel(const void *in, void *out, int dtype, int cnt,
                                                      int64_t inner, float si, float zi, float so, float zo, int seq_sum)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *e = reinterpret_cast<double *>(smem);          // [cnt + 256]: 256 zeros behind the row (running_sum_exact)
    float *red = reinterpret_cast<float *>(e + cnt + 256); // [256]
    const int64_t row = blockIdx.x;                         // outer * inner + k
    const int64_t o = row / inner, k = row - o * inner;
    const int64_t base = o * cnt * inner + k;
    const int tid = threadIdx.x;
    e[cnt + tid] = 0.0;
    SM_STAMP(0);
    // max (fmax over floats: exact whatever the order)
    float m = -3.402823466e+38f;
    for (int j = tid; j < cnt; j += 256) m = fmaxf(m, load_dequant(in, base + j * inner, dtype, si, zi));
    // wave maximum on DPP (inclusive max-scan, lane 63 holds the result), then one LDS hand-over of the four
    // wave results instead of an eight-barrier tree
#define SHL_MAX_DPP(CTRL, ROWS) \
    m = fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(m), __float_as_int(m), CTRL, ROWS, 0xf, false)))
    SHL_MAX_DPP(0x111, 0xf);
    SHL_MAX_DPP(0x112, 0xf);
    SHL_MAX_DPP(0x114, 0xf);
    SHL_MAX_DPP(0x118, 0xf);
    SHL_MAX_DPP(0x142, 0xa);
    SHL_MAX_DPP(0x143, 0xc);
#undef SHL_MAX_DPP
    if ((tid & 63) == 63) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    SM_STAMP(1);
    // int8: the row holds at most 256 distinct values -- thread t evaluates the exponential (and, below, the quotient and its
    // requantisation) of value t - 128 ONCE, the elements look theirs up (the same operations on the same operands as per
    // element: bit-identical; one f64 exp and one f64 division per thread instead of cnt / 256 of each)
    double *const lut_e = reinterpret_cast<double *>(red + 256);     // [256]
    int8_t *const lut_q = reinterpret_cast<int8_t *>(lut_e + 256);   // [256]
    uint8_t *const xb = reinterpret_cast<uint8_t *>(lut_q + 256);    // [cnt]: the row's bytes + 128 (the last pass reads them from LDS)
    const bool lut = dtype == SHL_MI355X_I8;
    if (lut) {
        lut_e[tid] = softmax_exp(dequant_i8(tid - 128, zi, si), m);  // load_dequant of the byte value tid - 128
        __syncthreads();
        for (int j = tid; j < cnt; j += 256) {
            const int v = (int)static_cast<const int8_t *>(in)[base + j * inner] + 128;
            xb[j] = (uint8_t)v;
            e[j] = lut_e[v];
        }
    } else {
        for (int j = tid; j < cnt; j += 256)
            e[j] = softmax_exp(load_dequant(in, base + j * inner, dtype, si, zi), m);
    }
    __syncthreads();
    SM_STAMP(2);
    if (seq_sum) {
        if (tid == 0) red[0] = running_sum_literal(e, cnt);
    } else if (tid < 64) {
        const float acc = running_sum_exact(e, cnt, tid);
        if (tid == 0) red[0] = acc;
    }
    __syncthreads();
    SM_STAMP(3);
    const double acc = (double)red[0];
    if (lut) {
        lut_q[tid] = (int8_t)requant_i8((float)(lut_e[tid] / acc), so, zo);  // store_requant's int8 branch
        __syncthreads();
        for (int j = tid; j < cnt; j += 256)
            static_cast<int8_t *>(out)[base + j * inner] = lut_q[xb[j]];
    } else {
        for (int j = tid; j < cnt; j += 256) store_requant(out, base + j * inner, (float)(e[j] / acc), dtype, so, zo);
    }
    SM_STAMP(4);
}

}  // namespace shl

#if SHL_SM_TRACE
extern "C" int shl_mi355x_debug_sm_trace(unsigned long long *host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(shl::g_sm_trace), 64) == hipSuccess ? 0 : -1;
}
#endif

extern "C" int shl_mi355x_debug_running_sum(const double *terms_host, int32_t count, int32_t literal, float *sum_host)
{
    if (!terms_host || !sum_host || count < 1 || count > shl::SOFTMAX_MAX_CNT) {
        shl::set_error("debug_running_sum: invalid argument");
        return SHL_MI355X_EINVAL;
    }
    double *d_terms = nullptr;
    float *d_sum = nullptr;
    SHL_HIP(hipMalloc((void **)&d_terms, (size_t)count * 8));
    if (hipMalloc((void **)&d_sum, 4) != hipSuccess) {
        (void)hipFree(d_terms);
        return shl::hip_fail(hipErrorOutOfMemory, "hipMalloc");
    }
    int rc = SHL_MI355X_OK;
    const size_t lds = ((size_t)count + 256) * 8;  // e[count + 256]
    static shl::LdsOptIn opted_in;
    if (lds > 48 * 1024) shl::lds_opt_in(opted_in, reinterpret_cast<const void *>(shl::running_sum_debug_kernel), 96 * 1024);
    hipError_t e = hipMemcpy(d_terms, terms_host, (size_t)count * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_sum, 0, 4);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(shl::running_sum_debug_kernel, dim3(1), dim3(256), lds, nullptr, d_terms, (int)count,
                           literal ? 1 : 0, d_sum);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(sum_host, d_sum, 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = shl::hip_fail(e, "debug_running_sum");
    (void)hipFree(d_terms);
    (void)hipFree(d_sum);
    return rc;
}

extern "C" int shl_mi355x_global_avgpool2d(const void *input_dev, void *output_dev, int32_t dtype, int32_t layout,
                                           int32_t batch, int32_t channels, int32_t pixels, float in_scale,
                                           int32_t in_zp, float out_scale, int32_t out_zp, void *stream)
{
    if (!input_dev || !output_dev || batch < 0 || channels <= 0 || pixels <= 0 ||
        (dtype != SHL_MI355X_I8 && dtype != SHL_MI355X_F16) || (layout != SHL_MI355X_NHWC && layout != SHL_MI355X_NCHW)) {
        shl::set_error("global_avgpool2d: invalid argument");
        return SHL_MI355X_EINVAL;
    }
    const int64_t nc = (int64_t)batch * channels;
    if (nc == 0) return SHL_MI355X_OK;
    if (dtype == SHL_MI355X_I8 && layout == SHL_MI355X_NHWC && channels % 4 == 0 && pixels <= 64) {
        // 64 threads per workgroup: MobileNetV1's 1024 channels spread over 16 CUs
        hipLaunchKernelGGL(shl::global_avgpool_nhwc_i8_kernel, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0,
                           (hipStream_t)stream, input_dev, output_dev, nc, (int)channels, (int)pixels,
                           in_scale, (float)in_zp, out_scale, (float)out_zp);
        SHL_HIP(hipGetLastError());
        return SHL_MI355X_OK;
    }
    hipLaunchKernelGGL(shl::global_avgpool_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       input_dev, output_dev, (int)dtype, layout == SHL_MI355X_NHWC ? 1 : 0, nc, (int)channels,
                       (int)pixels, in_scale, (float)in_zp, out_scale, (float)out_zp);
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

extern "C" int shl_mi355x_softmax(const void *input_dev, void *output_dev, int32_t dtype, int64_t outer, int32_t count,
                                  int64_t inner, float in_scale, int32_t in_zp, float out_scale, int32_t out_zp,
                                  void *stream)
{
    if (!input_dev || !output_dev || outer < 0 || inner <= 0 || count <= 0 ||
        (dtype != SHL_MI355X_I8 && dtype != SHL_MI355X_F16)) {
        shl::set_error("softmax: invalid argument");
        return SHL_MI355X_EINVAL;
    }
    if (count > shl::SOFTMAX_MAX_CNT) {
        shl::set_error("softmax: axis length %d exceeds %d", (int)count, shl::SOFTMAX_MAX_CNT);
        return SHL_MI355X_ENOTSUP;
    }
    const int64_t rows = outer * inner;
    if (rows == 0) return SHL_MI355X_OK;
    if (rows > 0x7FFFFFFF) {
        shl::set_error("softmax: too many rows");
        return SHL_MI355X_ENOTSUP;
    }
    const size_t lds = ((size_t)count + 256) * 8 + 256 * 4 + 256 * 8 + 256 + (size_t)count;  // e[count + 256] | red[256] | lut_e[256] | lut_q[256] | xb[count]
    static shl::LdsOptIn opted_in;
    if (lds > 48 * 1024) shl::lds_opt_in(opted_in, reinterpret_cast<const void *>(shl::softmax_kernel), 96 * 1024);
    static const char *seq_env = getenv("SHL_MI355X_SOFTMAX_SEQ");  // "1": the literal one-lane running sum (A/B, tests)
    hipLaunchKernelGGL(shl::softmax_kernel, dim3((unsigned)rows), dim3(256), lds, (hipStream_t)stream, input_dev,
                       output_dev, (int)dtype, (int)count, inner, in_scale, (float)in_zp, out_scale, (float)out_zp,
                       seq_env && seq_env[0] == '1' ? 1 : 0);
    SHL_HIP(hipGetLastError());
    return SHL_MI355X_OK;
}

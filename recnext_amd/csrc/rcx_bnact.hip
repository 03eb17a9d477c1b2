// The two BatchNorms of a channel mixer in a training step, each with what follows it as its epilogue (lsnet/model/recattn.py:199-205 mlp, :240-251 and
// :254-263 the blocks' `x + drop_path(channel_mixer(.))`, :208-223 the stem's ConvNorm -> GELU pairs; model/recnext.py:125-171 the same for M / A):
//   GELU   z   = gelu(BN(u))            the exact (erf) GELU of the batch-statistics BatchNorm; y = BN(u) is never stored, the backward forms it again from u
//   ADD    out = r + s[n] BN(u)         the residual add with the optional per-sample float32 DropPath scale s (NULL: 1); r and out (and the backward's g)
//                                       are of u's type or float32 (the autocast step of T / S / B carries a float32 residual beside 16-bit mixers)
// u is R x C, R = N H W rows of C contiguous channels, float32 / bf16 / f16; all arithmetic float32; the operand model, both access paths (16 bytes where
// C % V == 0 and the pointers allow, element-wide otherwise) and the grid rules are rcx_bn.hip's (rcx_bn.h), so repeat launches are bit-identical.
//   forward    k_bn_stats, k_bn_finalize (rcx_bn.hip's, launched as they are: bn::launch_stats), then
//              k_bnact_apply        y = fma(u - mean, invstd gamma, beta); GELU: z = y Phi(y); ADD: out = fma(s, y, r); one rounding, at the store
//   backward   k_bnact_bwd_stats    d per element -- GELU: gz (Phi(y) + y phi(y)), y formed again from u; ADD: s[n] g -- and the partials of sum d and
//                                   sum d xhat through the two-stage workspace scheme; then k_bn_bwd_finalize (bn::launch_bwd_finalize)
//              k_bnact_bwd_dx       d formed again, gu = gamma invstd (d - sum d / R - xhat sum(d xhat) / R); d is never stored
// No atomics, no waiting on another workgroup.
//
// Phi(y) = (1 + erf(y / sqrt 2)) / 2 on the device library's erff, a float32 erf good to a few ulps (an absolute error of some 1e-7, which the float64
// bounds of tests/test_bnact_gpu.py hold it to: they leave about 2e-6), and exactly +-1 once 1 - |erf| < 2^-25, |y| > 5.6, so that Phi is exactly 1 or 0
// there and gelu(y) exactly y or 0.  The 7.7e-5 fit of rcx_gelu.h (made for bf16 inference) is not used here.  phi(y) = exp(-y^2 / 2) / sqrt(2 pi) on the
// hardware exponential: its relative error grows with y^2 / 2 while y phi(y) falls as exp(-y^2 / 2), so the error of y phi(y) stays below 2e-8.
#include "rcx_common.h"
#include "rcx_launch.h"
#include "rcx_bn.h"

namespace rcx {
namespace bnact {

using namespace bn;

constexpr int kGelu = 0, kAdd = 1;

__device__ __forceinline__ float gelu_cdf(float y) { return fmaf(0.5f, erff(y * 0.70710678f), 0.5f); }
__device__ __forceinline__ float gelu_grad(float y) { return fmaf(y * 0.3989422804f, __expf(-0.5f * y * y), gelu_cdf(y)); }

// the DropPath scale of a row: s[row / HW], or 1
__device__ __forceinline__ float row_scale(const float* __restrict__ sc, unsigned row, unsigned HW) { return sc ? sc[row / HW] : 1.f; }

template <typename T, typename TR, int V, int EPI>
__global__ void __launch_bounds__(kThreads) k_bnact_apply(const T* __restrict__ u, const TR* __restrict__ r, const float* __restrict__ sc, TR* __restrict__ out,
                                                          const float* __restrict__ weight, const float* __restrict__ bias, const float* __restrict__ mean_,
                                                          const float* __restrict__ invstd_, int R, int C, int G, int RB, int HW)
{
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int g = blockIdx.x * TX + tx;
    if (g >= G) return;
    const size_t c0 = (size_t)g * V;
    float mean[V], scale[V], beta[V];
    load_vec<V>(mean_ + c0, mean);
    load_vec<V>(invstd_ + c0, scale);
    load_vec<V>(bias + c0, beta);
    {
        float w[V];
        load_vec<V>(weight + c0, w);
#pragma unroll
        for (int j = 0; j < V; ++j) scale[j] *= w[j];
    }
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    const size_t step = (size_t)TY * C;
    size_t off = ((size_t)r0 + ty) * C + c0;
    unsigned row = (unsigned)(r0 + ty);
#pragma unroll 2
    for (int i = 0; i < nrow; ++i, off += step, row += (unsigned)TY) {
        float v[V];
        load_vec<V>(u + off, v);
        if constexpr (EPI == kGelu) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float y = fmaf(v[j] - mean[j], scale[j], beta[j]);
                v[j] = y * gelu_cdf(y);
            }
        } else {
            float a[V];
            load_vec<V>(r + off, a);
            const float s = row_scale(sc, row, (unsigned)HW);
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = fmaf(s, fmaf(v[j] - mean[j], scale[j], beta[j]), a[j]);
        }
        store_vec<V>(out + off, v);
    }
}

// part: P x (sum d (C), sum d xhat (C))
template <typename T, typename TR, int V, int EPI>
__global__ void __launch_bounds__(kThreads) k_bnact_bwd_stats(const T* __restrict__ u, const TR* __restrict__ gout, const float* __restrict__ sc,
                                                              const float* __restrict__ weight, const float* __restrict__ bias, const float* __restrict__ mean_,
                                                              const float* __restrict__ invstd_, float* __restrict__ part, int R, int C, int G, int RB, int HW)
{
    __shared__ float sm[2 * V * kThreads];
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int g = blockIdx.x * TX + tx;
    const bool live = g < G;
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    float acc[2 * V];                                      // (sum d, sum d xhat) of channel j at 2 j, 2 j + 1
#pragma unroll
    for (int j = 0; j < 2 * V; ++j) acc[j] = 0.f;
    if (live) {
        const size_t c0 = (size_t)g * V;
        float mean[V], invstd[V];
        load_vec<V>(mean_ + c0, mean);
        load_vec<V>(invstd_ + c0, invstd);
        float scale[V], beta[V];
        if constexpr (EPI == kGelu) {
            load_vec<V>(weight + c0, scale);
            load_vec<V>(bias + c0, beta);
#pragma unroll
            for (int j = 0; j < V; ++j) scale[j] = invstd[j] * scale[j];
        }
        const size_t step = (size_t)TY * C;
        size_t off = ((size_t)r0 + ty) * C + c0;
        unsigned row = (unsigned)(r0 + ty);
#pragma unroll 2
        for (int i = 0; i < nrow; ++i, off += step, row += (unsigned)TY) {
            float v[V], d[V];
            load_vec<V>(u + off, v);
            load_vec<V>(gout + off, d);
            if constexpr (EPI == kGelu) {
#pragma unroll
                for (int j = 0; j < V; ++j) d[j] *= gelu_grad(fmaf(v[j] - mean[j], scale[j], beta[j]));
            } else {
                const float s = row_scale(sc, row, (unsigned)HW);
#pragma unroll
                for (int j = 0; j < V; ++j) d[j] *= s;
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                acc[2 * j] += d[j];
                acc[2 * j + 1] = fmaf(d[j], (v[j] - mean[j]) * invstd[j], acc[2 * j + 1]);
            }
        }
    }
    tree_sum<2 * V>(sm, acc, TX, TY, tx, ty);
    if (ty == 0 && live) {
        float sg[V], sgx[V];
#pragma unroll
        for (int j = 0; j < V; ++j) { sg[j] = acc[2 * j]; sgx[j] = acc[2 * j + 1]; }
        float* pm = part + (size_t)blockIdx.y * 2 * C + (size_t)g * V;
        store_vec<V>(pm, sg);
        store_vec<V>(pm + C, sgx);
    }
}

template <typename T, typename TR, int V, int EPI>
__global__ void __launch_bounds__(kThreads) k_bnact_bwd_dx(const T* __restrict__ u, const TR* __restrict__ gout, const float* __restrict__ sc, T* __restrict__ gu,
                                                           const float* __restrict__ weight, const float* __restrict__ bias, const float* __restrict__ mean_,
                                                           const float* __restrict__ invstd_, const float* __restrict__ sums, int R, int C, int G, int RB, int HW)
{
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int g = blockIdx.x * TX + tx;
    if (g >= G) return;
    const size_t c0 = (size_t)g * V;
    float k1[V], mean[V], invstd[V], c1[V], c2[V], beta[V];
    load_vec<V>(weight + c0, k1);
    load_vec<V>(invstd_ + c0, invstd);
    load_vec<V>(mean_ + c0, mean);
    load_vec<V>(sums + c0, c1);
    load_vec<V>(sums + C + c0, c2);
    if constexpr (EPI == kGelu) load_vec<V>(bias + c0, beta);
    const float ir = 1.f / (float)R;
#pragma unroll
    for (int j = 0; j < V; ++j) { k1[j] = invstd[j] * k1[j]; c1[j] *= ir; c2[j] *= ir; }
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    const size_t step = (size_t)TY * C;
    size_t off = ((size_t)r0 + ty) * C + c0;
    unsigned row = (unsigned)(r0 + ty);
#pragma unroll 2
    for (int i = 0; i < nrow; ++i, off += step, row += (unsigned)TY) {
        float v[V], d[V];
        load_vec<V>(u + off, v);
        load_vec<V>(gout + off, d);
        if constexpr (EPI == kGelu) {
#pragma unroll
            for (int j = 0; j < V; ++j) d[j] *= gelu_grad(fmaf(v[j] - mean[j], k1[j], beta[j]));
        } else {
            const float s = row_scale(sc, row, (unsigned)HW);
#pragma unroll
            for (int j = 0; j < V; ++j) d[j] *= s;
        }
#pragma unroll
        for (int j = 0; j < V; ++j) d[j] = k1[j] * (fmaf(-((v[j] - mean[j]) * invstd[j]), c2[j], d[j]) - c1[j]);
        store_vec<V>(gu + off, d);
    }
}


template <typename T, typename TR, int V, int EPI>
hipError_t fwd(const void* u, const void* r, const float* sc, void* out, const float* weight, const float* bias, float* run_mean, float* run_var,
               float* save_mean, float* save_invstd, float* ws, int R, int C, int HW, float momentum, float eps, hipStream_t s)
{
    if (hipError_t e = launch_stats(u, ws, save_mean, save_invstd, run_mean, run_var, R, C, momentum, eps, DtId<T>::id, V != 1, s); e != hipSuccess) return e;
    const Plan pa = apply_plan(R, C, V);
    hipLaunchKernelGGL((k_bnact_apply<T, TR, V, EPI>), grid_of(pa), block_of(pa), 0, s, (const T*)u, (const TR*)r, sc, (TR*)out, weight, bias,
                       (const float*)save_mean, (const float*)save_invstd, R, C, pa.G, pa.RB, HW);
    return hipGetLastError();
}

template <typename T, typename TR, int V, int EPI>
hipError_t bwd(const void* u, const void* gout, const float* sc, const float* weight, const float* bias, const float* mean, const float* invstd, void* gu,
               float* gweight, float* gbias, float* ws, int R, int C, int HW, hipStream_t s)
{
    const Plan ps = stats_plan(R, C, V);
    float* sums = gu ? ws + (size_t)ps.P * 2 * C : nullptr;
    hipLaunchKernelGGL((k_bnact_bwd_stats<T, TR, V, EPI>), grid_of(ps), block_of(ps), 0, s, (const T*)u, (const TR*)gout, sc, weight, bias, mean, invstd, ws,
                       R, C, ps.G, ps.RB, HW);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (hipError_t e = launch_bwd_finalize(ws, sums, gweight, gbias, C, ps.P, s); e != hipSuccess) return e;
    if (!gu) return hipSuccess;
    const Plan pa = apply_plan(R, C, V);
    hipLaunchKernelGGL((k_bnact_bwd_dx<T, TR, V, EPI>), grid_of(pa), block_of(pa), 0, s, (const T*)u, (const TR*)gout, sc, (T*)gu, weight, bias, mean, invstd,
                       (const float*)sums, R, C, pa.G, pa.RB, HW);
    return hipGetLastError();
}

// fn<T, TR, V, EPI>(args...): T of `dtype`, TR = T or (res32) float, V-wide where `wide`; GELU has no residual: TR = T
#define BNACT_V(fn, T, TR, EPI, wide, W, ...) ((wide) ? fn<T, TR, W, EPI>(__VA_ARGS__) : fn<T, TR, 1, EPI>(__VA_ARGS__))
#define BNACT_DISPATCH(fn, dtype, res32, epi, wide, ...)                                                                          \
    if ((epi) == bnact::kGelu) {                                                                                                         \
        switch (dtype) {                                                                                                          \
            case 0: return BNACT_V(fn, float, float, bnact::kGelu, wide, 4, __VA_ARGS__);                                                \
            case 1: return BNACT_V(fn, bf16_t, bf16_t, bnact::kGelu, wide, 8, __VA_ARGS__);                                              \
            case 2: return BNACT_V(fn, f16_t, f16_t, bnact::kGelu, wide, 8, __VA_ARGS__);                                                \
            default: return hipErrorInvalidValue;                                                                                 \
        }                                                                                                                         \
    }                                                                                                                             \
    switch (dtype) {                                                                                                              \
        case 0: return BNACT_V(fn, float, float, bnact::kAdd, wide, 4, __VA_ARGS__);                                                     \
        case 1: return (res32) ? BNACT_V(fn, bf16_t, float, bnact::kAdd, wide, 8, __VA_ARGS__) : BNACT_V(fn, bf16_t, bf16_t, bnact::kAdd, wide, 8, __VA_ARGS__); \
        case 2: return (res32) ? BNACT_V(fn, f16_t, float, bnact::kAdd, wide, 8, __VA_ARGS__) : BNACT_V(fn, f16_t, f16_t, bnact::kAdd, wide, 8, __VA_ARGS__);    \
        default: return hipErrorInvalidValue;                                                                                     \
    }

}  // namespace bnact

bool bn_act_applicable(long long N, long long H, long long W, long long C, int dtype, int rdtype, int epilogue)
{
    if (epilogue != bnact::kGelu && epilogue != bnact::kAdd) return false;
    if (rdtype != dtype && !(epilogue == bnact::kAdd && rdtype == 0)) return false;
    return batchnorm_applicable(N, H, W, C, dtype);
}

size_t bn_act_workspace_bytes(int R, int C, int dtype) { return batchnorm_workspace_bytes(R, C, dtype); }

hipError_t bn_act_train_fwd(const void* u, const void* r, const float* scale, void* out, const float* weight, const float* bias, float* run_mean, float* run_var,
                            float* save_mean, float* save_invstd, void* workspace, int R, int C, int HW, float momentum, float eps, int epilogue, int dtype,
                            int rdtype, hipStream_t s)
{
    const bool wide = bn::can_wide(C, dtype, {u, r, out, weight, bias, save_mean, save_invstd, workspace});
    BNACT_DISPATCH(bnact::fwd, dtype, rdtype != dtype, epilogue, wide, u, r, scale, out, weight, bias, run_mean, run_var, save_mean, save_invstd,
                   (float*)workspace, R, C, HW, momentum, eps, s)
}

hipError_t bn_act_train_bwd(const void* u, const void* g, const float* scale, const float* weight, const float* bias, const float* mean, const float* invstd,
                            void* gu, float* gweight, float* gbias, void* workspace, int R, int C, int HW, int epilogue, int dtype, int rdtype, hipStream_t s)
{
    const bool wide = bn::can_wide(C, dtype, {u, g, weight, bias, mean, invstd, gu, workspace});
    BNACT_DISPATCH(bnact::bwd, dtype, rdtype != dtype, epilogue, wide, u, g, scale, weight, bias, mean, invstd, gu, gweight, gbias, (float*)workspace, R, C, HW, s)
}

}  // namespace rcx

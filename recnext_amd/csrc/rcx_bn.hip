// BatchNorm2d of the training step on a dense NHWC tensor, forward and backward (lsnet/model/recattn.py:130-146 ConvNorm's nn.BatchNorm2d,
// engine.py:38-71 the step that runs it): x is R x C, R = N H W rows of C contiguous channels, float32 / bf16 / f16; every sum is per channel over the
// R rows, all arithmetic float32.
//
//   statistics  k_bn_stats       a workgroup of TX x TY threads owns TX groups of V adjacent channels and RB rows; a thread walks its rows TY apart
//                                with one V-wide load each (16 bytes where C and the pointers allow: V = 8 | 4, else V = 1) and sums (x - p) and
//                                (x - p)^2 against the pivot p = its first element: never sum x and sum x^2.  The threads' (n, mean, M2) are combined
//                                pairwise (Chan) through LDS in a fixed tree; one partial (mean, M2) a workgroup goes to the workspace.
//               k_bn_finalize    16 channels x 16 lanes: a lane combines a contiguous run of the P partials in index order, the 16 lanes in the same
//                                fixed tree -> save_mean, save_invstd and the running update (unbiased variance), as nn.BatchNorm2d.
//   apply       k_bn_apply       y = (x - mean) * (invstd * gamma) + beta, one rounding at the store; FROZEN: mean = running_mean and
//                                invstd = 1 / sqrt(running_var + eps) per thread (the eval-mode BatchNorm of a frozen backbone).
//   backward    k_bn_bwd_stats   partials of sum gy and sum gy * xhat, xhat = (x - mean) * invstd, same two stages (k_bn_bwd_finalize),
//               k_bn_bwd_dx      gx = gamma * invstd * (gy - sum gy / R - xhat * sum(gy xhat) / R), or gamma * invstd * gy with frozen statistics.
// P and the tiling are functions of (R, C, dtype) and of which of the two paths the pointers allow: repeat launches are bit-identical.  No atomics, no
// waiting on another workgroup; the finalize is a launch of its own.
#include "rcx_common.h"
#include "rcx_launch.h"
#include "rcx_bn.h"

namespace rcx {
namespace bn {

template <typename T, int V>
__global__ void __launch_bounds__(kThreads) k_bn_stats(const T* __restrict__ x, float* __restrict__ part, int R, int C, int G, int RB, int P)
{
    __shared__ float sm[2 * V * kThreads];
    __shared__ float sn[kThreads];
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int g = blockIdx.x * TX + tx;
    const bool live = g < G;
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    float piv[V], s1[V], s2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) piv[j] = s1[j] = s2[j] = 0.f;
    const int cnt = live ? nrow : 0;
    if (cnt) {
        const T* px = x + ((size_t)r0 + ty) * C + (size_t)g * V;
        load_vec<V>(px, piv);
        const size_t step = (size_t)TY * C;
#pragma unroll 4
        for (int i = 0; i < cnt; ++i, px += step) {
            float v[V];
            load_vec<V>(px, v);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float d = v[j] - piv[j];
                s1[j] += d;
                s2[j] = fmaf(d, d, s2[j]);
            }
        }
    }
    float n = (float)cnt, mean[V], m2[V];
    const float inv = cnt ? 1.f / (float)cnt : 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float a = s1[j] * inv;
        mean[j] = piv[j] + a;
        m2[j] = fmaxf(fmaf(-s1[j], a, s2[j]), 0.f);
    }
    for (int s = tree_top(TY); s >= 1; s >>= 1) {
        if (ty >= s && ty < 2 * s) {
            sn[ty * TX + tx] = n;
#pragma unroll
            for (int j = 0; j < V; ++j) { sm[BN_SLOT(2 * j)] = mean[j]; sm[BN_SLOT(2 * j + 1)] = m2[j]; }
        }
        __syncthreads();
        if (ty < s && ty + s < TY) {
            const float nb = sn[(ty + s) * TX + tx];
            float na = n;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                na = n;
                chan(na, mean[j], m2[j], nb, sm[BN_SLOT_AT(2 * j, ty + s)], sm[BN_SLOT_AT(2 * j + 1, ty + s)]);
            }
            n = na;
        }
        __syncthreads();
    }
    if (ty == 0 && live) {
        float* pm = part + (size_t)blockIdx.y * 2 * C + (size_t)g * V;
        store_vec<V>(pm, mean);
        store_vec<V>(pm + C, m2);
    }
}

// part: P x (mean (C), M2 (C)); chunk p holds min(R, (p + 1) RB) - p RB rows
__global__ void __launch_bounds__(kFin * kFin) k_bn_finalize(const float* __restrict__ part, float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                             float* __restrict__ run_mean, float* __restrict__ run_var, int R, int C, int RB, int P,
                                                             float momentum, float eps)
{
    __shared__ float sm[3 * kFin * kFin];
    const int TX = kFin, TY = kFin, tx = threadIdx.x, ty = threadIdx.y;
    const int c = blockIdx.x * kFin + tx;
    const int q = (P + kFin - 1) / kFin;
    float n = 0.f, mean = 0.f, m2 = 0.f;
    if (c < C) {
        const int pe = min(P, (ty + 1) * q);
        for (int p = ty * q; p < pe; ++p) {
            int r0;
            const float nb = (float)chunk_rows(R, RB, p, r0);
            chan(n, mean, m2, nb, part[(size_t)p * 2 * C + c], part[(size_t)p * 2 * C + C + c]);
        }
    }
    for (int s = kFin / 2; s >= 1; s >>= 1) {
        if (ty >= s && ty < 2 * s) { sm[BN_SLOT(0)] = n; sm[BN_SLOT(1)] = mean; sm[BN_SLOT(2)] = m2; }
        __syncthreads();
        if (ty < s) chan(n, mean, m2, sm[BN_SLOT_AT(0, ty + s)], sm[BN_SLOT_AT(1, ty + s)], sm[BN_SLOT_AT(2, ty + s)]);
        __syncthreads();
    }
    if (ty == 0 && c < C) {
        const float var = m2 / (float)R;
        save_mean[c] = mean;
        save_invstd[c] = 1.f / sqrtf(var + eps);
        if (run_mean) {
            run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mean;
            run_var[c] = (1.f - momentum) * run_var[c] + momentum * (m2 / (float)(R - 1));
        }
    }
}

// FROZEN: stat2 is the variance and the thread forms 1 / sqrt(var + eps); else stat2 is invstd.  save_invstd (FROZEN, optional): what the threads formed.
template <typename T, int V, bool FROZEN>
__global__ void __launch_bounds__(kThreads) k_bn_apply(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ weight, const float* __restrict__ bias,
                                                       const float* __restrict__ mean_, const float* __restrict__ stat2, float* __restrict__ save_invstd,
                                                       int R, int C, int G, int RB, float eps)
{
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int g = blockIdx.x * TX + tx;
    if (g >= G) return;
    const size_t c0 = (size_t)g * V;
    float mean[V], scale[V], beta[V];
    load_vec<V>(mean_ + c0, mean);
    load_vec<V>(stat2 + c0, scale);
    load_vec<V>(bias + c0, beta);
    if constexpr (FROZEN) {
#pragma unroll
        for (int j = 0; j < V; ++j) scale[j] = 1.f / sqrtf(scale[j] + eps);
        if (save_invstd && blockIdx.y == 0 && ty == 0) store_vec<V>(save_invstd + c0, scale);
    }
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
#pragma unroll 4
    for (int i = 0; i < nrow; ++i, off += step) {
        float v[V];
        load_vec<V>(x + off, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = fmaf(v[j] - mean[j], scale[j], beta[j]);
        store_vec<V>(y + off, v);
    }
}

// part: P x (sum gy (C), sum gy xhat (C))
template <typename T, int V>
__global__ void __launch_bounds__(kThreads) k_bn_bwd_stats(const T* __restrict__ x, const T* __restrict__ gy, const float* __restrict__ mean_,
                                                           const float* __restrict__ invstd_, float* __restrict__ part, int R, int C, int G, int RB)
{
    __shared__ float sm[2 * V * kThreads];
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int g = blockIdx.x * TX + tx;
    const bool live = g < G;
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    float sg[V], sgx[V];
#pragma unroll
    for (int j = 0; j < V; ++j) sg[j] = sgx[j] = 0.f;
    if (live) {
        const size_t c0 = (size_t)g * V;
        float mean[V], invstd[V];
        load_vec<V>(mean_ + c0, mean);
        load_vec<V>(invstd_ + c0, invstd);
        const size_t step = (size_t)TY * C;
        size_t off = ((size_t)r0 + ty) * C + c0;
#pragma unroll 4
        for (int i = 0; i < nrow; ++i, off += step) {
            float v[V], d[V];
            load_vec<V>(x + off, v);
            load_vec<V>(gy + off, d);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                sg[j] += d[j];
                sgx[j] = fmaf(d[j], (v[j] - mean[j]) * invstd[j], sgx[j]);
            }
        }
    }
    for (int s = tree_top(TY); s >= 1; s >>= 1) {
        if (ty >= s && ty < 2 * s) {
#pragma unroll
            for (int j = 0; j < V; ++j) { sm[BN_SLOT(2 * j)] = sg[j]; sm[BN_SLOT(2 * j + 1)] = sgx[j]; }
        }
        __syncthreads();
        if (ty < s && ty + s < TY) {
#pragma unroll
            for (int j = 0; j < V; ++j) { sg[j] += sm[BN_SLOT_AT(2 * j, ty + s)]; sgx[j] += sm[BN_SLOT_AT(2 * j + 1, ty + s)]; }
        }
        __syncthreads();
    }
    if (ty == 0 && live) {
        float* pm = part + (size_t)blockIdx.y * 2 * C + (size_t)g * V;
        store_vec<V>(pm, sg);
        store_vec<V>(pm + C, sgx);
    }
}

// sums: (sum gy (C), sum gy xhat (C)) for k_bn_bwd_dx, or NULL; gweight / gbias: the same two sums for the caller, or NULL
__global__ void __launch_bounds__(kFin * kFin) k_bn_bwd_finalize(const float* __restrict__ part, float* __restrict__ sums, float* __restrict__ gweight,
                                                                 float* __restrict__ gbias, int C, int P)
{
    __shared__ float sm[2 * kFin * kFin];
    const int TX = kFin, TY = kFin, tx = threadIdx.x, ty = threadIdx.y;
    const int c = blockIdx.x * kFin + tx;
    const int q = (P + kFin - 1) / kFin;
    float sg = 0.f, sgx = 0.f;
    if (c < C) {
        const int pe = min(P, (ty + 1) * q);
        for (int p = ty * q; p < pe; ++p) {
            sg += part[(size_t)p * 2 * C + c];
            sgx += part[(size_t)p * 2 * C + C + c];
        }
    }
    for (int s = kFin / 2; s >= 1; s >>= 1) {
        if (ty >= s && ty < 2 * s) { sm[BN_SLOT(0)] = sg; sm[BN_SLOT(1)] = sgx; }
        __syncthreads();
        if (ty < s) { sg += sm[BN_SLOT_AT(0, ty + s)]; sgx += sm[BN_SLOT_AT(1, ty + s)]; }
        __syncthreads();
    }
    if (ty == 0 && c < C) {
        if (sums) { sums[c] = sg; sums[C + c] = sgx; }
        if (gbias) gbias[c] = sg;
        if (gweight) gweight[c] = sgx;
    }
}

template <typename T, int V, bool BATCH>
__global__ void __launch_bounds__(kThreads) k_bn_bwd_dx(const T* __restrict__ x, const T* __restrict__ gy, T* __restrict__ gx, const float* __restrict__ weight,
                                                        const float* __restrict__ mean_, const float* __restrict__ invstd_, const float* __restrict__ sums,
                                                        int R, int C, int G, int RB)
{
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int g = blockIdx.x * TX + tx;
    if (g >= G) return;
    const size_t c0 = (size_t)g * V;
    float k1[V], mean[V], invstd[V], c1[V], c2[V];
    load_vec<V>(weight + c0, k1);
    load_vec<V>(invstd_ + c0, invstd);
#pragma unroll
    for (int j = 0; j < V; ++j) k1[j] *= invstd[j];
    if constexpr (BATCH) {
        load_vec<V>(mean_ + c0, mean);
        load_vec<V>(sums + c0, c1);
        load_vec<V>(sums + C + c0, c2);
        const float ir = 1.f / (float)R;
#pragma unroll
        for (int j = 0; j < V; ++j) { c1[j] *= ir; c2[j] *= ir; }
    }
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    const size_t step = (size_t)TY * C;
    size_t off = ((size_t)r0 + ty) * C + c0;
#pragma unroll 4
    for (int i = 0; i < nrow; ++i, off += step) {
        float d[V];
        load_vec<V>(gy + off, d);
        if constexpr (BATCH) {
            float v[V];
            load_vec<V>(x + off, v);
#pragma unroll
            for (int j = 0; j < V; ++j) d[j] = k1[j] * (fmaf(-((v[j] - mean[j]) * invstd[j]), c2[j], d[j]) - c1[j]);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) d[j] *= k1[j];
        }
        store_vec<V>(gx + off, d);
    }
}


// the two statistics launches: k_bn_stats, k_bn_finalize (train_fwd's, and through launch_stats those of the operators that bring their own apply)
template <typename T, int V>
hipError_t stats_fwd(const void* x, float* ws, float* save_mean, float* save_invstd, float* run_mean, float* run_var, int R, int C, float momentum, float eps,
                     hipStream_t s)
{
    const Plan ps = stats_plan(R, C, V);
    hipLaunchKernelGGL((k_bn_stats<T, V>), grid_of(ps), block_of(ps), 0, s, (const T*)x, ws, R, C, ps.G, ps.RB, ps.P);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bn_finalize, dim3((unsigned)((C + kFin - 1) / kFin)), dim3(kFin, kFin), 0, s, (const float*)ws, save_mean, save_invstd, run_mean, run_var,
                       R, C, ps.RB, ps.P, momentum, eps);
    return hipGetLastError();
}

template <typename T, int V>
hipError_t train_fwd(const void* x, void* y, const float* weight, const float* bias, float* run_mean, float* run_var, float* save_mean, float* save_invstd,
                     float* ws, int R, int C, float momentum, float eps, hipStream_t s)
{
    if (hipError_t e = stats_fwd<T, V>(x, ws, save_mean, save_invstd, run_mean, run_var, R, C, momentum, eps, s); e != hipSuccess) return e;
    const Plan pa = apply_plan(R, C, V);
    hipLaunchKernelGGL((k_bn_apply<T, V, false>), grid_of(pa), block_of(pa), 0, s, (const T*)x, (T*)y, weight, bias, (const float*)save_mean,
                       (const float*)save_invstd, (float*)nullptr, R, C, pa.G, pa.RB, eps);
    return hipGetLastError();
}

template <typename T, int V>
hipError_t frozen_fwd(const void* x, void* y, const float* weight, const float* bias, const float* mean, const float* var, float* save_invstd, int R, int C,
                      float eps, hipStream_t s)
{
    const Plan pa = apply_plan(R, C, V);
    hipLaunchKernelGGL((k_bn_apply<T, V, true>), grid_of(pa), block_of(pa), 0, s, (const T*)x, (T*)y, weight, bias, mean, var, save_invstd, R, C, pa.G, pa.RB, eps);
    return hipGetLastError();
}

template <typename T, int V>
hipError_t bwd(const void* x, const void* gy, const float* weight, const float* mean, const float* invstd, void* gx, float* gweight, float* gbias, float* ws,
               int R, int C, bool batch, hipStream_t s)
{
    const bool reduce = batch ? (gx || gweight || gbias) : (gweight || gbias);
    float* sums = nullptr;
    if (reduce) {
        const Plan ps = stats_plan(R, C, V);
        sums = batch && gx ? ws + (size_t)ps.P * 2 * C : nullptr;
        hipLaunchKernelGGL((k_bn_bwd_stats<T, V>), grid_of(ps), block_of(ps), 0, s, (const T*)x, (const T*)gy, mean, invstd, ws, R, C, ps.G, ps.RB);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        hipLaunchKernelGGL(k_bn_bwd_finalize, dim3((unsigned)((C + kFin - 1) / kFin)), dim3(kFin, kFin), 0, s, (const float*)ws, sums, gweight, gbias, C, ps.P);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (gx) {
        const Plan pa = apply_plan(R, C, V);
        if (batch)
            hipLaunchKernelGGL((k_bn_bwd_dx<T, V, true>), grid_of(pa), block_of(pa), 0, s, (const T*)x, (const T*)gy, (T*)gx, weight, mean, invstd, (const float*)sums,
                               R, C, pa.G, pa.RB);
        else
            hipLaunchKernelGGL((k_bn_bwd_dx<T, V, false>), grid_of(pa), block_of(pa), 0, s, (const T*)x, (const T*)gy, (T*)gx, weight, mean, invstd, (const float*)nullptr,
                               R, C, pa.G, pa.RB);
        return hipGetLastError();
    }
    return hipSuccess;
}


// stats_fwd for the operators that bring their own apply (rcx_bnact.hip)
hipError_t launch_stats(const void* x, float* ws, float* save_mean, float* save_invstd, float* run_mean, float* run_var, int R, int C, float momentum, float eps,
                        int dtype, bool wide, hipStream_t s)
{
    BN_DISPATCH(stats_fwd, dtype, wide, x, ws, save_mean, save_invstd, run_mean, run_var, R, C, momentum, eps, s)
}

// k_bn_bwd_finalize over the P partials another operator's reduction left in ws
hipError_t launch_bwd_finalize(const float* ws, float* sums, float* gweight, float* gbias, int C, int P, hipStream_t s)
{
    hipLaunchKernelGGL(k_bn_bwd_finalize, dim3((unsigned)((C + kFin - 1) / kFin)), dim3(kFin, kFin), 0, s, ws, sums, gweight, gbias, C, P);
    return hipGetLastError();
}

}  // namespace bn

bool batchnorm_applicable(long long N, long long H, long long W, long long C, int dtype)
{
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || dtype < 0 || dtype > 2) return false;
    const long long lim = 1ll << 31;
    if (N >= lim || H >= lim || W >= lim || C >= lim) return false;
    const long long nh = N * H;
    if (nh >= lim) return false;
    const long long r = nh * W;
    if (r >= lim) return false;
    return r * C < lim;
}

size_t batchnorm_workspace_bytes(int R, int C, int dtype)
{
    const bn::Plan w = bn::stats_plan(R, C, C % bn::wide_v(dtype) ? 1 : bn::wide_v(dtype)), n = bn::stats_plan(R, C, 1);
    const int P = w.P > n.P ? w.P : n.P;
    return sizeof(float) * ((size_t)P * 2 * C + 2 * (size_t)C);
}

hipError_t batchnorm_train_fwd(const void* x, void* y, const float* weight, const float* bias, float* run_mean, float* run_var, float* save_mean,
                               float* save_invstd, void* workspace, int R, int C, float momentum, float eps, int dtype, hipStream_t s)
{
    const bool wide = bn::can_wide(C, dtype, {x, y, weight, bias, save_mean, save_invstd, workspace});
    BN_DISPATCH(bn::train_fwd, dtype, wide, x, y, weight, bias, run_mean, run_var, save_mean, save_invstd, (float*)workspace, R, C, momentum, eps, s)
}

hipError_t batchnorm_frozen_fwd(const void* x, void* y, const float* weight, const float* bias, const float* mean, const float* var, float* save_invstd,
                                int R, int C, float eps, int dtype, hipStream_t s)
{
    const bool wide = bn::can_wide(C, dtype, {x, y, weight, bias, mean, var, save_invstd});
    BN_DISPATCH(bn::frozen_fwd, dtype, wide, x, y, weight, bias, mean, var, save_invstd, R, C, eps, s)
}

hipError_t batchnorm_bwd(const void* x, const void* gy, const float* weight, const float* mean, const float* invstd, void* gx, float* gweight, float* gbias,
                         void* workspace, int R, int C, bool batch_stats, int dtype, hipStream_t s)
{
    const bool wide = bn::can_wide(C, dtype, {x, gy, weight, mean, invstd, gx, workspace});
    BN_DISPATCH(bn::bwd, dtype, wide, x, gy, weight, mean, invstd, gx, gweight, gbias, (float*)workspace, R, C, batch_stats, s)
}

}  // namespace rcx

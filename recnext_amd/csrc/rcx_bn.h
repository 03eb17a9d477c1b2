// What the NHWC per-channel reduction kernels share (rcx_bn.hip: nn.BatchNorm2d; rcx_repdw.hip: RepVGGDW of a training step; rcx_dwbn.hip: a depthwise
// ConvNorm of a training step): the plan of a launch, the pivoted (n, mean, M2) combine, the row walk of a thread, the LDS slots of the fixed tree, the
// tree itself and the dtype dispatch.
#pragma once
#include <initializer_list>
#include "rcx_common.h"

namespace rcx {
namespace bn {

constexpr int kThreads = 256;
constexpr int kMaxTX = 64;            // column groups a workgroup
constexpr int kStatBlocks = 2048;     // workgroups of a reduction pass, at most: eight a CU
constexpr int kFin = 16;              // finalize: kFin channels x kFin lanes

struct Plan {
    int V, G, CT, TX, TY;             // channels a thread, column groups, channel tiles (grid.x), threads across and down
    int P, RB;                        // row chunks (grid.y) and rows a chunk
};

// rpt: rows a thread is given at least, while the chunks stay under cap
inline Plan make_plan(int R, int C, int V, int rpt, int cap)
{
    Plan p{};
    p.V = V;
    p.G = C / V;
    p.CT = (p.G + kMaxTX - 1) / kMaxTX;
    p.TX = (p.G + p.CT - 1) / p.CT;
    p.TY = kThreads / p.TX;
    const long long per = (long long)p.TY * rpt;
    long long want = (R + per - 1) / per;
    const long long lim = cap / p.CT > 1 ? cap / p.CT : 1;
    if (want > lim) want = lim;
    if (want < 1) want = 1;
    p.RB = (int)((R + want - 1) / want);
    p.RB = (p.RB + p.TY - 1) / p.TY * p.TY;
    p.P = (R + p.RB - 1) / p.RB;
    return p;
}

inline int wide_v(int dtype) { return dtype == 0 ? 4 : 8; }

// the 16-byte path: C a multiple of V and every pointer the kernels read V-wide aligned to 16 bytes
inline bool can_wide(int C, int dtype, std::initializer_list<const void*> ps)
{
    if (C % wide_v(dtype)) return false;
    for (const void* p : ps)
        if ((size_t)p & 15) return false;
    return true;
}

inline Plan stats_plan(int R, int C, int V) { return make_plan(R, C, V, 8, kStatBlocks); }
inline Plan apply_plan(int R, int C, int V) { return make_plan(R, C, V, 4, 32768); }

// (na, ma, Ma) <- (na, ma, Ma) + (nb, mb, Mb): counts, means and sums of squared deviations of two disjoint sets of rows
__device__ __forceinline__ void chan(float& na, float& ma, float& Ma, float nb, float mb, float Mb)
{
    if (nb == 0.f) return;
    if (na == 0.f) { na = nb; ma = mb; Ma = Mb; return; }
    const float n = na + nb, d = mb - ma, f = nb / n;
    ma = fmaf(d, f, ma);
    Ma = (Ma + Mb) + d * d * (na * f);
    na = n;
}

// rows [r0, r0 + nb) of chunk `chunk`, and how many of them thread row ty of TY walks (ints that never pass R: R may be close to 2^31)
__device__ __forceinline__ int chunk_rows(int R, int RB, int chunk, int& r0)
{
    r0 = chunk * RB;
    return R - r0 > RB ? RB : R - r0;
}
__device__ __forceinline__ int thread_rows(int nb, int ty, int TY) { return ty < nb ? (nb - ty + TY - 1) / TY : 0; }

__device__ __forceinline__ int tree_top(int n)
{
    int s = 1;
    while (s * 2 < n) s *= 2;
    return n > 1 ? s : 0;
}

// LDS of the reduction kernels: [j][ty][tx] floats, tx fastest (no bank conflicts across a row of threads)
#define BN_SLOT(j) (((j) * TY + ty) * TX + tx)
#define BN_SLOT_AT(j, yy) (((j) * TY + (yy)) * TX + tx)

// the fixed tree of k_bn_stats over the TY thread rows for one set of V (mean, M2); sm holds 2 V kThreads floats, sn kThreads.  Ends on a barrier.
template <int V>
__device__ __forceinline__ void tree_chan(float* sm, float* sn, float n, float (&mean)[V], float (&m2)[V], int TX, int TY, int tx, int ty)
{
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
}

// ... and for plain sums: K values a thread, added in the same tree.  sm holds K kThreads floats.  Ends on a barrier.
template <int K>
__device__ __forceinline__ void tree_sum(float* sm, float (&v)[K], int TX, int TY, int tx, int ty)
{
    for (int s = tree_top(TY); s >= 1; s >>= 1) {
        if (ty >= s && ty < 2 * s) {
#pragma unroll
            for (int j = 0; j < K; ++j) sm[BN_SLOT(j)] = v[j];
        }
        __syncthreads();
        if (ty < s && ty + s < TY) {
#pragma unroll
            for (int j = 0; j < K; ++j) v[j] += sm[BN_SLOT_AT(j, ty + s)];
        }
        __syncthreads();
    }
}

inline dim3 grid_of(const Plan& p) { return dim3((unsigned)p.CT, (unsigned)p.P); }
inline dim3 block_of(const Plan& p) { return dim3((unsigned)p.TX, (unsigned)p.TY); }

// F<T, V>::run(args...) on the element type of `dtype`, V-wide where `wide`
#define BN_DISPATCH(fn, dtype, wide, ...)                                                    \
    switch (dtype) {                                                                         \
        case 0: return (wide) ? fn<float, 4>(__VA_ARGS__) : fn<float, 1>(__VA_ARGS__);       \
        case 1: return (wide) ? fn<bf16_t, 8>(__VA_ARGS__) : fn<bf16_t, 1>(__VA_ARGS__);     \
        case 2: return (wide) ? fn<f16_t, 8>(__VA_ARGS__) : fn<f16_t, 1>(__VA_ARGS__);       \
        default: return hipErrorInvalidValue;                                                \
    }

// rcx_bn.hip's own launches for the operators that put another apply behind them (rcx_bnact.hip): k_bn_stats + k_bn_finalize exactly as
// batchnorm_train_fwd launches them (ws: batchnorm_workspace_bytes; `wide`: the caller's can_wide over every pointer it reads V-wide), and
// k_bn_bwd_finalize over P partials of (sum d (C), sum d xhat (C))
hipError_t launch_stats(const void* x, float* ws, float* save_mean, float* save_invstd, float* run_mean, float* run_var, int R, int C, float momentum, float eps,
                        int dtype, bool wide, hipStream_t s);
hipError_t launch_bwd_finalize(const float* ws, float* sums, float* gweight, float* gbias, int C, int P, hipStream_t s);

}  // namespace bn
}  // namespace rcx

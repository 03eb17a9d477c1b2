// The classifier head of every registered model (model/recnext.py forward_head + RecNextClassifier; lsnet/model/recattn.py:266-293 and RecNext's
// forward_head, :307-387) behind the last block: global average pool + linear, one launch, no workspace, float32 arithmetic throughout.
//     y[n][k] = b[k] + sum_c w[k][c] * ((1 / (H W)) sum_p x[n][p][c])
// k_head_pool_linear: a workgroup of 8 waves takes kImgs = 4 images and a tile of KT classes (KT a multiple of 32, chosen by the host from N and K).
//   1. The pool.  Thread (cv, s) sums the pixels p = s, s + S, ... of the 8 channels 8 cv .. 8 cv + 7 of each image (one 16-byte load a pixel for a
//      16-bit x, two for float32; S = 8 pixel slices, 4 when C > 512), four pixels of every image in flight and no load behind a branch, and
//      leaves its 8 float32 sums in LDS.  After a barrier one thread a (image, channel) adds the slices as the fixed tree
//      ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)) and multiplies by the float32 1 / (H W).
//   2. The product.  Lane l of every wave keeps the pooled means of the channels 8 (64 j + l) .. + 7, j < CH = ceil(C / 512), of the 4 images in
//      registers.  A wave walks the tile four classes at a time: a class's row of w is read once, coalesced (lane l the same 8 channels, 16 or 32
//      bytes; the next four rows are in flight under this group's sums), and widened exactly; the lane's 4 x 4 sums are fmaf chains over its own
//      8 CH channels, and the 64 lanes' sums are added as a tree over the lane bits 5, 4, 3, 2, 1, 0, the first four levels folding the 16
//      values so that every level moves half of what is left (15 + 2 cross-lane moves for 16 outputs).  bias is added last, and the output is
//      rounded once, at the store.
// Every output is therefore one fixed expression of its image's pixels and its class's row: the same bits at any N, at any position in the
// batch and in any class tile, and on every launch.  No atomics.  x is read ceil(K / KT) times and w ceil(N / 4) times.
// k_head_pool: step 1 alone for one image a workgroup, the means stored in x's type (num_classes = 0).
#include "rcx_common.h"
#include "rcx_launch.h"

namespace rcx {
namespace head {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kImgs = 4;                    // images a workgroup of the fused kernel takes
constexpr int kCls = 4;                     // classes a wave takes at a time: kImgs kCls = 16 sums a lane
constexpr int kMaxC = 1024;
constexpr int kPix = 4;                     // pixels of an image a pooling thread has in flight

struct PoolPlan {
    int nvec;                               // 8-channel vectors of a pixel: C / 8
    int lg;                                 // log2 of the vectors' power-of-two cover NV (8 .. 128)
    int S;                                  // pixel slices: 8, or 4 when NV = 128
};

PoolPlan pool_plan(int C)
{
    PoolPlan p;
    p.nvec = C / 8;
    p.lg = 3;
    while ((1 << p.lg) < p.nvec) ++p.lg;
    p.S = (1 << p.lg) > 64 ? 4 : 8;
    return p;
}

// the pooled means of IT images (from n0; zeros for an image past N) -> lds[(i S) C + c]; lds holds IT S C floats.  Ends in a barrier.
template <typename T, int IT>
__device__ __forceinline__ void pool_to_lds(const T* __restrict__ x, float* __restrict__ lds, int n0, int N, int P, int C, PoolPlan pp, float inv)
{
    const int t = threadIdx.x;
    const int cv = t & ((1 << pp.lg) - 1), s = t >> pp.lg;
    if (cv < pp.nvec && s < pp.S) {
        float a[IT][8];
#pragma unroll
        for (int i = 0; i < IT; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) a[i][j] = 0.f;
        const T* px = x + (size_t)n0 * P * C + cv * 8;
        // kPix pixels of every image at a time: IT kPix loads in flight; a slice's pixels are still added in pixel order (a pixel past P adds zeros)
#pragma unroll 1
        for (int p = s; p < P; p += kPix * pp.S) {
            float v[IT][kPix][8];
#pragma unroll
            for (int u = 0; u < kPix; ++u)
#pragma unroll
                for (int i = 0; i < IT; ++i) {
                    // no branch around a load (it would wait for each in turn): a pixel past P or an image past N reads the last one and is zeroed
                    const bool live = p + u * pp.S < P && n0 + i < N;
                    load_vec<8>(px + ((size_t)min(i, N - 1 - n0) * P + min(p + u * pp.S, P - 1)) * C, v[i][u]);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[i][u][j] = live ? v[i][u][j] : 0.f;
                }
#pragma unroll
            for (int u = 0; u < kPix; ++u)
#pragma unroll
                for (int i = 0; i < IT; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) a[i][j] += v[i][u][j];
        }
#pragma unroll
        for (int i = 0; i < IT; ++i) store_vec<8>(lds + (size_t)(i * pp.S + s) * C + cv * 8, a[i]);
    }
    __syncthreads();
    for (int e = t; e < IT * C; e += kThreads) {
        const int i = e / C, c = e - i * C;
        float* base = lds + (size_t)i * pp.S * C + c;
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = q < pp.S ? base[(size_t)q * C] : 0.f;
        base[0] = (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))) * inv;       // slice 0's slot: read and written by this thread alone
    }
    __syncthreads();
}

template <typename T>
__global__ void __launch_bounds__(kThreads) k_head_pool(const T* __restrict__ x, T* __restrict__ y, int N, int P, int C, PoolPlan pp, float inv)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int n = blockIdx.x;
    pool_to_lds<T, 1>(x, lds, n, N, P, C, pp, inv);
    for (int c = threadIdx.x; c < C; c += kThreads) {
        const float one[1] = {lds[c]};
        store_vec<1>(y + (size_t)n * C + c, one);
    }
}

// one half of a fold level: the lanes whose bit `mask` is clear keep lo and receive the partner's lo, the others keep hi and receive the partner's hi
__device__ __forceinline__ float fold(float lo, float hi, bool upper, int mask)
{
    const float keep = upper ? hi : lo, send = upper ? lo : hi;
    return keep + __shfl_xor(send, mask, 64);
}

template <typename T, typename WT, int CH>
__global__ void __launch_bounds__(kThreads) k_head_pool_linear(const T* __restrict__ x, const WT* __restrict__ w, const float* __restrict__ bias, T* __restrict__ y,
                                                                int N, int P, int C, int K, int KT, int ktiles, PoolPlan pp, float inv)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int kt = blockIdx.x % ktiles, n0 = (blockIdx.x / ktiles) * kImgs;
    pool_to_lds<T, kImgs>(x, lds, n0, N, P, C, pp, inv);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float pm[kImgs][CH][8];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        const int c0 = (j * 64 + lane) * 8;
#pragma unroll
        for (int i = 0; i < kImgs; ++i) {
            if (c0 < C) load_vec<8>(lds + (size_t)i * pp.S * C + c0, pm[i][j]);
            else {
#pragma unroll
                for (int u = 0; u < 8; ++u) pm[i][j][u] = 0.f;
            }
        }
    }

    const int kend = min(K, (kt + 1) * KT);
    // a group's rows of w: lane l its 8 CH channels of each of the 4 classes; zeros past C
    auto load_rows = [&](int kg, float (&dst)[kCls][CH][8]) {
#pragma unroll
        for (int q = 0; q < kCls; ++q)
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                // no branch around a load: a class past K reads the last row (its sums are not stored), a lane past C reads channel 0 and is zeroed
                const int c0 = (j * 64 + lane) * 8;
                load_vec<8>(w + (size_t)min(kg + q, K - 1) * C + (c0 < C ? c0 : 0), dst[q][j]);
#pragma unroll
                for (int u = 0; u < 8; ++u) dst[q][j][u] = c0 < C ? dst[q][j][u] : 0.f;
            }
    };
    float wn[kCls][CH][8];
    if (kt * KT + wave * kCls < kend) load_rows(kt * KT + wave * kCls, wn);
#pragma unroll 1
    for (int kg = kt * KT + wave * kCls; kg < kend; kg += kWaves * kCls) {
        float wv[kCls][CH][8];
#pragma unroll
        for (int q = 0; q < kCls; ++q)
#pragma unroll
            for (int j = 0; j < CH; ++j)
#pragma unroll
                for (int u = 0; u < 8; ++u) wv[q][j][u] = wn[q][j][u];
        if (kg + kWaves * kCls < kend) load_rows(kg + kWaves * kCls, wn);            // the next group's rows, in flight under this group's sums
        float acc[kImgs * kCls];
#pragma unroll
        for (int i = 0; i < kImgs; ++i)
#pragma unroll
            for (int q = 0; q < kCls; ++q) {
                float a = 0.f;
#pragma unroll
                for (int j = 0; j < CH; ++j)
#pragma unroll
                    for (int u = 0; u < 8; ++u) a = fmaf(wv[q][j][u], pm[i][j][u], a);
                acc[i * kCls + q] = a;
            }
        // the tree over the 64 lanes: index bit 3 goes with lane bit 5, bit 2 with 4, bit 1 with 3, bit 0 with 2; then lane bits 1 and 0
        const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8, b2 = lane & 4;
        float f8[8], f4[4], f2[2];
#pragma unroll
        for (int v = 0; v < 8; ++v) f8[v] = fold(acc[v], acc[v + 8], b5, 32);
#pragma unroll
        for (int v = 0; v < 4; ++v) f4[v] = fold(f8[v], f8[v + 4], b4, 16);
#pragma unroll
        for (int v = 0; v < 2; ++v) f2[v] = fold(f4[v], f4[v + 2], b3, 8);
        float r = fold(f2[0], f2[1], b2, 4);
        r += __shfl_xor(r, 2, 64);
        r += __shfl_xor(r, 1, 64);
        const int i = (b5 ? 2 : 0) + (b4 ? 1 : 0), q = (b3 ? 2 : 0) + (b2 ? 1 : 0);
        if ((lane & 3) == 0 && n0 + i < N && kg + q < K) {
            const float out[1] = {r + (bias ? bias[kg + q] : 0.f)};
            store_vec<1>(y + (size_t)(n0 + i) * K + kg + q, out);
        }
    }
}

// classes a workgroup takes: the largest of 256, 128, 64, 32 that still leaves a workgroup a CU, else 32
int class_tile(int N, int K)
{
    const long long tiles = (N + kImgs - 1) / kImgs;
    for (int kt = 256; kt > 32; kt >>= 1)
        if (tiles * ((K + kt - 1) / kt) >= 256) return kt;
    return 32;
}

template <typename T, typename WT>
hipError_t launch_linear(const void* x, const void* w, const float* bias, void* y, int N, int P, int C, int K, hipStream_t s)
{
    const PoolPlan pp = pool_plan(C);
    const int KT = class_tile(N, K), ktiles = (K + KT - 1) / KT;
    const unsigned grid = (unsigned)((size_t)((N + kImgs - 1) / kImgs) * ktiles);
    const size_t lds = sizeof(float) * kImgs * pp.S * C;
    const float inv = 1.0f / (float)P;
    if (C <= 512)
        hipLaunchKernelGGL((k_head_pool_linear<T, WT, 1>), dim3(grid), dim3(kThreads), lds, s, (const T*)x, (const WT*)w, bias, (T*)y, N, P, C, K, KT, ktiles, pp, inv);
    else
        hipLaunchKernelGGL((k_head_pool_linear<T, WT, 2>), dim3(grid), dim3(kThreads), lds, s, (const T*)x, (const WT*)w, bias, (T*)y, N, P, C, K, KT, ktiles, pp, inv);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_pool(const void* x, void* y, int N, int P, int C, hipStream_t s)
{
    const PoolPlan pp = pool_plan(C);
    hipLaunchKernelGGL((k_head_pool<T>), dim3((unsigned)N), dim3(kThreads), sizeof(float) * pp.S * C, s, (const T*)x, (T*)y, N, P, C, pp, 1.0f / (float)P);
    return hipGetLastError();
}

}  // namespace head

bool global_pool_applicable(long long N, long long H, long long W, long long C, int dtype)
{
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || dtype < 0 || dtype > 2) return false;
    const long long lim = 1ll << 31;
    if (N >= lim || H >= lim || W >= lim || H * W >= lim || C % 8 || C > head::kMaxC) return false;
    return N * C < lim && H * W * C < lim && N * (H * W * C) < lim;
}

bool pool_head_applicable(long long N, long long H, long long W, long long C, long long K, int xdtype, int wdtype)
{
    if (!global_pool_applicable(N, H, W, C, xdtype) || K <= 0 || (wdtype != 0 && wdtype != xdtype)) return false;
    const long long lim = 1ll << 31;
    return K < lim && N * K < lim && K * C < lim && ((N + head::kImgs - 1) / head::kImgs) * ((K + 31) / 32) < lim;
}

hipError_t pool_head_fwd(const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int C, int K, int xdtype, int wdtype, hipStream_t s)
{
    if (!pool_head_applicable(N, H, W, C, K, xdtype, wdtype)) return hipErrorInvalidValue;
    const int P = H * W;
    switch (xdtype) {
        case 0: return head::launch_linear<float, float>(x, w, bias, y, N, P, C, K, s);
        case 1: return wdtype == 0 ? head::launch_linear<bf16_t, float>(x, w, bias, y, N, P, C, K, s) : head::launch_linear<bf16_t, bf16_t>(x, w, bias, y, N, P, C, K, s);
        case 2: return wdtype == 0 ? head::launch_linear<f16_t, float>(x, w, bias, y, N, P, C, K, s) : head::launch_linear<f16_t, f16_t>(x, w, bias, y, N, P, C, K, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t global_pool_fwd(const void* x, void* y, int N, int H, int W, int C, int dtype, hipStream_t s)
{
    if (!global_pool_applicable(N, H, W, C, dtype)) return hipErrorInvalidValue;
    switch (dtype) {
        case 0: return head::launch_pool<float>(x, y, N, H * W, C, s);
        case 1: return head::launch_pool<bf16_t>(x, y, N, H * W, C, s);
        case 2: return head::launch_pool<f16_t>(x, y, N, H * W, C, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rcx

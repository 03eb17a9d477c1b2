// The token half of a share block of the LSNet-style share-channel RecNeXt-T / S / B (lsnet/model/recattn_share_channel.py:8-15, :281-283,
// :302-304): r = RepVGGDW(x), t = r + cat(x1s), where x1s are the slice-mixer outputs of the blocks since the last share block.  Each of those
// is the first `split` channels of an earlier block's t, so the sources are read where they lie (pixels `stride` elements apart): no slice copy,
// no concatenation.  One launch on a wide grid, one thread per pixel and four channels; the nine taps in k_lt_rep's order (rcx_lstile.hip), so r
// has the same bits as every other token half's; t = the unrounded float32 r + the source, rounded once at its store.  No LDS, no atomics, no
// workspace.
#include "rcx_common.h"
#include "rcx_launch.h"

namespace rcx {
namespace {

constexpr int kShareThreads = 256;

struct ShareArgs {
    const float *w_rep, *b_rep;            // (3, 3, C), (C): the folded RepVGGDW
    const void* src[kLsShareMaxSrc];       // source j supplies t's channels [j split, (j + 1) split)
    long long stride;                      // elements between two pixels of a source
    int N, H, W, C, split;
};

template <typename T>
__global__ void __launch_bounds__(kShareThreads) k_ls_share(const T* __restrict__ x, T* __restrict__ r, T* __restrict__ t, ShareArgs a)
{
    const int H = a.H, W = a.W, C = a.C;
    const int cv = C >> 2;
    const size_t total = (size_t)a.N * H * W * cv;
    const size_t i = (size_t)blockIdx.x * kShareThreads + threadIdx.x;
    if (i >= total) return;
    const int c = 4 * (int)(i % cv);
    const size_t pix = i / cv;
    const int px = (int)(pix % W);
    const int py = (int)((pix / W) % H);
    const size_t img = pix / ((size_t)H * W);
    float acc[4];
    load_vec<4>(a.b_rep + c, acc);
    for (int ky = 0; ky < 3; ++ky) {
        const int yy = py + ky - 1;
        if (yy < 0 || yy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int xx = px + kx - 1;
            if (xx < 0 || xx >= W) continue;
            float v[4], wt[4];
            load_vec<4>(x + ((img * H + yy) * W + xx) * C + c, v);
            load_vec<4>(a.w_rep + (ky * 3 + kx) * C + c, wt);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(wt[j], v[j], acc[j]);
        }
    }
    store_vec<4>(r + pix * C + c, acc);
    // split % 4 == 0: the four channels lie in one source
    const int j = c / a.split, cs = c - j * a.split;
    const T* sp = nullptr;
#pragma unroll
    for (int u = 0; u < kLsShareMaxSrc; ++u)       // a select chain: the by-value pointer array stays in registers
        if (u == j) sp = (const T*)a.src[u];
    float s4[4];
    load_vec<4>(sp + pix * (size_t)a.stride + cs, s4);
#pragma unroll
    for (int u = 0; u < 4; ++u) s4[u] += acc[u];
    store_vec<4>(t + pix * C + c, s4);
}

template <typename T>
hipError_t launch_share(const void* x, void* r, void* t, const ShareArgs& a, hipStream_t s)
{
    const size_t total = (size_t)a.N * a.H * a.W * (a.C >> 2);
    hipLaunchKernelGGL((k_ls_share<T>), dim3((unsigned)((total + kShareThreads - 1) / kShareThreads)), dim3(kShareThreads), 0, s, (const T*)x, (T*)r,
                       (T*)t, a);
    return hipGetLastError();
}

}  // namespace

bool ls_share_applicable(int B, int H, int W, int C, int split, int n_src, long long stride, int dtype)
{
    return B > 0 && H > 0 && W > 0 && C > 0 && split > 0 && C % 4 == 0 && split % 4 == 0 && n_src >= 1 && n_src <= kLsShareMaxSrc
           && (long long)n_src * split == C && stride >= split && stride % 4 == 0 && dtype >= 0 && dtype <= 2
           && (size_t)B * H * W * C < ((size_t)1 << 31);
}

hipError_t ls_share_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const void* const* srcs, int n_src, long long stride,
                        int B, int H, int W, int C, int split, int dtype, hipStream_t s)
{
    if (!ls_share_applicable(B, H, W, C, split, n_src, stride, dtype)) return hipErrorInvalidValue;
    ShareArgs a{};
    a.w_rep = w_rep;
    a.b_rep = b_rep;
    for (int j = 0; j < n_src; ++j) a.src[j] = srcs[j];
    a.stride = stride;
    a.N = B; a.H = H; a.W = W; a.C = C; a.split = split;
    switch (dtype) {
        case 0: return launch_share<float>(x, r, t, a, s);
        case 1: return launch_share<bf16_t>(x, r, t, a, s);
        case 2: return launch_share<f16_t>(x, r, t, a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rcx

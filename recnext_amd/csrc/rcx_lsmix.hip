// The token half of the LSNet-style RecNeXt-T / S / B blocks (lsnet/model/recattn.py:226-251), inference, BatchNorms folded:
//     r = RepVGGDW(x) = dw3x3(x) + dw1x1(x) + x                       (:8-34; folded into ONE biased depthwise 3x3 conv)
//     t = cat(mixer(r[..., :Cs]), r[..., Cs:])                         (:226-237, PartialChannelOperation)
// mixer = RecAttn2d (:115-127: conv5(r_s + nearest(LA(dw5s2(r_s))))) or LinearAttention3 (:89-112, at full resolution).
//
// Two launches, independent of each other (they write disjoint channels of r and t):
//   k_ls_pass   the passthrough channels [Cs, C): RepVGGDW on a wide grid (one thread per pixel and 4 channels), r and t both written;
//   k_ls_slice  one workgroup per image for the slice [0, Cs): RepVGGDW of the slice into LDS (and r), then the mixer entirely in LDS --
//               the stride-2 conv's plane d, the projections k and q (one buffer, k first), k^T v, mean(k), the normaliser -- and the
//               attention output added in place into the fine plane (each fine pixel has ONE nearest source, so one thread owns each
//               element), then the final conv from LDS to t.  Nothing of the slice but r goes through memory.
// float32 arithmetic throughout, every output rounded once at its store, every reduction in a fixed order (no atomics): deterministic,
// and an image's result does not depend on the batch around it.
#include "rcx_common.h"
#include "rcx_launch.h"

namespace rcx {
namespace {

constexpr int kSliceThreads = 512;
constexpr int kLdsLimit = 160 * 1024;

__device__ __forceinline__ float elu1(float a) { return a > 0.f ? a + 1.f : expm1f(a) + 1.f; }

// r = t = RepVGGDW(x) on channels [c0, C): w (3, 3, C) and b (C) float32 packs of the folded conv.
template <typename T>
__global__ void __launch_bounds__(256) k_ls_pass(const T* __restrict__ x, T* __restrict__ r, T* __restrict__ t, const float* __restrict__ w,
                                                 const float* __restrict__ b, int N, int H, int W, int C, int c0)
{
    const int cv = (C - c0) >> 2;
    const size_t total = (size_t)N * H * W * cv;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int g = (int)(i % cv);
    const size_t pix = i / cv;
    const int px = (int)(pix % W);
    const int py = (int)((pix / W) % H);
    const size_t img = pix / ((size_t)H * W);
    const int c = c0 + 4 * g;
    float acc[4];
    load_vec<4>(b + c, acc);
    for (int ky = 0; ky < 3; ++ky) {
        const int yy = py + ky - 1;
        if (yy < 0 || yy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int xx = px + kx - 1;
            if (xx < 0 || xx >= W) continue;
            float v[4], wt[4];
            load_vec<4>(x + ((img * H + yy) * W + xx) * C + c, v);
            load_vec<4>(w + (ky * 3 + kx) * C + c, wt);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(wt[j], v[j], acc[j]);
        }
    }
    store_vec<4>(r + pix * C + c, acc);
    store_vec<4>(t + pix * C + c, acc);
}

struct SliceArgs {
    const float *w_rep, *b_rep;     // (3, 3, C), (C): the folded RepVGGDW
    const float *w_dn, *b_dn;       // (5, 5, Cs), (Cs): RecAttn2d's stride-2 conv (RecAttn2d only)
    const float *wqT, *bq;          // (Kin, Cq), (Cq): the q projection, transposed
    const float *wkT, *bk;          // (Kin, Cq), (Cq): the k projection, transposed; reads v's channels [k_off, k_off + Kin)
    const float *w_pe, *b_pe;       // (3, 3, Cs), (Cs)
    const float *w_cv, *b_cv;       // (5, 5, Cs), (Cs): RecAttn2d's final conv (RecAttn2d only)
    int N, H, W, C, Cs, heads, Cq, Kin, k_off;
};

// LDS floats of one image: fine plane (Cs) + [coarse plane d (Cs)] + k / q (Cq) + k^T v (Cq x dv) + mean(k) (Cq) + normaliser (heads)
inline size_t slice_lds_floats(int attn, int H, int W, int Cs, int heads, int Cq)
{
    const size_t hw_f = (size_t)H * W;
    const size_t hw = attn ? (size_t)((H + 1) / 2) * ((W + 1) / 2) : hw_f;
    const size_t dv = (size_t)Cs / heads;
    return hw_f * Cs + (attn ? hw * Cs : 0) + hw * Cq + (size_t)Cq * dv + Cq + hw * heads;
}

// ATTN = 1: RecAttn2d (one workgroup per image); ATTN = 0: LinearAttention3 (v = the fine plane, no resize, no final conv)
template <typename T, int ATTN>
__global__ void __launch_bounds__(kSliceThreads) k_ls_slice(const T* __restrict__ x, T* __restrict__ r, T* __restrict__ t, SliceArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = a.H, W = a.W, C = a.C, Cs = a.Cs, Cq = a.Cq, heads = a.heads;
    const int HW = H * W;
    const int hc = ATTN ? (H + 1) / 2 : H, wc = ATTN ? (W + 1) / 2 : W;
    const int hw = hc * wc;
    const int dq = Cq / heads, dv = Cs / heads;
    const size_t img = blockIdx.x;
    const int tid = threadIdx.x;
    float* rs = lds;                                   // HW x Cs
    float* v = ATTN ? rs + (size_t)HW * Cs : rs;       // hw x Cs: d (RecAttn2d) or the fine plane itself (LinearAttention3)
    float* kq = ATTN ? v + (size_t)hw * Cs : rs + (size_t)HW * Cs;     // hw x Cq: k, then q
    float* kv = kq + (size_t)hw * Cq;                  // heads x dq x dv
    float* km = kv + (size_t)Cq * dv;                  // Cq
    float* den = km + Cq;                              // hw x heads
    const T* xi = x + img * HW * C;
    T* ri = r + img * HW * C;
    T* ti = t + img * HW * C;

    // 1. the slice of r = RepVGGDW(x): into LDS (float32) and to r (rounded once)
    const int cs4 = Cs >> 2;
    for (int e = tid; e < HW * cs4; e += kSliceThreads) {
        const int p = e / cs4, c = 4 * (e - p * cs4);
        const int py = p / W, px = p - py * W;
        float acc[4];
        load_vec<4>(a.b_rep + c, acc);
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = py + ky - 1;
            if (yy < 0 || yy >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = px + kx - 1;
                if (xx < 0 || xx >= W) continue;
                float xv[4], wt[4];
                load_vec<4>(xi + (size_t)(yy * W + xx) * C + c, xv);
                load_vec<4>(a.w_rep + (ky * 3 + kx) * C + c, wt);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(wt[j], xv[j], acc[j]);
            }
        }
        store_vec<4>(rs + (size_t)p * Cs + c, acc);
        store_vec<4>(ri + (size_t)p * C + c, acc);
    }
    __syncthreads();

    // 2. RecAttn2d: d = dw5 stride 2 (padding 2) of the slice
    if constexpr (ATTN) {
        for (int e = tid; e < hw * cs4; e += kSliceThreads) {
            const int q = e / cs4, c = 4 * (e - q * cs4);
            const int qy = q / wc, qx = q - qy * wc;
            float acc[4];
            load_vec<4>(a.b_dn + c, acc);
            for (int ky = 0; ky < 5; ++ky) {
                const int yy = 2 * qy + ky - 2;
                if (yy < 0 || yy >= H) continue;
                for (int kx = 0; kx < 5; ++kx) {
                    const int xx = 2 * qx + kx - 2;
                    if (xx < 0 || xx >= W) continue;
                    float sv[4], wt[4];
                    load_vec<4>(rs + (size_t)(yy * W + xx) * Cs + c, sv);
                    load_vec<4>(a.w_dn + (ky * 5 + kx) * Cs + c, wt);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = fmaf(wt[j], sv[j], acc[j]);
                }
            }
            store_vec<4>(v + (size_t)q * Cs + c, acc);
        }
        __syncthreads();
    }

    // 3. k = elu(W_k v + b_k) + 1
    for (int e = tid; e < hw * Cq; e += kSliceThreads) {
        const int m = e / Cq, o = e - m * Cq;
        const float* vm = v + (size_t)m * Cs + a.k_off;
        float acc = a.bk[o];
        for (int c = 0; c < a.Kin; ++c) acc = fmaf(a.wkT[(size_t)c * Cq + o], vm[c], acc);
        kq[e] = elu1(acc);
    }
    __syncthreads();

    // 4. kv[h][i][j] = sum_m (k[m][h dq + i] s) (v[m][h dv + j] s), s = n^-1/2;  km[o] = mean_m k[m][o]
    const float s = 1.0f / sqrtf((float)hw);
    for (int e = tid; e < Cq * dv; e += kSliceThreads) {
        const int hi = e / dv, j = e - hi * dv;        // hi = h dq + i
        const int h = hi / dq;
        float acc = 0.f;
        for (int m = 0; m < hw; ++m) acc = fmaf(kq[(size_t)m * Cq + hi] * s, v[(size_t)m * Cs + h * dv + j] * s, acc);
        kv[e] = acc;
    }
    for (int o = tid; o < Cq; o += kSliceThreads) {
        float acc = 0.f;
        for (int m = 0; m < hw; ++m) acc += kq[(size_t)m * Cq + o];
        km[o] = acc / (float)hw;
    }
    __syncthreads();

    // 5a. q = elu(W_q v + b_q) + 1, over k's buffer
    for (int e = tid; e < hw * Cq; e += kSliceThreads) {
        const int m = e / Cq, o = e - m * Cq;
        const float* vm = v + (size_t)m * Cs;
        float acc = a.bq[o];
        for (int c = 0; c < a.Kin; ++c) acc = fmaf(a.wqT[(size_t)c * Cq + o], vm[c], acc);
        kq[e] = elu1(acc);
    }
    __syncthreads();
    // 5b. the normaliser q . mean(k) + 1e-6, per token and head
    for (int e = tid; e < hw * heads; e += kSliceThreads) {
        const int m = e / heads, h = e - m * heads;
        float acc = 0.f;
        for (int i = 0; i < dq; ++i) acc = fmaf(kq[(size_t)m * Cq + h * dq + i], km[h * dq + i], acc);
        den[e] = acc + 1e-6f;
    }
    __syncthreads();
    // 5c. o = q kv / den + pe(v); RecAttn2d adds it into every fine pixel whose nearest source it is, LinearAttention3 stores it
    const float sy = (float)hc / (float)H, sx = (float)wc / (float)W;
    for (int e = tid; e < hw * Cs; e += kSliceThreads) {
        const int m = e / Cs, j = e - m * Cs;
        const int h = j / dv, jj = j - h * dv;
        const float* qm = kq + (size_t)m * Cq + h * dq;
        const float* kvh = kv + (size_t)h * dq * dv + jj;
        float acc = 0.f;
        for (int i = 0; i < dq; ++i) acc = fmaf(qm[i], kvh[(size_t)i * dv], acc);
        const int my = m / wc, mx = m - my * wc;
        float pe = a.b_pe[j];
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = my + ky - 1;
            if (yy < 0 || yy >= hc) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = mx + kx - 1;
                if (xx < 0 || xx >= wc) continue;
                pe = fmaf(a.w_pe[(ky * 3 + kx) * Cs + j], v[(size_t)(yy * wc + xx) * Cs + j], pe);
            }
        }
        const float o = acc / den[m * heads + h] + pe;
        if constexpr (ATTN) {
            for (int y = 0; y < H; ++y) {
                if (nearest_src(y, hc, sy) != my) continue;
                for (int xx = 0; xx < W; ++xx)
                    if (nearest_src(xx, wc, sx) == mx) rs[(size_t)(y * W + xx) * Cs + j] += o;
            }
        } else {
            float ov[1] = {o};
            store_vec<1>(ti + (size_t)m * C + j, ov);
        }
    }

    // 6. RecAttn2d: t = conv5(r_s + nearest(o)) (padding 2)
    if constexpr (ATTN) {
        __syncthreads();
        for (int e = tid; e < HW * cs4; e += kSliceThreads) {
            const int p = e / cs4, c = 4 * (e - p * cs4);
            const int py = p / W, px = p - py * W;
            float acc[4];
            load_vec<4>(a.b_cv + c, acc);
            for (int ky = 0; ky < 5; ++ky) {
                const int yy = py + ky - 2;
                if (yy < 0 || yy >= H) continue;
                for (int kx = 0; kx < 5; ++kx) {
                    const int xx = px + kx - 2;
                    if (xx < 0 || xx >= W) continue;
                    float sv[4], wt[4];
                    load_vec<4>(rs + (size_t)(yy * W + xx) * Cs + c, sv);
                    load_vec<4>(a.w_cv + (ky * 5 + kx) * Cs + c, wt);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = fmaf(wt[j], sv[j], acc[j]);
                }
            }
            store_vec<4>(ti + (size_t)p * C + c, acc);
        }
    }
}

template <typename T, int ATTN>
hipError_t launch_ls(const void* x, void* r, void* t, const SliceArgs& a, hipStream_t s)
{
    const T* xp = (const T*)x;
    T* rp = (T*)r;
    T* tp = (T*)t;
    const size_t pass = (size_t)a.N * a.H * a.W * ((a.C - a.Cs) >> 2);
    if (pass) {
        hipLaunchKernelGGL((k_ls_pass<T>), dim3((unsigned)((pass + 255) / 256)), dim3(256), 0, s, xp, rp, tp, a.w_rep, a.b_rep, a.N, a.H, a.W, a.C, a.Cs);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const size_t lds = sizeof(float) * slice_lds_floats(ATTN, a.H, a.W, a.Cs, a.heads, a.Cq);
    RCX_SET_LDS_ONCE((k_ls_slice<T, ATTN>), lds);
    hipLaunchKernelGGL((k_ls_slice<T, ATTN>), dim3(a.N), dim3(kSliceThreads), lds, s, xp, rp, tp, a);
    return hipGetLastError();
}

template <int ATTN>
hipError_t launch_ls_dt(const void* x, void* r, void* t, const SliceArgs& a, int dt, hipStream_t s)
{
    switch (dt) {
        case 0: return launch_ls<float, ATTN>(x, r, t, a, s);
        case 1: return launch_ls<bf16_t, ATTN>(x, r, t, a, s);
        case 2: return launch_ls<f16_t, ATTN>(x, r, t, a, s);
        default: return hipErrorInvalidValue;
    }
}

bool common_ok(int B, int H, int W, int C, int split, int dtype)
{
    return B > 0 && H > 0 && W > 0 && C > 0 && split > 0 && split <= C && C % 4 == 0 && split % 4 == 0 && dtype >= 0 && dtype <= 2
        && (size_t)B * H * W * C < ((size_t)1 << 31);
}

}  // namespace

// RecAttn2d on the slice: one head (the family's stages 0-2), any plane whose image fits the LDS
bool ls_recattn_applicable(int B, int H, int W, int C, int split, int heads, int dtype)
{
    if (!common_ok(B, H, W, C, split, dtype) || heads != 1) return false;
    return sizeof(float) * slice_lds_floats(1, H, W, split, 1, split) <= (size_t)kLdsLimit;
}

// LinearAttention3 on the slice: `heads` = the module's own num_heads (the constructor's // 2); q, k: split / 2 channels, v: split; planes of at most 64 tokens
bool ls_la3_applicable(int B, int H, int W, int C, int split, int heads, int dtype)
{
    if (!common_ok(B, H, W, C, split, dtype) || heads <= 0 || split % (2 * heads) || H * W > 64) return false;
    return sizeof(float) * slice_lds_floats(0, H, W, split, heads, split / 2) <= (size_t)kLdsLimit;
}

hipError_t ls_recattn_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const float* w_dn, const float* b_dn,
                          const float* wqT, const float* bq, const float* wkT, const float* bk, const float* w_pe, const float* b_pe,
                          const float* w_cv, const float* b_cv, int B, int H, int W, int C, int split, int dtype, hipStream_t s)
{
    const SliceArgs a{w_rep, b_rep, w_dn, b_dn, wqT, bq, wkT, bk, w_pe, b_pe, w_cv, b_cv, B, H, W, C, split, 1, split, split / 2, split / 2};
    return launch_ls_dt<1>(x, r, t, a, dtype, s);
}

hipError_t ls_la3_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const float* wqT, const float* bq,
                      const float* wkT, const float* bk, const float* w_pe, const float* b_pe, int B, int H, int W, int C, int split, int heads,
                      int dtype, hipStream_t s)
{
    const SliceArgs a{w_rep, b_rep, nullptr, nullptr, wqT, bq, wkT, bk, w_pe, b_pe, nullptr, nullptr, B, H, W, C, split, heads, split / 2, split, 0};
    return launch_ls_dt<0>(x, r, t, a, dtype, s);
}

}  // namespace rcx

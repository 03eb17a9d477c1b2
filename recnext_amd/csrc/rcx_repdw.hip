// RepVGGDW of a training step as one operator, forward and backward (lsnet/model/recattn.py:8-15: lk = ConvNorm 3x3 depthwise, sk = ConvNorm 1x1
// depthwise, r = lk(x) + sk(x) + x, both BatchNorms on batch statistics).  x is N x H x W x C, R = N H W rows of C contiguous channels, float32 / bf16 /
// f16; the parameters, statistics and r are float32; every sum is per channel over the R rows, all arithmetic float32.  With
//   u = sum_d w3[d] x(p + d) + b3 (zero padding),  ia = 1 / sqrt(var u + eps_a),  ib = 1 / sqrt(w1^2 var x + eps_b):
//
//   forward   k_rep_stats      the layout of k_bn_stats (rcx_bn.hip): a thread owns V adjacent channels and walks its rows TY apart; at each row it forms
//                              u from the nine taps (V-wide loads; the neighbours come from the cache) and sums (x - px), (x - px)^2, (u - pu), (u - pu)^2
//                              against the pivots px, pu = its first x and u: never sum x and sum x^2.  The threads' (n, mean, M2) of x and of u are
//                              combined pairwise (Chan) through LDS in the fixed tree; one partial a workgroup goes to the workspace.
//             k_rep_finalize   the P partials of a channel in index order -> mean x, var x, mean u, ia and the four running buffers.
//             k_rep_apply      r = gamma_a (u - mean u) ia + beta_a + gamma_b w1 (x - mean x) ib + beta_b + x, u formed again from x.
//   backward  k_rep_bwd_sums   partials of S0 = sum g, Su = sum g uhat, Sx = sum g (x - mean x), uhat = (u - mean u) ia, u formed again.
//             k_rep_bwd_finalize  the three sums in index order, and from them the seven per-channel parameter gradients (gb3 = gb1 = 0 exactly).
//             k_rep_bwd_dx     gu(p) = gamma_a ia (g - S0 / R - uhat Su / R) at the nine pixels p = q - d that lie in the plane (u formed at each of them
//                              with its own zero padding), gx(q) = sum_d w3[d] gu(q - d) + gamma_b w1 ib (g - S0 / R - (x - mean x) w1^2 ib^2 Sx / R) + g,
//                              and, because gw3[d] = sum_p gu(p) x(p + d) = sum_q x(q) gu(q - d), the nine tap sums of the thread's rows from the same gu;
//                              these are added through LDS in the fixed tree, one partial of nine taps a workgroup.
//             k_rep_bwd_gw3    the P partials of a tap in index order -> gw3 (C,1,3,3).
// P and the tiling are functions of (N H W, C, dtype) and of which of the two paths the pointers allow: repeat launches are bit-identical.  No atomics,
// no waiting on another workgroup.  u is never stored.
#include "rcx_common.h"
#include "rcx_launch.h"
#include "rcx_bn.h"

namespace rcx {
namespace repdw {

using bn::kThreads;
using bn::kFin;
using bn::Plan;
using bn::chan;
using bn::chunk_rows;
using bn::thread_rows;
using bn::tree_top;
using bn::tree_chan;
using bn::tree_sum;

// the three reductions, the apply and the input gradient all walk the rows by the plan of the statistics: one P for the workspace
inline Plan plan_of(int R, int C, int V) { return bn::stats_plan(R, C, V); }

__device__ __forceinline__ float inv_b(float w1, float vx, float eps_b) { return 1.f / sqrtf(fmaf(w1 * w1, vx, eps_b)); }

// w3 is (C, 9): the nine taps of this thread's V channels, tap-major in registers
template <int V>
__device__ __forceinline__ void load_taps(const float* __restrict__ w3, size_t c0, float (&w)[9][V])
{
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
        for (int k = 0; k < 9; ++k) w[k][j] = w3[(c0 + j) * 9 + k];
}

// row r of the R rows -> its image's first element of this thread's channels, and (h, w)
template <typename T>
__device__ __forceinline__ const T* pixel_of(const T* __restrict__ x, int r, int H, int W, int C, size_t c0, int& h, int& w)
{
    const int hw = H * W, n = r / hw, rem = r - n * hw;
    h = rem / W;
    w = rem - h * W;
    return x + (size_t)n * hw * C + c0;
}

// u(h, w) = sum over the taps inside the plane of w3[ky][kx] x(h + ky - 1, w + kx - 1), in tap order, + b3; xi from pixel_of
template <typename T, int V>
__device__ __forceinline__ void conv_u(const T* __restrict__ xi, int h, int w, int H, int W, int C, const float (&w3)[9][V], const float (&b3)[V], float (&u)[V])
{
#pragma unroll
    for (int j = 0; j < V; ++j) u[j] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int hh = h + ky - 1;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ww = w + kx - 1;
            if (hh >= 0 && hh < H && ww >= 0 && ww < W) {
                float v[V];
                load_vec<V>(xi + ((size_t)hh * W + ww) * C, v);
#pragma unroll
                for (int j = 0; j < V; ++j) u[j] = fmaf(w3[ky * 3 + kx][j], v[j], u[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) u[j] += b3[j];
}

// part: P x (mean x, M2 x, mean u, M2 u), each (C)
template <typename T, int V>
__global__ void __launch_bounds__(kThreads) k_rep_stats(const T* __restrict__ x, const float* __restrict__ w3_, const float* __restrict__ b3_,
                                                        float* __restrict__ part, int R, int H, int W, int C, int G, int RB)
{
    __shared__ float sm[2 * V * kThreads];
    __shared__ float sn[kThreads];
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int g = blockIdx.x * TX + tx;
    const bool live = g < G;
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    const int cnt = live ? nrow : 0;
    float px[V], sx1[V], sx2[V], pu[V], su1[V], su2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) px[j] = sx1[j] = sx2[j] = pu[j] = su1[j] = su2[j] = 0.f;
    if (cnt) {
        const size_t c0 = (size_t)g * V;
        float w3[9][V], b3[V];
        load_taps<V>(w3_, c0, w3);
        load_vec<V>(b3_ + c0, b3);
        for (int i = 0; i < cnt; ++i) {
            int h, w;
            const T* xi = pixel_of(x, r0 + ty + i * TY, H, W, C, c0, h, w);
            float v[V], u[V];
            load_vec<V>(xi + ((size_t)h * W + w) * C, v);
            conv_u<T, V>(xi, h, w, H, W, C, w3, b3, u);
            if (i == 0) {
#pragma unroll
                for (int j = 0; j < V; ++j) { px[j] = v[j]; pu[j] = u[j]; }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float dx = v[j] - px[j], du = u[j] - pu[j];
                sx1[j] += dx;
                sx2[j] = fmaf(dx, dx, sx2[j]);
                su1[j] += du;
                su2[j] = fmaf(du, du, su2[j]);
            }
        }
    }
    const float n = (float)cnt, inv = cnt ? 1.f / (float)cnt : 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float a = sx1[j] * inv, b = su1[j] * inv;
        px[j] += a;                                                   // the thread's means and M2s, in place of the pivots and the sums of squares
        sx2[j] = fmaxf(fmaf(-sx1[j], a, sx2[j]), 0.f);
        pu[j] += b;
        su2[j] = fmaxf(fmaf(-su1[j], b, su2[j]), 0.f);
    }
    tree_chan<V>(sm, sn, n, px, sx2, TX, TY, tx, ty);
    tree_chan<V>(sm, sn, n, pu, su2, TX, TY, tx, ty);
    if (ty == 0 && live) {
        float* pm = part + (size_t)blockIdx.y * 4 * C + (size_t)g * V;
        store_vec<V>(pm, px);
        store_vec<V>(pm + C, sx2);
        store_vec<V>(pm + 2 * (size_t)C, pu);
        store_vec<V>(pm + 3 * (size_t)C, su2);
    }
}

// 16 channels x 16 lanes, as k_bn_finalize: a lane combines a contiguous run of the P partials in index order, the 16 lanes in the fixed tree
__device__ __forceinline__ void fin_chan(const float* __restrict__ part, int stride, int c, bool live, int R, int RB, int P, float* sm, float& mean, float& m2)
{
    const int TX = kFin, TY = kFin, tx = threadIdx.x, ty = threadIdx.y;
    const int q = (P + kFin - 1) / kFin;
    float n = 0.f;
    mean = m2 = 0.f;
    if (live) {
        const int pe = min(P, (ty + 1) * q);
        for (int p = ty * q; p < pe; ++p) {
            int r0;
            const float nb = (float)chunk_rows(R, RB, p, r0);
            chan(n, mean, m2, nb, part[(size_t)p * stride + c], part[(size_t)p * stride + (stride / 4) + c]);
        }
    }
    for (int s = kFin / 2; s >= 1; s >>= 1) {
        if (ty >= s && ty < 2 * s) { sm[BN_SLOT(0)] = n; sm[BN_SLOT(1)] = mean; sm[BN_SLOT(2)] = m2; }
        __syncthreads();
        if (ty < s) chan(n, mean, m2, sm[BN_SLOT_AT(0, ty + s)], sm[BN_SLOT_AT(1, ty + s)], sm[BN_SLOT_AT(2, ty + s)]);
        __syncthreads();
    }
}

// run: lk running_mean, lk running_var, sk running_mean, sk running_var, all or none
__global__ void __launch_bounds__(kFin * kFin) k_rep_finalize(const float* __restrict__ part, const float* __restrict__ w1, const float* __restrict__ b1,
                                                              float* __restrict__ mean_x, float* __restrict__ var_x, float* __restrict__ mean_u,
                                                              float* __restrict__ invstd_u, float* __restrict__ lk_rm, float* __restrict__ lk_rv,
                                                              float* __restrict__ sk_rm, float* __restrict__ sk_rv, int R, int C, int RB, int P,
                                                              float mom_a, float eps_a, float mom_b)
{
    __shared__ float sm[3 * kFin * kFin];
    const int c = blockIdx.x * kFin + threadIdx.x;
    const bool live = c < C;
    float mx, m2x, mu, m2u;
    fin_chan(part, 4 * C, c, live, R, RB, P, sm, mx, m2x);
    fin_chan(part + 2 * (size_t)C, 4 * C, c, live, R, RB, P, sm, mu, m2u);
    if (threadIdx.y == 0 && live) {
        mean_x[c] = mx;
        var_x[c] = m2x / (float)R;
        mean_u[c] = mu;
        invstd_u[c] = 1.f / sqrtf(m2u / (float)R + eps_a);
        if (lk_rm) {
            const float w = w1[c];
            lk_rm[c] = (1.f - mom_a) * lk_rm[c] + mom_a * mu;
            lk_rv[c] = (1.f - mom_a) * lk_rv[c] + mom_a * (m2u / (float)(R - 1));
            sk_rm[c] = (1.f - mom_b) * sk_rm[c] + mom_b * fmaf(w, mx, b1[c]);
            sk_rv[c] = (1.f - mom_b) * sk_rv[c] + mom_b * ((w * w) * (m2x / (float)(R - 1)));
        }
    }
}

template <typename T, int V>
__global__ void __launch_bounds__(kThreads) k_rep_apply(const T* __restrict__ x, float* __restrict__ out, const float* __restrict__ w3_, const float* __restrict__ b3_,
                                                        const float* __restrict__ gamma_a, const float* __restrict__ beta_a, const float* __restrict__ w1_,
                                                        const float* __restrict__ gamma_b, const float* __restrict__ beta_b, const float* __restrict__ mean_x,
                                                        const float* __restrict__ var_x, const float* __restrict__ mean_u, const float* __restrict__ invstd_u,
                                                        int R, int H, int W, int C, int G, int RB, float eps_b)
{
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int g = blockIdx.x * TX + tx;
    if (g >= G) return;
    const size_t c0 = (size_t)g * V;
    float w3[9][V], b3[V], sa[V], ba[V], sb[V], bb[V], mx[V], mu[V];
    load_taps<V>(w3_, c0, w3);
    load_vec<V>(b3_ + c0, b3);
    load_vec<V>(gamma_a + c0, sa);
    load_vec<V>(beta_a + c0, ba);
    load_vec<V>(gamma_b + c0, sb);
    load_vec<V>(beta_b + c0, bb);
    load_vec<V>(mean_x + c0, mx);
    load_vec<V>(mean_u + c0, mu);
    {
        float ia[V], w1[V], vx[V];
        load_vec<V>(invstd_u + c0, ia);
        load_vec<V>(w1_ + c0, w1);
        load_vec<V>(var_x + c0, vx);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            sa[j] *= ia[j];
            sb[j] = sb[j] * w1[j] * inv_b(w1[j], vx[j], eps_b);
        }
    }
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    for (int i = 0; i < nrow; ++i) {
        const int r = r0 + ty + i * TY;
        int h, w;
        const T* xi = pixel_of(x, r, H, W, C, c0, h, w);
        float v[V], u[V];
        load_vec<V>(xi + ((size_t)h * W + w) * C, v);
        conv_u<T, V>(xi, h, w, H, W, C, w3, b3, u);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = (fmaf(u[j] - mu[j], sa[j], ba[j]) + fmaf(v[j] - mx[j], sb[j], bb[j])) + v[j];
        store_vec<V>(out + (size_t)r * C + c0, v);
    }
}

// part: P x (S0, Su, Sx), each (C)
template <typename T, int V>
__global__ void __launch_bounds__(kThreads) k_rep_bwd_sums(const T* __restrict__ x, const float* __restrict__ gr, const float* __restrict__ w3_,
                                                           const float* __restrict__ b3_, const float* __restrict__ mean_x, const float* __restrict__ mean_u,
                                                           const float* __restrict__ invstd_u, float* __restrict__ part, int R, int H, int W, int C, int G, int RB)
{
    __shared__ float sm[3 * V * kThreads];
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int g = blockIdx.x * TX + tx;
    const bool live = g < G;
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    float acc[3 * V];
#pragma unroll
    for (int j = 0; j < 3 * V; ++j) acc[j] = 0.f;
    if (live && nrow) {
        const size_t c0 = (size_t)g * V;
        float w3[9][V], b3[V], mx[V], mu[V], ia[V];
        load_taps<V>(w3_, c0, w3);
        load_vec<V>(b3_ + c0, b3);
        load_vec<V>(mean_x + c0, mx);
        load_vec<V>(mean_u + c0, mu);
        load_vec<V>(invstd_u + c0, ia);
        for (int i = 0; i < nrow; ++i) {
            const int r = r0 + ty + i * TY;
            int h, w;
            const T* xi = pixel_of(x, r, H, W, C, c0, h, w);
            float v[V], u[V], d[V];
            load_vec<V>(xi + ((size_t)h * W + w) * C, v);
            load_vec<V>(gr + (size_t)r * C + c0, d);
            conv_u<T, V>(xi, h, w, H, W, C, w3, b3, u);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                acc[j] += d[j];
                acc[V + j] = fmaf(d[j], (u[j] - mu[j]) * ia[j], acc[V + j]);
                acc[2 * V + j] = fmaf(d[j], v[j] - mx[j], acc[2 * V + j]);
            }
        }
    }
    tree_sum<3 * V>(sm, acc, TX, TY, tx, ty);
    if (ty == 0 && live) {
        float* pm = part + (size_t)blockIdx.y * 3 * C + (size_t)g * V;
        float t[V];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int j = 0; j < V; ++j) t[j] = acc[k * V + j];
            store_vec<V>(pm + (size_t)k * C, t);
        }
    }
}

// sums: (S0, Su, Sx), each (C), for k_rep_bwd_dx; the seven parameter gradients all or none
__global__ void __launch_bounds__(kFin * kFin) k_rep_bwd_finalize(const float* __restrict__ part, float* __restrict__ sums, const float* __restrict__ w1_,
                                                                  const float* __restrict__ gamma_b, const float* __restrict__ var_x, float* __restrict__ gb3,
                                                                  float* __restrict__ ggamma_a, float* __restrict__ gbeta_a, float* __restrict__ gw1,
                                                                  float* __restrict__ gb1, float* __restrict__ ggamma_b, float* __restrict__ gbeta_b, int C, int P,
                                                                  float eps_b)
{
    __shared__ float sm[3 * kFin * kFin];
    const int TX = kFin, TY = kFin, tx = threadIdx.x, ty = threadIdx.y;
    const int c = blockIdx.x * kFin + tx;
    const int q = (P + kFin - 1) / kFin;
    float s0 = 0.f, su = 0.f, sx = 0.f;
    if (c < C) {
        const int pe = min(P, (ty + 1) * q);
        for (int p = ty * q; p < pe; ++p) {
            s0 += part[(size_t)p * 3 * C + c];
            su += part[(size_t)p * 3 * C + C + c];
            sx += part[(size_t)p * 3 * C + 2 * (size_t)C + c];
        }
    }
    for (int s = kFin / 2; s >= 1; s >>= 1) {
        if (ty >= s && ty < 2 * s) { sm[BN_SLOT(0)] = s0; sm[BN_SLOT(1)] = su; sm[BN_SLOT(2)] = sx; }
        __syncthreads();
        if (ty < s) { s0 += sm[BN_SLOT_AT(0, ty + s)]; su += sm[BN_SLOT_AT(1, ty + s)]; sx += sm[BN_SLOT_AT(2, ty + s)]; }
        __syncthreads();
    }
    if (ty == 0 && c < C) {
        sums[c] = s0;
        sums[C + c] = su;
        sums[2 * (size_t)C + c] = sx;
        if (gw1) {
            const float w = w1_[c], ib = inv_b(w, var_x[c], eps_b);
            gb3[c] = 0.f;
            gb1[c] = 0.f;
            gbeta_a[c] = s0;
            gbeta_b[c] = s0;
            ggamma_a[c] = su;
            ggamma_b[c] = (w * ib) * sx;
            gw1[c] = ((gamma_b[c] * eps_b) * ((ib * ib) * ib)) * sx;
        }
    }
}

// gx NULL: only the tap partials; partw NULL: only gx.  partw: P x 9 x (C)
template <typename T, int V>
__global__ void __launch_bounds__(kThreads) k_rep_bwd_dx(const T* __restrict__ x, const float* __restrict__ gr, T* __restrict__ gx, const float* __restrict__ w3_,
                                                         const float* __restrict__ b3_, const float* __restrict__ gamma_a, const float* __restrict__ w1_,
                                                         const float* __restrict__ gamma_b, const float* __restrict__ mean_x, const float* __restrict__ var_x,
                                                         const float* __restrict__ mean_u, const float* __restrict__ invstd_u, const float* __restrict__ sums,
                                                         float* __restrict__ partw, int R, int H, int W, int C, int G, int RB, float eps_b)
{
    __shared__ float sm[V * kThreads];
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int g = blockIdx.x * TX + tx;
    const bool live = g < G;
    if (!partw && !live) return;                                      // no barrier follows
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    float gw[9][V];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) gw[k][j] = 0.f;
    if (live && nrow) {
        const size_t c0 = (size_t)g * V;
        // gu = A (g - m0 - (u - mu) k1),  the sk branch: B (g - m0 - (x - mx) k2)
        float w3[9][V], b3[V], A[V], m0[V], mu[V], k1[V], B[V], mx[V], k2[V];
        load_taps<V>(w3_, c0, w3);
        load_vec<V>(b3_ + c0, b3);
        load_vec<V>(gamma_a + c0, A);
        load_vec<V>(sums + c0, m0);
        load_vec<V>(mean_u + c0, mu);
        load_vec<V>(sums + C + c0, k1);
        load_vec<V>(gamma_b + c0, B);
        load_vec<V>(mean_x + c0, mx);
        load_vec<V>(sums + 2 * (size_t)C + c0, k2);
        {
            float ia[V], w1[V], vx[V];
            load_vec<V>(invstd_u + c0, ia);
            load_vec<V>(w1_ + c0, w1);
            load_vec<V>(var_x + c0, vx);
            const float ir = 1.f / (float)R;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float ib = inv_b(w1[j], vx[j], eps_b), wib = w1[j] * ib;
                A[j] *= ia[j];
                m0[j] *= ir;
                k1[j] = ia[j] * (k1[j] * ir);
                B[j] *= wib;
                k2[j] = (wib * wib) * (k2[j] * ir);
            }
        }
        for (int i = 0; i < nrow; ++i) {
            const int r = r0 + ty + i * TY;
            int h, w;
            const T* xi = pixel_of(x, r, H, W, C, c0, h, w);
            const float* gi = gr + ((size_t)r - ((size_t)h * W + w)) * C + c0;      // this image's first row of g
            float xq[V], acc[V];
            load_vec<V>(xi + ((size_t)h * W + w) * C, xq);
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = 0.f;
            // tap (ky, kx) of the conv reads x(p + d): the pixel p whose u holds w3[d] x(q) is p = q - d
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int ph = h - (ky - 1);
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int pw = w - (kx - 1);
                    if (ph >= 0 && ph < H && pw >= 0 && pw < W) {
                        float u[V], d[V];
                        conv_u<T, V>(xi, ph, pw, H, W, C, w3, b3, u);
                        load_vec<V>(gi + ((size_t)ph * W + pw) * C, d);
#pragma unroll
                        for (int j = 0; j < V; ++j) {
                            const float gu = A[j] * (fmaf(-(u[j] - mu[j]), k1[j], d[j]) - m0[j]);
                            acc[j] = fmaf(w3[ky * 3 + kx][j], gu, acc[j]);
                            gw[ky * 3 + kx][j] = fmaf(xq[j], gu, gw[ky * 3 + kx][j]);
                        }
                    }
                }
            }
            if (gx) {
                float d[V];
                load_vec<V>(gr + (size_t)r * C + c0, d);
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] = (acc[j] + B[j] * (fmaf(-(xq[j] - mx[j]), k2[j], d[j]) - m0[j])) + d[j];
                store_vec<V>(gx + (size_t)r * C + c0, acc);
            }
        }
    }
    if (!partw) return;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        tree_sum<V>(sm, gw[k], TX, TY, tx, ty);
        if (ty == 0 && live) store_vec<V>(partw + ((size_t)blockIdx.y * 9 + k) * C + (size_t)g * V, gw[k]);
    }
}

// 16 (tap, channel) pairs x 16 lanes: the P partials in index order, as the other finalizes; gw3 is (C, 9)
__global__ void __launch_bounds__(kFin * kFin) k_rep_bwd_gw3(const float* __restrict__ partw, float* __restrict__ gw3, int C, int P)
{
    __shared__ float sm[kFin * kFin];
    const int TX = kFin, TY = kFin, tx = threadIdx.x, ty = threadIdx.y;
    const int i = blockIdx.x * kFin + tx;                              // k * C + c
    const bool live = i < 9 * C;
    const int q = (P + kFin - 1) / kFin;
    float s0 = 0.f;
    if (live) {
        const int pe = min(P, (ty + 1) * q);
        for (int p = ty * q; p < pe; ++p) s0 += partw[(size_t)p * 9 * C + i];
    }
    for (int s = kFin / 2; s >= 1; s >>= 1) {
        if (ty >= s && ty < 2 * s) sm[BN_SLOT(0)] = s0;
        __syncthreads();
        if (ty < s) s0 += sm[BN_SLOT_AT(0, ty + s)];
        __syncthreads();
    }
    if (ty == 0 && live) {
        const int k = i / C, c = i - k * C;
        gw3[(size_t)c * 9 + k] = s0;
    }
}

struct Fwd {
    const void* x; float* out; const float *w3, *b3, *gamma_a, *beta_a, *w1, *b1, *gamma_b, *beta_b;
    float *lk_rm, *lk_rv, *sk_rm, *sk_rv, *mean_x, *var_x, *mean_u, *invstd_u, *ws;
    int N, H, W, C; float mom_a, eps_a, mom_b, eps_b;
};
struct Bwd {
    const void* x; const float *g, *w3, *b3, *gamma_a, *w1, *gamma_b, *mean_x, *var_x, *mean_u, *invstd_u;
    void* gx; float *gw3, *gb3, *ggamma_a, *gbeta_a, *gw1, *gb1, *ggamma_b, *gbeta_b, *ws;
    int N, H, W, C; float eps_b;
};

inline dim3 fin_grid(int n) { return dim3((unsigned)((n + kFin - 1) / kFin)); }

// workspace: (S0, Su, Sx) (3 C floats), then the partials of the launch in flight (P x 4 C, P x 3 C or P x 9 C floats)
template <typename T, int V>
hipError_t fwd(const Fwd& a, hipStream_t s)
{
    const int R = a.N * a.H * a.W, C = a.C;
    const Plan p = plan_of(R, C, V);
    float* part = a.ws + 3 * (size_t)C;
    hipLaunchKernelGGL((k_rep_stats<T, V>), bn::grid_of(p), bn::block_of(p), 0, s, (const T*)a.x, a.w3, a.b3, part, R, a.H, a.W, C, p.G, p.RB);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rep_finalize, fin_grid(C), dim3(kFin, kFin), 0, s, (const float*)part, a.w1, a.b1, a.mean_x, a.var_x, a.mean_u, a.invstd_u, a.lk_rm,
                       a.lk_rv, a.sk_rm, a.sk_rv, R, C, p.RB, p.P, a.mom_a, a.eps_a, a.mom_b);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL((k_rep_apply<T, V>), bn::grid_of(p), bn::block_of(p), 0, s, (const T*)a.x, a.out, a.w3, a.b3, a.gamma_a, a.beta_a, a.w1, a.gamma_b, a.beta_b,
                       (const float*)a.mean_x, (const float*)a.var_x, (const float*)a.mean_u, (const float*)a.invstd_u, R, a.H, a.W, C, p.G, p.RB, a.eps_b);
    return hipGetLastError();
}

template <typename T, int V>
hipError_t bwd(const Bwd& a, hipStream_t s)
{
    const int R = a.N * a.H * a.W, C = a.C;
    const Plan p = plan_of(R, C, V);
    float* part = a.ws + 3 * (size_t)C;
    hipLaunchKernelGGL((k_rep_bwd_sums<T, V>), bn::grid_of(p), bn::block_of(p), 0, s, (const T*)a.x, a.g, a.w3, a.b3, a.mean_x, a.mean_u, a.invstd_u, part, R, a.H, a.W,
                       C, p.G, p.RB);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rep_bwd_finalize, fin_grid(C), dim3(kFin, kFin), 0, s, (const float*)part, a.ws, a.w1, a.gamma_b, a.var_x, a.gb3, a.ggamma_a, a.gbeta_a,
                       a.gw1, a.gb1, a.ggamma_b, a.gbeta_b, C, p.P, a.eps_b);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    float* partw = a.gw3 ? part : nullptr;
    hipLaunchKernelGGL((k_rep_bwd_dx<T, V>), bn::grid_of(p), bn::block_of(p), 0, s, (const T*)a.x, a.g, (T*)a.gx, a.w3, a.b3, a.gamma_a, a.w1, a.gamma_b, a.mean_x,
                       a.var_x, a.mean_u, a.invstd_u, (const float*)a.ws, partw, R, a.H, a.W, C, p.G, p.RB, a.eps_b);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (partw) {
        hipLaunchKernelGGL(k_rep_bwd_gw3, fin_grid(9 * C), dim3(kFin, kFin), 0, s, (const float*)partw, a.gw3, C, p.P);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace repdw

size_t repdw_train_workspace_bytes(int R, int C, int dtype)
{
    const bn::Plan w = repdw::plan_of(R, C, C % bn::wide_v(dtype) ? 1 : bn::wide_v(dtype)), n = repdw::plan_of(R, C, 1);
    const int P = w.P > n.P ? w.P : n.P;
    return sizeof(float) * ((size_t)P * 9 * C + 3 * (size_t)C);
}

hipError_t repdw_train_fwd(const void* x, float* out, const float* w3, const float* b3, const float* gamma_a, const float* beta_a, const float* w1, const float* b1,
                           const float* gamma_b, const float* beta_b, float* lk_rm, float* lk_rv, float* sk_rm, float* sk_rv, float* mean_x, float* var_x,
                           float* mean_u, float* invstd_u, void* workspace, int N, int H, int W, int C, float mom_a, float eps_a, float mom_b, float eps_b,
                           int dtype, hipStream_t s)
{
    const repdw::Fwd a{x, out, w3, b3, gamma_a, beta_a, w1, b1, gamma_b, beta_b, lk_rm, lk_rv, sk_rm, sk_rv, mean_x, var_x, mean_u, invstd_u, (float*)workspace,
                       N, H, W, C, mom_a, eps_a, mom_b, eps_b};
    const bool wide = bn::can_wide(C, dtype, {x, out, b3, gamma_a, beta_a, w1, gamma_b, beta_b, mean_x, var_x, mean_u, invstd_u, workspace});
    BN_DISPATCH(repdw::fwd, dtype, wide, a, s)
}

hipError_t repdw_train_bwd(const void* x, const float* g, const float* w3, const float* b3, const float* gamma_a, const float* w1, const float* gamma_b,
                           const float* mean_x, const float* var_x, const float* mean_u, const float* invstd_u, void* gx, float* gw3, float* gb3, float* ggamma_a,
                           float* gbeta_a, float* gw1, float* gb1, float* ggamma_b, float* gbeta_b, void* workspace, int N, int H, int W, int C, float eps_b,
                           int dtype, hipStream_t s)
{
    const repdw::Bwd a{x, g, w3, b3, gamma_a, w1, gamma_b, mean_x, var_x, mean_u, invstd_u, gx, gw3, gb3, ggamma_a, gbeta_a, gw1, gb1, ggamma_b, gbeta_b,
                       (float*)workspace, N, H, W, C, eps_b};
    const bool wide = bn::can_wide(C, dtype, {x, g, b3, gamma_a, w1, gamma_b, mean_x, var_x, mean_u, invstd_u, gx, workspace});
    BN_DISPATCH(repdw::bwd, dtype, wide, a, s)
}

}  // namespace rcx

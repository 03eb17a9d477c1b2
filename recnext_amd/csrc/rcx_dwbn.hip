// A depthwise ConvNorm of a training step as one operator, forward and backward: the slice mixers' down[0] (5x5 stride 2), pe (3x3), conv (5x5 on
// x + resize(a)) and LinearAttention3.pe (3x3) (lsnet/model/recattn.py:54-67, :89-112).  x is N x H x W x C (float32 / bf16 / f16), a the optional
// float32 N x Hc x Wc x C coarse plane (nearest resize, stride 1 only), the output plane Ho x Wo = ((H - 1) / s + 1) x ((W - 1) / s + 1), R = N Ho Wo rows:
//
//   z = x + a(nearest(h), nearest(w))       u = sum_d w[d] z(p s + d - k/2) + b (zero padding)       y = gamma (u - mean u) ia + beta, ia = 1 / sqrt(var u + eps)
//
//   forward   k_dwbn_stats        the layout of k_bn_stats (rcx_bn.hip): a thread owns V adjacent channels and walks its rows TY apart; it forms u from the k^2
//                                 taps, STORES it (float32, R x C: the apply and the whole backward read it, nothing forms u again) and sums (u - pu),
//                                 (u - pu)^2 against the pivot pu = its first u.  (n, mean, M2) are combined pairwise (Chan) through LDS in the fixed tree;
//                                 one partial a workgroup goes to the workspace.
//             k_dwbn_finalize     the P partials of a channel in index order -> mean u, ia and the running buffers.
//             k_dwbn_apply        y = gamma ia (u - mean u) + beta from the stored u, rounded once at the store.
//   backward  k_dwbn_bwd_sums     partials of S0 = sum g, Su = sum g uhat, uhat = (u - mean u) ia, from g (in y's type) and the stored u.
//             k_dwbn_bwd_finalize the two sums in index order; ggamma = Su, gbeta = S0, gb = 0 exactly.
//             k_dwbn_bwd_dx       gz(q) = sum_d w[d] gu(p), p s + d - k/2 = q, gu = gamma ia (g - S0 / R - uhat Su / R) from g and u at the (at most k^2) p:
//                                 2 k^2 loads a pixel, never k^2 k^2 taps.  Plain form: a thread walks the input pixels, gx = gz.
//             k_dwbn_bwd_dx_up    up-add form: a thread walks the COARSE pixels; the fine pixels whose nearest source is that coarse pixel are a rectangle,
//                                 and the rectangles tile the fine plane: gx = gz at each of them, ga = their sum in raster order (a gather, no atomics).
//             k_dwbn_bwd_gw       gw[ky][kx] = sum_p gu(p) z(p s + d - k/2): grid.z = ky, a thread keeps the k taps of that row; added through LDS in the
//                                 fixed tree, one partial of k taps a workgroup.
//             k_dwbn_bwd_gw_fin   the P partials of a tap in index order -> gw (C,1,k,k).
// The taps of a workgroup's channels sit in LDS ([tap][channel], read V-wide): 25 taps of 8 channels would not fit a thread's registers.  P and the tiling are
// functions of (rows, C, dtype) and of which of the two paths the pointers allow: repeat launches are bit-identical.  No atomics, no waiting on another workgroup.
#include "rcx_common.h"
#include "rcx_launch.h"
#include "rcx_bn.h"

namespace rcx {
namespace dwbn {

using bn::kThreads;
using bn::kFin;
using bn::kMaxTX;
using bn::Plan;
using bn::chan;
using bn::chunk_rows;
using bn::thread_rows;
using bn::tree_chan;
using bn::tree_sum;

// Hc = 0: the plain form.  sy, sx = (float)Hc / H, (float)Wc / W, as ATen's nearest resize and rcx_upadd_dwconv_fwd
struct Geo { int H, W, Ho, Wo, Hc, Wc, stride; float sy, sx; };

constexpr int lds_floats(int K, int V, int tree) { return K * K * kMaxTX * V > tree ? K * K * kMaxTX * V : tree; }

// the K^2 taps of this workgroup's TX V channels, w (C, K^2) -> sw[tap][channel]; ends on a barrier
template <int K>
__device__ __forceinline__ void stage_taps(const float* __restrict__ w, float* sw, int C, int CW)
{
    const int cb = blockIdx.x * CW, tid = threadIdx.y * blockDim.x + threadIdx.x, nt = blockDim.x * blockDim.y;      // TX TY may be short of kThreads
    for (int i = tid; i < CW * K * K; i += nt) {
        const int cl = i / (K * K), t = i - cl * (K * K);
        sw[t * CW + cl] = cb + cl < C ? w[(size_t)(cb + cl) * (K * K) + t] : 0.f;
    }
    __syncthreads();
}

// row r of a plane of hw = h_ w_ pixels -> image n and (h, w)
__device__ __forceinline__ int pixel_of(int r, int h_, int w_, int& h, int& w)
{
    const int hw = h_ * w_, n = r / hw, rem = r - n * hw;
    h = rem / w_;
    w = rem - h * w_;
    return n;
}

// z(hh, ww) of one image: xi, ai = the image's first element of this thread's channels (ai NULL: the plain form)
template <typename T, int V>
__device__ __forceinline__ void load_z(const T* __restrict__ xi, const float* __restrict__ ai, int hh, int ww, const Geo& g, int C, float (&v)[V])
{
    load_vec<V>(xi + ((size_t)hh * g.W + ww) * C, v);
    if (ai) {
        float t[V];
        load_vec<V>(ai + ((size_t)nearest_src(hh, g.Hc, g.sy) * g.Wc + nearest_src(ww, g.Wc, g.sx)) * C, t);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] += t[j];
    }
}

// u(ho, wo) = sum over the taps inside the plane, in tap order, + b; sw = this thread's column of the staged taps
template <typename T, int V, int K>
__device__ __forceinline__ void conv_u(const T* __restrict__ xi, const float* __restrict__ ai, int ho, int wo, const Geo& g, int C, const float* sw, int CW,
                                       const float (&b)[V], float (&u)[V])
{
#pragma unroll
    for (int j = 0; j < V; ++j) u[j] = 0.f;
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
        const int hh = ho * g.stride + ky - K / 2;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const int ww = wo * g.stride + kx - K / 2;
            if (hh >= 0 && hh < g.H && ww >= 0 && ww < g.W) {
                float v[V], t[V];
                load_z<T, V>(xi, ai, hh, ww, g, C, v);
                load_vec<V>(sw + (ky * K + kx) * CW, t);
#pragma unroll
                for (int j = 0; j < V; ++j) u[j] = fmaf(t[j], v[j], u[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) u[j] += b[j];
}

// part: P x (mean u, M2 u), each (C); ubuf: R x C
template <typename T, int V, int K>
__global__ void __launch_bounds__(kThreads) k_dwbn_stats(const T* __restrict__ x, const float* __restrict__ a, const float* __restrict__ w_, const float* __restrict__ b_,
                                                         float* __restrict__ ubuf, float* __restrict__ part, Geo geo, int R, int C, int G, int RB)
{
    __shared__ __attribute__((aligned(16))) float sm[lds_floats(K, V, (2 * V + 1) * kThreads)];
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y, CW = TX * V;
    const int g = blockIdx.x * TX + tx;
    const bool live = g < G;
    stage_taps<K>(w_, sm, C, CW);
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    const int cnt = live ? nrow : 0;
    float pu[V], s1[V], s2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) pu[j] = s1[j] = s2[j] = 0.f;
    if (cnt) {
        const size_t c0 = (size_t)g * V;
        float b[V];
#pragma unroll
        for (int j = 0; j < V; ++j) b[j] = 0.f;
        if (b_) load_vec<V>(b_ + c0, b);
        for (int i = 0; i < cnt; ++i) {
            const int r = r0 + ty + i * TY;
            int ho, wo;
            const int n = pixel_of(r, geo.Ho, geo.Wo, ho, wo);
            const T* xi = x + (size_t)n * geo.H * geo.W * C + c0;
            const float* ai = a ? a + (size_t)n * geo.Hc * geo.Wc * C + c0 : nullptr;
            float u[V];
            conv_u<T, V, K>(xi, ai, ho, wo, geo, C, sm + tx * V, CW, b, u);
            store_vec<V>(ubuf + (size_t)r * C + c0, u);
            if (i == 0) {
#pragma unroll
                for (int j = 0; j < V; ++j) pu[j] = u[j];
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float du = u[j] - pu[j];
                s1[j] += du;
                s2[j] = fmaf(du, du, s2[j]);
            }
        }
    }
    const float n = (float)cnt, inv = cnt ? 1.f / (float)cnt : 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float m = s1[j] * inv;
        pu[j] += m;                                                   // the thread's mean and M2, in place of the pivot and the sum of squares
        s2[j] = fmaxf(fmaf(-s1[j], m, s2[j]), 0.f);
    }
    __syncthreads();                                                  // the taps are done with: the tree takes their LDS
    tree_chan<V>(sm, sm + 2 * V * kThreads, n, pu, s2, TX, TY, tx, ty);
    if (ty == 0 && live) {
        float* pm = part + (size_t)blockIdx.y * 2 * C + (size_t)g * V;
        store_vec<V>(pm, pu);
        store_vec<V>(pm + C, s2);
    }
}

// 16 channels x 16 lanes, as k_bn_finalize: a lane combines a contiguous run of the P partials in index order, the 16 lanes in the fixed tree
__global__ void __launch_bounds__(kFin * kFin) k_dwbn_finalize(const float* __restrict__ part, float* __restrict__ mean_u, float* __restrict__ invstd_u,
                                                               float* __restrict__ rm, float* __restrict__ rv, int R, int C, int RB, int P, float mom, float eps)
{
    __shared__ float sm[3 * kFin * kFin];
    const int TX = kFin, TY = kFin, tx = threadIdx.x, ty = threadIdx.y;
    const int c = blockIdx.x * kFin + tx;
    const bool live = c < C;
    const int q = (P + kFin - 1) / kFin;
    float n = 0.f, mean = 0.f, m2 = 0.f;
    if (live) {
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
    if (ty == 0 && live) {
        mean_u[c] = mean;
        invstd_u[c] = 1.f / sqrtf(m2 / (float)R + eps);
        if (rm) {
            rm[c] = (1.f - mom) * rm[c] + mom * mean;
            rv[c] = (1.f - mom) * rv[c] + mom * (m2 / (float)(R - 1));
        }
    }
}

template <typename T, int V>
__global__ void __launch_bounds__(kThreads) k_dwbn_apply(const float* __restrict__ ubuf, T* __restrict__ y, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ mean_u, const float* __restrict__ invstd_u,
                                                         int R, int C, int G, int RB)
{
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int g = blockIdx.x * TX + tx;
    if (g >= G) return;
    const size_t c0 = (size_t)g * V;
    float sa[V], ba[V], mu[V], ia[V];
    load_vec<V>(gamma + c0, sa);
    load_vec<V>(beta + c0, ba);
    load_vec<V>(mean_u + c0, mu);
    load_vec<V>(invstd_u + c0, ia);
#pragma unroll
    for (int j = 0; j < V; ++j) sa[j] *= ia[j];
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    for (int i = 0; i < nrow; ++i) {
        const size_t o = (size_t)(r0 + ty + i * TY) * C + c0;
        float u[V];
        load_vec<V>(ubuf + o, u);
#pragma unroll
        for (int j = 0; j < V; ++j) u[j] = fmaf(u[j] - mu[j], sa[j], ba[j]);
        store_vec<V>(y + o, u);
    }
}

// part: P x (S0, Su), each (C)
template <typename T, int V>
__global__ void __launch_bounds__(kThreads) k_dwbn_bwd_sums(const float* __restrict__ ubuf, const T* __restrict__ gy, const float* __restrict__ mean_u,
                                                            const float* __restrict__ invstd_u, float* __restrict__ part, int R, int C, int G, int RB)
{
    __shared__ float sm[2 * V * kThreads];
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int g = blockIdx.x * TX + tx;
    const bool live = g < G;
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    float acc[2 * V];
#pragma unroll
    for (int j = 0; j < 2 * V; ++j) acc[j] = 0.f;
    if (live && nrow) {
        const size_t c0 = (size_t)g * V;
        float mu[V], ia[V];
        load_vec<V>(mean_u + c0, mu);
        load_vec<V>(invstd_u + c0, ia);
        for (int i = 0; i < nrow; ++i) {
            const size_t o = (size_t)(r0 + ty + i * TY) * C + c0;
            float u[V], d[V];
            load_vec<V>(ubuf + o, u);
            load_vec<V>(gy + o, d);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                acc[j] += d[j];
                acc[V + j] = fmaf(d[j], (u[j] - mu[j]) * ia[j], acc[V + j]);
            }
        }
    }
    tree_sum<2 * V>(sm, acc, TX, TY, tx, ty);
    if (ty == 0 && live) {
        float* pm = part + (size_t)blockIdx.y * 2 * C + (size_t)g * V;
        float t[V];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int j = 0; j < V; ++j) t[j] = acc[k * V + j];
            store_vec<V>(pm + (size_t)k * C, t);
        }
    }
}

// sums: (S0, Su), each (C), for the two kernels that form gu; gb, ggamma, gbeta each or NULL
__global__ void __launch_bounds__(kFin * kFin) k_dwbn_bwd_finalize(const float* __restrict__ part, float* __restrict__ sums, float* __restrict__ gb,
                                                                   float* __restrict__ ggamma, float* __restrict__ gbeta, int C, int P)
{
    __shared__ float sm[2 * kFin * kFin];
    const int TX = kFin, TY = kFin, tx = threadIdx.x, ty = threadIdx.y;
    const int c = blockIdx.x * kFin + tx;
    const int q = (P + kFin - 1) / kFin;
    float s0 = 0.f, su = 0.f;
    if (c < C) {
        const int pe = min(P, (ty + 1) * q);
        for (int p = ty * q; p < pe; ++p) {
            s0 += part[(size_t)p * 2 * C + c];
            su += part[(size_t)p * 2 * C + C + c];
        }
    }
    for (int s = kFin / 2; s >= 1; s >>= 1) {
        if (ty >= s && ty < 2 * s) { sm[BN_SLOT(0)] = s0; sm[BN_SLOT(1)] = su; }
        __syncthreads();
        if (ty < s) { s0 += sm[BN_SLOT_AT(0, ty + s)]; su += sm[BN_SLOT_AT(1, ty + s)]; }
        __syncthreads();
    }
    if (ty == 0 && c < C) {
        sums[c] = s0;
        sums[C + c] = su;
        if (gb) gb[c] = 0.f;                                          // a bias in front of a BatchNorm on batch statistics has no gradient
        if (ggamma) ggamma[c] = su;
        if (gbeta) gbeta[c] = s0;
    }
}

// the per-channel constants of gu = A (g - m0 - (u - mu) k1)
template <int V>
struct GuConst { float A[V], m0[V], mu[V], k1[V]; };

template <int V>
__device__ __forceinline__ void load_gu_const(const float* __restrict__ gamma, const float* __restrict__ mean_u, const float* __restrict__ invstd_u,
                                              const float* __restrict__ sums, int R, int C, size_t c0, GuConst<V>& k)
{
    float ia[V];
    load_vec<V>(gamma + c0, k.A);
    load_vec<V>(sums + c0, k.m0);
    load_vec<V>(mean_u + c0, k.mu);
    load_vec<V>(sums + C + c0, k.k1);
    load_vec<V>(invstd_u + c0, ia);
    const float ir = 1.f / (float)R;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        k.A[j] *= ia[j];
        k.m0[j] *= ir;
        k.k1[j] = ia[j] * (k.k1[j] * ir);
    }
}

template <typename T, int V>
__device__ __forceinline__ void load_gu(const float* __restrict__ up, const T* __restrict__ gp, const GuConst<V>& k, float (&gu)[V])
{
    float u[V], d[V];
    load_vec<V>(up, u);
    load_vec<V>(gp, d);
#pragma unroll
    for (int j = 0; j < V; ++j) gu[j] = k.A[j] * (fmaf(-(u[j] - k.mu[j]), k.k1[j], d[j]) - k.m0[j]);
}

// gz(h, w) = sum_d w[d] gu(p), p s + d - K/2 = (h, w): ui, gi = the image's first row of u and g (this thread's channels)
template <typename T, int V, int K>
__device__ __forceinline__ void grad_z(const float* __restrict__ ui, const T* __restrict__ gi, int h, int w, const Geo& g, int C, const float* sw, int CW,
                                       const GuConst<V>& k, float (&acc)[V])
{
    const int sh = g.stride - 1;                                      // stride 1 | 2: the division is a shift, the remainder a mask
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
        const int ty_ = h + K / 2 - ky, ph = ty_ >> sh;
        if (ty_ < 0 || (ty_ & sh) || ph >= g.Ho) continue;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const int tx_ = w + K / 2 - kx, pw = tx_ >> sh;
            if (tx_ < 0 || (tx_ & sh) || pw >= g.Wo) continue;
            const size_t o = ((size_t)ph * g.Wo + pw) * C;
            float gu[V], t[V];
            load_gu<T, V>(ui + o, gi + o, k, gu);
            load_vec<V>(sw + (ky * K + kx) * CW, t);
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = fmaf(t[j], gu[j], acc[j]);
        }
    }
}

// the plain form: rows = the N H W input pixels
template <typename T, int V, int K>
__global__ void __launch_bounds__(kThreads) k_dwbn_bwd_dx(const float* __restrict__ ubuf, const T* __restrict__ gy, T* __restrict__ gx, const float* __restrict__ w_,
                                                          const float* __restrict__ gamma, const float* __restrict__ mean_u, const float* __restrict__ invstd_u,
                                                          const float* __restrict__ sums, Geo geo, int R, int Rin, int C, int G, int RB)
{
    __shared__ __attribute__((aligned(16))) float sm[K * K * kMaxTX * V];
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y, CW = TX * V;
    const int g = blockIdx.x * TX + tx;
    stage_taps<K>(w_, sm, C, CW);
    if (g >= G) return;                                               // no barrier follows
    int r0;
    const int nrow = thread_rows(chunk_rows(Rin, RB, blockIdx.y, r0), ty, TY);
    if (!nrow) return;
    const size_t c0 = (size_t)g * V;
    GuConst<V> k;
    load_gu_const<V>(gamma, mean_u, invstd_u, sums, R, C, c0, k);
    for (int i = 0; i < nrow; ++i) {
        const int r = r0 + ty + i * TY;
        int h, w;
        const int n = pixel_of(r, geo.H, geo.W, h, w);
        const size_t oi = (size_t)n * geo.Ho * geo.Wo * C + c0;
        float acc[V];
        grad_z<T, V, K>(ubuf + oi, gy + oi, h, w, geo, C, sm + tx * V, CW, k, acc);
        store_vec<V>(gx + (size_t)r * C + c0, acc);
    }
}

// the smallest d of [0, n_out] whose nearest source is >= target (n_out when there is none): nearest_src is monotone in d
__device__ __forceinline__ int first_of(int target, int n_out, int n_in, float scale)
{
    int d = (int)(((long long)target * n_out + n_in - 1) / n_in);
    d = d < n_out ? d : n_out;
    while (d > 0 && nearest_src(d - 1, n_in, scale) >= target) --d;
    while (d < n_out && nearest_src(d, n_in, scale) < target) ++d;
    return d;
}

// the up-add form (stride 1): rows = the N Hc Wc coarse pixels; gx and ga each or NULL
template <typename T, int V, int K>
__global__ void __launch_bounds__(kThreads) k_dwbn_bwd_dx_up(const float* __restrict__ ubuf, const T* __restrict__ gy, T* __restrict__ gx, float* __restrict__ ga,
                                                             const float* __restrict__ w_, const float* __restrict__ gamma, const float* __restrict__ mean_u,
                                                             const float* __restrict__ invstd_u, const float* __restrict__ sums, Geo geo, int R, int Rc, int C,
                                                             int G, int RB)
{
    __shared__ __attribute__((aligned(16))) float sm[K * K * kMaxTX * V];
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y, CW = TX * V;
    const int g = blockIdx.x * TX + tx;
    stage_taps<K>(w_, sm, C, CW);
    if (g >= G) return;                                               // no barrier follows
    int r0;
    const int nrow = thread_rows(chunk_rows(Rc, RB, blockIdx.y, r0), ty, TY);
    if (!nrow) return;
    const size_t c0 = (size_t)g * V;
    GuConst<V> k;
    load_gu_const<V>(gamma, mean_u, invstd_u, sums, R, C, c0, k);
    for (int i = 0; i < nrow; ++i) {
        const int r = r0 + ty + i * TY;
        int hc, wc;
        const int n = pixel_of(r, geo.Hc, geo.Wc, hc, wc);
        const int h0 = first_of(hc, geo.H, geo.Hc, geo.sy), h1 = first_of(hc + 1, geo.H, geo.Hc, geo.sy);
        const int w0 = first_of(wc, geo.W, geo.Wc, geo.sx), w1 = first_of(wc + 1, geo.W, geo.Wc, geo.sx);
        const size_t oi = (size_t)n * geo.H * geo.W * C + c0;         // stride 1: the output plane is the input plane
        float sum[V];
#pragma unroll
        for (int j = 0; j < V; ++j) sum[j] = 0.f;
        for (int h = h0; h < h1; ++h)
            for (int w = w0; w < w1; ++w) {
                float acc[V];
                grad_z<T, V, K>(ubuf + oi, gy + oi, h, w, geo, C, sm + tx * V, CW, k, acc);
                if (gx) store_vec<V>(gx + oi + ((size_t)h * geo.W + w) * C, acc);
#pragma unroll
                for (int j = 0; j < V; ++j) sum[j] += acc[j];
            }
        if (ga) store_vec<V>(ga + (size_t)r * C + c0, sum);
    }
}

// grid.z = ky; partw: P x K x K x (C)
template <typename T, int V, int K>
__global__ void __launch_bounds__(kThreads) k_dwbn_bwd_gw(const T* __restrict__ x, const float* __restrict__ a, const float* __restrict__ ubuf,
                                                          const T* __restrict__ gy, const float* __restrict__ gamma, const float* __restrict__ mean_u,
                                                          const float* __restrict__ invstd_u, const float* __restrict__ sums, float* __restrict__ partw, Geo geo,
                                                          int R, int C, int G, int RB)
{
    __shared__ float sm[V * kThreads];
    const int TX = blockDim.x, TY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y, ky = blockIdx.z;
    const int g = blockIdx.x * TX + tx;
    const bool live = g < G;
    int r0;
    const int nrow = thread_rows(chunk_rows(R, RB, blockIdx.y, r0), ty, TY);
    float gw[K][V];
#pragma unroll
    for (int kx = 0; kx < K; ++kx)
#pragma unroll
        for (int j = 0; j < V; ++j) gw[kx][j] = 0.f;
    if (live && nrow) {
        const size_t c0 = (size_t)g * V;
        GuConst<V> k;
        load_gu_const<V>(gamma, mean_u, invstd_u, sums, R, C, c0, k);
        for (int i = 0; i < nrow; ++i) {
            const int r = r0 + ty + i * TY;
            int ho, wo;
            const int n = pixel_of(r, geo.Ho, geo.Wo, ho, wo);
            const int hh = ho * geo.stride + ky - K / 2;
            if (hh < 0 || hh >= geo.H) continue;
            const T* xi = x + (size_t)n * geo.H * geo.W * C + c0;
            const float* ai = a ? a + (size_t)n * geo.Hc * geo.Wc * C + c0 : nullptr;
            float gu[V];
            load_gu<T, V>(ubuf + (size_t)r * C + c0, gy + (size_t)r * C + c0, k, gu);
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int ww = wo * geo.stride + kx - K / 2;
                if (ww >= 0 && ww < geo.W) {
                    float v[V];
                    load_z<T, V>(xi, ai, hh, ww, geo, C, v);
#pragma unroll
                    for (int j = 0; j < V; ++j) gw[kx][j] = fmaf(gu[j], v[j], gw[kx][j]);
                }
            }
        }
    }
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
        tree_sum<V>(sm, gw[kx], TX, TY, tx, ty);
        if (ty == 0 && live) store_vec<V>(partw + (((size_t)blockIdx.y * K + ky) * K + kx) * C + (size_t)g * V, gw[kx]);
    }
}

// 16 (tap, channel) pairs x 16 lanes: the P partials in index order, as the other finalizes; gw is (C, KK)
__global__ void __launch_bounds__(kFin * kFin) k_dwbn_bwd_gw_fin(const float* __restrict__ partw, float* __restrict__ gw, int C, int KK, int P)
{
    __shared__ float sm[kFin * kFin];
    const int TX = kFin, TY = kFin, tx = threadIdx.x, ty = threadIdx.y;
    const int i = blockIdx.x * kFin + tx;                              // t * C + c
    const bool live = i < KK * C;
    const int q = (P + kFin - 1) / kFin;
    float s0 = 0.f;
    if (live) {
        const int pe = min(P, (ty + 1) * q);
        for (int p = ty * q; p < pe; ++p) s0 += partw[(size_t)p * KK * C + i];
    }
    for (int s = kFin / 2; s >= 1; s >>= 1) {
        if (ty >= s && ty < 2 * s) sm[BN_SLOT(0)] = s0;
        __syncthreads();
        if (ty < s) s0 += sm[BN_SLOT_AT(0, ty + s)];
        __syncthreads();
    }
    if (ty == 0 && live) {
        const int t = i / C, c = i - t * C;
        gw[(size_t)c * KK + t] = s0;
    }
}

struct Fwd {
    const void* x; const float *a, *w, *b, *gamma, *beta; float *rm, *rv; void* y; float *u, *mean_u, *invstd_u, *ws;
    int N, C; Geo g; float mom, eps;
};
struct Bwd {
    const void* x; const float *a, *u; const void* gy; const float *w, *gamma, *mean_u, *invstd_u;
    void* gx; float *ga, *gw, *gb, *ggamma, *gbeta, *ws;
    int N, C; Geo g;
};

inline dim3 fin_grid(int n) { return dim3((unsigned)((n + kFin - 1) / kFin)); }
inline int rows_out(const Geo& g, int N) { return N * g.Ho * g.Wo; }

// workspace: (S0, Su) (2 C floats), then the partials of the launch in flight (P x 2 C or P x K K C floats)
template <typename T, int V, int K>
hipError_t fwd(const Fwd& a, hipStream_t s)
{
    const int R = rows_out(a.g, a.N), C = a.C;
    const Plan p = bn::stats_plan(R, C, V), q = bn::apply_plan(R, C, V);
    float* part = a.ws + 2 * (size_t)C;
    hipLaunchKernelGGL((k_dwbn_stats<T, V, K>), bn::grid_of(p), bn::block_of(p), 0, s, (const T*)a.x, a.a, a.w, a.b, a.u, part, a.g, R, C, p.G, p.RB);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_dwbn_finalize, fin_grid(C), dim3(kFin, kFin), 0, s, (const float*)part, a.mean_u, a.invstd_u, a.rm, a.rv, R, C, p.RB, p.P, a.mom, a.eps);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL((k_dwbn_apply<T, V>), bn::grid_of(q), bn::block_of(q), 0, s, (const float*)a.u, (T*)a.y, a.gamma, a.beta, (const float*)a.mean_u,
                       (const float*)a.invstd_u, R, C, q.G, q.RB);
    return hipGetLastError();
}

template <typename T, int V, int K>
hipError_t bwd(const Bwd& a, hipStream_t s)
{
    const int R = rows_out(a.g, a.N), C = a.C;
    const Plan p = bn::stats_plan(R, C, V);
    float* part = a.ws + 2 * (size_t)C;
    hipLaunchKernelGGL((k_dwbn_bwd_sums<T, V>), bn::grid_of(p), bn::block_of(p), 0, s, a.u, (const T*)a.gy, a.mean_u, a.invstd_u, part, R, C, p.G, p.RB);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_dwbn_bwd_finalize, fin_grid(C), dim3(kFin, kFin), 0, s, (const float*)part, a.ws, a.gb, a.ggamma, a.gbeta, C, p.P);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (a.a && (a.gx || a.ga)) {
        const int Rc = a.N * a.g.Hc * a.g.Wc;
        const Plan q = bn::apply_plan(Rc, C, V);
        hipLaunchKernelGGL((k_dwbn_bwd_dx_up<T, V, K>), bn::grid_of(q), bn::block_of(q), 0, s, a.u, (const T*)a.gy, (T*)a.gx, a.ga, a.w, a.gamma, a.mean_u, a.invstd_u,
                           (const float*)a.ws, a.g, R, Rc, C, q.G, q.RB);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    } else if (a.gx) {
        const int Rin = a.N * a.g.H * a.g.W;
        const Plan q = bn::apply_plan(Rin, C, V);
        hipLaunchKernelGGL((k_dwbn_bwd_dx<T, V, K>), bn::grid_of(q), bn::block_of(q), 0, s, a.u, (const T*)a.gy, (T*)a.gx, a.w, a.gamma, a.mean_u, a.invstd_u,
                           (const float*)a.ws, a.g, R, Rin, C, q.G, q.RB);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (a.gw) {
        dim3 grid = bn::grid_of(p);
        grid.z = K;
        hipLaunchKernelGGL((k_dwbn_bwd_gw<T, V, K>), grid, bn::block_of(p), 0, s, (const T*)a.x, a.a, a.u, (const T*)a.gy, a.gamma, a.mean_u, a.invstd_u,
                           (const float*)a.ws, part, a.g, R, C, p.G, p.RB);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        hipLaunchKernelGGL(k_dwbn_bwd_gw_fin, fin_grid(K * K * C), dim3(kFin, kFin), 0, s, (const float*)part, a.gw, C, K * K, p.P);
        return hipGetLastError();
    }
    return hipSuccess;
}

inline Geo geo_of(int H, int W, int Hc, int Wc, int stride)
{
    Geo g{H, W, (H - 1) / stride + 1, (W - 1) / stride + 1, Hc, Wc, stride, 0.f, 0.f};
    if (Hc > 0) { g.sy = (float)Hc / (float)H; g.sx = (float)Wc / (float)W; }
    return g;
}

// F<T, V, K>(args...) on the element type of `dtype`, V-wide where `wide`, K = 3 | 5
#define DWBN_DISPATCH_K(fn, T, W, k, ...) ((k) == 3 ? ((wide) ? fn<T, W, 3>(__VA_ARGS__) : fn<T, 1, 3>(__VA_ARGS__)) : ((wide) ? fn<T, W, 5>(__VA_ARGS__) : fn<T, 1, 5>(__VA_ARGS__)))
#define DWBN_DISPATCH(fn, dtype, k, ...)                                   \
    switch (dtype) {                                                       \
        case 0: return DWBN_DISPATCH_K(fn, float, 4, k, __VA_ARGS__);      \
        case 1: return DWBN_DISPATCH_K(fn, bf16_t, 8, k, __VA_ARGS__);     \
        case 2: return DWBN_DISPATCH_K(fn, f16_t, 8, k, __VA_ARGS__);      \
        default: return hipErrorInvalidValue;                              \
    }

}  // namespace dwbn

bool dwconv_bn_train_applicable(long long N, long long H, long long W, long long C, int k, int stride, int has_coarse, int dtype)
{
    if ((k != 3 && k != 5) || (stride != 1 && stride != 2) || (has_coarse != 0 && has_coarse != 1) || (has_coarse && stride != 1)) return false;
    return batchnorm_applicable(N, H, W, C, dtype);
}

size_t dwconv_bn_train_workspace_bytes(int N, int H, int W, int C, int k, int stride, int dtype)
{
    const int R = N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
    const bn::Plan w = bn::stats_plan(R, C, C % bn::wide_v(dtype) ? 1 : bn::wide_v(dtype)), n = bn::stats_plan(R, C, 1);
    const int P = w.P > n.P ? w.P : n.P;
    return sizeof(float) * ((size_t)P * k * k * C + 2 * (size_t)C);
}

hipError_t dwconv_bn_train_fwd(const void* x, const float* a, int Hc, int Wc, const float* w, const float* b, const float* gamma, const float* beta, float* rm,
                               float* rv, void* y, float* u, float* mean_u, float* invstd_u, void* workspace, int N, int H, int W, int C, int k, int stride,
                               float momentum, float eps, int dtype, hipStream_t s)
{
    const dwbn::Fwd f{x, a, w, b, gamma, beta, rm, rv, y, u, mean_u, invstd_u, (float*)workspace, N, C, dwbn::geo_of(H, W, a ? Hc : 0, a ? Wc : 0, stride), momentum, eps};
    const bool wide = bn::can_wide(C, dtype, {x, a, b, gamma, beta, y, u, mean_u, invstd_u, workspace});
    DWBN_DISPATCH(dwbn::fwd, dtype, k, f, s)
}

hipError_t dwconv_bn_train_bwd(const void* x, const float* a, int Hc, int Wc, const float* u, const void* gy, const float* w, const float* gamma, const float* mean_u,
                               const float* invstd_u, void* gx, float* ga, float* gw, float* gb, float* ggamma, float* gbeta, void* workspace, int N, int H, int W,
                               int C, int k, int stride, int dtype, hipStream_t s)
{
    const dwbn::Bwd f{x, a, u, gy, w, gamma, mean_u, invstd_u, gx, ga, gw, gb, ggamma, gbeta, (float*)workspace, N, C, dwbn::geo_of(H, W, a ? Hc : 0, a ? Wc : 0, stride)};
    const bool wide = bn::can_wide(C, dtype, {x, a, u, gy, gamma, mean_u, invstd_u, gx, ga, workspace});
    DWBN_DISPATCH(dwbn::bwd, dtype, k, f, s)
}

}  // namespace rcx

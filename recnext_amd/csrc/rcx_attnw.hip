// Linear-attention core with separate q / k and v widths, up to 128 channels a head (the LSNet-style RecNeXt-T / S / B in training):
//
//     q = elu(qpre) + 1,  k = elu(kpre) + 1                               qpre, kpre: (B, n, Cqk), head h owns channels [h Dk, (h+1) Dk)
//     kv = (1/n) k^T v,  kbar = mean_tokens(k)                            v: (B, n, Cv), head h owns channels [h Dv, (h+1) Dv)
//     out = q kv / (q . kbar + 1e-6) + pe                                  pe, out: (B, n, Cv)
//
// lsnet/model/recattn.py:97-109 (LinearAttention3: Dk = s/2 / heads, Dv = s / heads) and, with Dk = Dv, :45-56 / :71-82 (LinearAttention1 / 2 of
// 96-channel heads).  rcx_attn.hip keeps the heads of at most 64 channels with Dk = Dv; this unit takes Dk, Dv = 4, 8 .. 128 in any pairing.
//
// One workgroup per (image, head), 256 threads, all arithmetic float32 whatever the I/O type.  Tokens stream through LDS in tiles of
// LW_TT; kv (Dk x Dv, rows padded by four floats) stays in LDS for the whole launch.  Every sum runs over its index in ascending order in a
// single thread (the k^T v sums: 4 x 4 register blocks, one owner thread each), so the results are bitwise deterministic and an image's
// results do not depend on the others in the batch.  No atomics.
//
// Backward (the derivation above k_linattn_bwd in rcx_attn.hip, with the Dv columns kept apart from the Dk rows).  With u = q kv,
// w = q . kbar + 1e-6 and g = dL/dout:
//     du = g / w,  dw = -(g . u) / w^2,  dq = du kv^T + dw kbar,  dkv = q^T du,  dkbar = q^T dw
//     dk = (v dkv^T + dkbar) / n,  dv = k dkv / n,  then elu'(x) = min(elu(x) + 1, 1) on both pre-activations
// Three sweeps over the tokens: kv and kbar; u, w, dq and the dkv / dkbar sums; dk and dv.  dkv overwrites kv in LDS between the second
// and the third sweep, so one Dk x Dv matrix is resident at a time.
#include "rcx_common.h"
#include "rcx_launch.h"

namespace rcx {

namespace attnw {

constexpr int LW_NT = 256;              // threads per workgroup
constexpr int LW_TT = 32;               // tokens per LDS tile
constexpr int LW_DMAX = 128;            // widest head (q / k and v alike)
constexpr int LW_BLOCKS = (LW_DMAX / 4) * (LW_DMAX / 4) / LW_NT;   // 4 x 4 blocks of k^T v per thread at 128 x 128: 4
constexpr int LW_LDS_LIMIT = 160 * 1024;

__device__ __forceinline__ float elu1w(float x) { return x > 0.f ? x + 1.f : __expf(x); }

template <typename T> __device__ __forceinline__ void ld4(const T* p, float (&o)[4]) { load_vec<4>(p, o); }
template <typename T> __device__ __forceinline__ void st4(T* p, const float (&o)[4]) { store_vec<4>(p, o); }
__device__ __forceinline__ float4 lds4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void lds4_st(float* p, const float (&o)[4]) { *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]); }

__host__ __device__ __forceinline__ int kv_pitch(int Dv) { return Dv + 4; }     // consecutive rows of kv start four banks apart

// LDS floats: kv, kbar, (dkbar, w, dw), the token tiles (k / q: LW_TT x Dk; v / g: LW_TT x Dv; bwd also g * u: LW_TT x Dv), den
__host__ __device__ __forceinline__ size_t fwd_lds_floats(int Dk, int Dv)
{
    return (size_t)Dk * kv_pitch(Dv) + Dk + (size_t)LW_TT * Dk + (size_t)LW_TT * Dv + LW_TT;
}
__host__ __device__ __forceinline__ size_t bwd_lds_floats(int Dk, int Dv)
{
    return (size_t)Dk * kv_pitch(Dv) + 2 * (size_t)Dk + 2 * LW_TT + (size_t)LW_TT * Dk + 2 * (size_t)LW_TT * Dv;
}

// kv-style sums over one token tile: acc[j] (4 x 4 block `it` = tid + j * LW_NT of the Dk x Dv matrix) += a[t][rows] x b[t][cols], t ascending
__device__ __forceinline__ void tile_outer(float (&acc)[LW_BLOCKS][16], const float* a_s, const float* b_s, int tt, int Dk, int Dv)
{
    const int Qv = Dv / 4, items = (Dk / 4) * Qv;
#pragma unroll
    for (int j = 0; j < LW_BLOCKS; ++j) {
        const int it = threadIdx.x + j * LW_NT;
        if (it < items) {
            const int r4 = (it / Qv) * 4, c4 = (it % Qv) * 4;
            for (int t = 0; t < tt; ++t) {
                const float4 a = lds4(a_s + t * Dk + r4), b = lds4(b_s + t * Dv + c4);
                const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[j][4 * r + c] = fmaf(av[r], bv[c], acc[j][4 * r + c]);
            }
        }
    }
}

__device__ __forceinline__ void store_outer(const float (&acc)[LW_BLOCKS][16], float* m_s, float scale, int Dk, int Dv)
{
    const int Qv = Dv / 4, items = (Dk / 4) * Qv, P = kv_pitch(Dv);
#pragma unroll
    for (int j = 0; j < LW_BLOCKS; ++j) {
        const int it = threadIdx.x + j * LW_NT;
        if (it < items) {
            const int r4 = (it / Qv) * 4, c4 = (it % Qv) * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float o[4] = {acc[j][4 * r] * scale, acc[j][4 * r + 1] * scale, acc[j][4 * r + 2] * scale, acc[j][4 * r + 3] * scale};
                lds4_st(m_s + (size_t)(r4 + r) * P + c4, o);
            }
        }
    }
}

// o[c] = sum_e a[e] m[e][c4 + c], e ascending (a row of Dk, the matrix Dk x Dv): u = q kv, dv = k dkv
__device__ __forceinline__ void row_times_m(const float* a_row, const float* m_s, int c4, int Dk, int P, float (&o)[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = 0.f;
#pragma unroll 4
    for (int e = 0; e < Dk; ++e) {
        const float a = a_row[e];
        const float4 m = lds4(m_s + (size_t)e * P + c4);
        o[0] = fmaf(a, m.x, o[0]); o[1] = fmaf(a, m.y, o[1]); o[2] = fmaf(a, m.z, o[2]); o[3] = fmaf(a, m.w, o[3]);
    }
}

// o[r] = sum_f b[f] m[r4 + r][f], f ascending (a row of Dv against rows r4 .. r4+3 of the matrix): dq = du kv^T, dk = v dkv^T
__device__ __forceinline__ void row_times_mT(const float* b_row, const float* m_s, int r4, int Dv, int P, float (&o)[4])
{
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = 0.f;
    for (int f = 0; f < Dv; f += 4) {
        const float4 b = lds4(b_row + f);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float4 m = lds4(m_s + (size_t)(r4 + r) * P + f);
            o[r] = fmaf(b.x, m.x, o[r]); o[r] = fmaf(b.y, m.y, o[r]); o[r] = fmaf(b.z, m.z, o[r]); o[r] = fmaf(b.w, m.w, o[r]);
        }
    }
}

// sweep 1 of both kernels: kv (scaled 1/n) and kbar into LDS.  a_s / b_s: the token tiles.  Ends with a barrier.
template <typename T>
__device__ __forceinline__ void sweep_kv(const T* __restrict__ kpre, const T* __restrict__ v, size_t qk_base, size_t v_base, int n, int Cqk, int Cv,
                                         int Dk, int Dv, float* a_s, float* b_s, float* kv_s, float* kbar_s)
{
    const int tid = threadIdx.x, Qk = Dk / 4, Qv = Dv / 4;
    float acc[LW_BLOCKS][16];
#pragma unroll
    for (int j = 0; j < LW_BLOCKS; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    float ksum = 0.f;
    for (int t0 = 0; t0 < n; t0 += LW_TT) {
        const int tt = min(LW_TT, n - t0);
        __syncthreads();
        for (int i = tid; i < tt * Qk; i += LW_NT) {
            const int t = i / Qk, e = (i - t * Qk) * 4;
            float kk[4];
            ld4(kpre + qk_base + (size_t)(t0 + t) * Cqk + e, kk);
#pragma unroll
            for (int c = 0; c < 4; ++c) kk[c] = elu1w(kk[c]);
            lds4_st(a_s + t * Dk + e, kk);
        }
        for (int i = tid; i < tt * Qv; i += LW_NT) {
            const int t = i / Qv, e = (i - t * Qv) * 4;
            float vv[4];
            ld4(v + v_base + (size_t)(t0 + t) * Cv + e, vv);
            lds4_st(b_s + t * Dv + e, vv);
        }
        __syncthreads();
        tile_outer(acc, a_s, b_s, tt, Dk, Dv);
        if (tid < Dk)
            for (int t = 0; t < tt; ++t) ksum += a_s[t * Dk + tid];
    }
    store_outer(acc, kv_s, 1.f / (float)n, Dk, Dv);
    if (tid < Dk) kbar_s[tid] = ksum / (float)n;
    __syncthreads();
}

template <typename T>
__global__ void __launch_bounds__(LW_NT)
k_linattn_wide_fwd(const T* __restrict__ qpre, const T* __restrict__ kpre, const T* __restrict__ v, const T* __restrict__ pe,
                   T* __restrict__ out, int n, int Cqk, int Cv, int heads)
{
    extern __shared__ __attribute__((aligned(16))) float lds_lw[];
    const int Dk = Cqk / heads, Dv = Cv / heads, P = kv_pitch(Dv), Qk = Dk / 4, Qv = Dv / 4;
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const size_t qk_base = (size_t)b * n * Cqk + (size_t)h * Dk, v_base = (size_t)b * n * Cv + (size_t)h * Dv;
    const int tid = threadIdx.x;
    float* kv_s = lds_lw;                               // Dk x P
    float* kbar_s = kv_s + (size_t)Dk * P;              // Dk
    float* a_s = kbar_s + Dk;                           // LW_TT x Dk: k, then q
    float* b_s = a_s + LW_TT * Dk;                      // LW_TT x Dv: v
    float* den_s = b_s + LW_TT * Dv;                    // LW_TT

    sweep_kv(kpre, v, qk_base, v_base, n, Cqk, Cv, Dk, Dv, a_s, b_s, kv_s, kbar_s);

    for (int t0 = 0; t0 < n; t0 += LW_TT) {
        const int tt = min(LW_TT, n - t0);
        __syncthreads();
        for (int i = tid; i < tt * Qk; i += LW_NT) {
            const int t = i / Qk, e = (i - t * Qk) * 4;
            float qq[4];
            ld4(qpre + qk_base + (size_t)(t0 + t) * Cqk + e, qq);
#pragma unroll
            for (int c = 0; c < 4; ++c) qq[c] = elu1w(qq[c]);
            lds4_st(a_s + t * Dk + e, qq);
        }
        __syncthreads();
        if (tid < tt) {
            float d = 0.f;
            for (int e = 0; e < Dk; ++e) d = fmaf(a_s[tid * Dk + e], kbar_s[e], d);
            den_s[tid] = d + 1e-6f;
        }
        __syncthreads();
        for (int i = tid; i < tt * Qv; i += LW_NT) {
            const int t = i / Qv, c4 = (i - t * Qv) * 4;
            float o[4], pp[4];
            row_times_m(a_s + t * Dk, kv_s, c4, Dk, P, o);
            const size_t g = v_base + (size_t)(t0 + t) * Cv + c4;
            ld4(pe + g, pp);
            const float inv = 1.f / den_s[t];
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = fmaf(o[c], inv, pp[c]);
            st4(out + g, o);
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(LW_NT)
k_linattn_wide_bwd(const T* __restrict__ qpre, const T* __restrict__ kpre, const T* __restrict__ v, const T* __restrict__ gout,
                   T* __restrict__ gq, T* __restrict__ gk, T* __restrict__ gv, int n, int Cqk, int Cv, int heads)
{
    extern __shared__ __attribute__((aligned(16))) float lds_lw[];
    const int Dk = Cqk / heads, Dv = Cv / heads, P = kv_pitch(Dv), Qk = Dk / 4, Qv = Dv / 4;
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const size_t qk_base = (size_t)b * n * Cqk + (size_t)h * Dk, v_base = (size_t)b * n * Cv + (size_t)h * Dv;
    const int tid = threadIdx.x;
    float* kv_s = lds_lw;                               // Dk x P: kv, then dkv
    float* kbar_s = kv_s + (size_t)Dk * P;              // Dk
    float* dkbar_s = kbar_s + Dk;                       // Dk
    float* w_s = dkbar_s + Dk;                          // LW_TT
    float* dw_s = w_s + LW_TT;                          // LW_TT
    float* a_s = dw_s + LW_TT;                          // LW_TT x Dk: k / q / k
    float* b_s = a_s + LW_TT * Dk;                      // LW_TT x Dv: v / g, then du / v
    float* c_s = b_s + LW_TT * Dv;                      // LW_TT x Dv: g * u
    const float inv_n = 1.f / (float)n;

    sweep_kv(kpre, v, qk_base, v_base, n, Cqk, Cv, Dk, Dv, a_s, b_s, kv_s, kbar_s);

    // ---- sweep 2: u, w, du, dw; dq -> gq; dkv += q^T du, dkbar += q^T dw
    float acc[LW_BLOCKS][16];
#pragma unroll
    for (int j = 0; j < LW_BLOCKS; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    float dkb = 0.f;
    for (int t0 = 0; t0 < n; t0 += LW_TT) {
        const int tt = min(LW_TT, n - t0);
        __syncthreads();
        for (int i = tid; i < tt * Qk; i += LW_NT) {
            const int t = i / Qk, e = (i - t * Qk) * 4;
            float qq[4];
            ld4(qpre + qk_base + (size_t)(t0 + t) * Cqk + e, qq);
#pragma unroll
            for (int c = 0; c < 4; ++c) qq[c] = elu1w(qq[c]);
            lds4_st(a_s + t * Dk + e, qq);
        }
        for (int i = tid; i < tt * Qv; i += LW_NT) {
            const int t = i / Qv, e = (i - t * Qv) * 4;
            float gg[4];
            ld4(gout + v_base + (size_t)(t0 + t) * Cv + e, gg);
            lds4_st(b_s + t * Dv + e, gg);
        }
        __syncthreads();
        for (int i = tid; i < tt * Qv; i += LW_NT) {            // g * u, elementwise
            const int t = i / Qv, c4 = (i - t * Qv) * 4;
            float u[4];
            row_times_m(a_s + t * Dk, kv_s, c4, Dk, P, u);
            const float4 g = lds4(b_s + t * Dv + c4);
            const float gu[4] = {g.x * u[0], g.y * u[1], g.z * u[2], g.w * u[3]};
            lds4_st(c_s + t * Dv + c4, gu);
        }
        __syncthreads();
        if (tid < tt) {                                         // one thread per token: w and dw
            float ws = 0.f, gu = 0.f;
            for (int e = 0; e < Dk; ++e) ws = fmaf(a_s[tid * Dk + e], kbar_s[e], ws);
            for (int e = 0; e < Dv; ++e) gu += c_s[tid * Dv + e];
            ws += 1e-6f;
            w_s[tid] = ws;
            dw_s[tid] = -gu / (ws * ws);
        }
        __syncthreads();
        for (int i = tid; i < tt * Qv; i += LW_NT) {            // du = g / w, in place
            const int t = i / Qv, e = (i - t * Qv) * 4;
            const float4 g = lds4(b_s + t * Dv + e);
            const float wt = w_s[t];
            const float du[4] = {g.x / wt, g.y / wt, g.z / wt, g.w / wt};
            lds4_st(b_s + t * Dv + e, du);
        }
        __syncthreads();
        for (int i = tid; i < tt * Qk; i += LW_NT) {            // dq = du kv^T + dw kbar, times elu'(qpre)
            const int t = i / Qk, r4 = (i - t * Qk) * 4;
            float dq[4];
            row_times_mT(b_s + t * Dv, kv_s, r4, Dv, P, dq);
            const float4 q = lds4(a_s + t * Dk + r4);
            const float qv[4] = {q.x, q.y, q.z, q.w};
            const float dwt = dw_s[t];
#pragma unroll
            for (int r = 0; r < 4; ++r) dq[r] = fmaf(dwt, kbar_s[r4 + r], dq[r]) * fminf(qv[r], 1.f);
            st4(gq + qk_base + (size_t)(t0 + t) * Cqk + r4, dq);
        }
        tile_outer(acc, a_s, b_s, tt, Dk, Dv);                  // dkv += q^T du
        if (tid < Dk)
            for (int t = 0; t < tt; ++t) dkb = fmaf(dw_s[t], a_s[t * Dk + tid], dkb);
    }
    __syncthreads();                                            // every read of kv is done: dkv takes its place
    store_outer(acc, kv_s, inv_n, Dk, Dv);
    if (tid < Dk) dkbar_s[tid] = dkb * inv_n;

    // ---- sweep 3: dk = v dkv^T + dkbar, dv = k dkv
    for (int t0 = 0; t0 < n; t0 += LW_TT) {
        const int tt = min(LW_TT, n - t0);
        __syncthreads();
        for (int i = tid; i < tt * Qk; i += LW_NT) {
            const int t = i / Qk, e = (i - t * Qk) * 4;
            float kk[4];
            ld4(kpre + qk_base + (size_t)(t0 + t) * Cqk + e, kk);
#pragma unroll
            for (int c = 0; c < 4; ++c) kk[c] = elu1w(kk[c]);
            lds4_st(a_s + t * Dk + e, kk);
        }
        for (int i = tid; i < tt * Qv; i += LW_NT) {
            const int t = i / Qv, e = (i - t * Qv) * 4;
            float vv[4];
            ld4(v + v_base + (size_t)(t0 + t) * Cv + e, vv);
            lds4_st(b_s + t * Dv + e, vv);
        }
        __syncthreads();
        for (int i = tid; i < tt * Qk; i += LW_NT) {
            const int t = i / Qk, r4 = (i - t * Qk) * 4;
            float dk[4];
            row_times_mT(b_s + t * Dv, kv_s, r4, Dv, P, dk);
            const float4 k = lds4(a_s + t * Dk + r4);
            const float kv4[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) dk[r] = (dk[r] + dkbar_s[r4 + r]) * fminf(kv4[r], 1.f);
            st4(gk + qk_base + (size_t)(t0 + t) * Cqk + r4, dk);
        }
        for (int i = tid; i < tt * Qv; i += LW_NT) {
            const int t = i / Qv, c4 = (i - t * Qv) * 4;
            float dv[4];
            row_times_m(a_s + t * Dk, kv_s, c4, Dk, P, dv);
            st4(gv + v_base + (size_t)(t0 + t) * Cv + c4, dv);
        }
    }
}

bool head_ok(int d) { return d >= 4 && d <= LW_DMAX && d % 4 == 0; }

template <typename T>
hipError_t launch_wide_fwd(const void* qpre, const void* kpre, const void* v, const void* pe, void* out, int B, int n, int Cqk, int Cv, int heads,
                           hipStream_t s)
{
    const size_t lds = sizeof(float) * fwd_lds_floats(Cqk / heads, Cv / heads);
    RCX_SET_LDS_ONCE((k_linattn_wide_fwd<T>), lds);
    hipLaunchKernelGGL((k_linattn_wide_fwd<T>), dim3((unsigned)(B * heads)), dim3(LW_NT), lds, s, (const T*)qpre, (const T*)kpre, (const T*)v,
                       (const T*)pe, (T*)out, n, Cqk, Cv, heads);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_wide_bwd(const void* qpre, const void* kpre, const void* v, const void* gout, void* gq, void* gk, void* gv, int B, int n, int Cqk,
                           int Cv, int heads, hipStream_t s)
{
    const size_t lds = sizeof(float) * bwd_lds_floats(Cqk / heads, Cv / heads);
    RCX_SET_LDS_ONCE((k_linattn_wide_bwd<T>), lds);
    hipLaunchKernelGGL((k_linattn_wide_bwd<T>), dim3((unsigned)(B * heads)), dim3(LW_NT), lds, s, (const T*)qpre, (const T*)kpre, (const T*)v,
                       (const T*)gout, (T*)gq, (T*)gk, (T*)gv, n, Cqk, Cv, heads);
    return hipGetLastError();
}

}  // namespace attnw

bool linattn_wide_applicable(int B, int n, int Cqk, int Cv, int heads, int dtype)
{
    if (B <= 0 || n <= 0 || heads <= 0 || Cqk <= 0 || Cv <= 0 || dtype < 0 || dtype > 2) return false;
    if (Cqk % heads || Cv % heads) return false;
    const int Dk = Cqk / heads, Dv = Cv / heads;
    if (!attnw::head_ok(Dk) || !attnw::head_ok(Dv)) return false;
    if ((long long)B * heads > 0x7fffffffLL || (long long)n * (Cqk > Cv ? Cqk : Cv) > 0x7fffffffLL) return false;
    return sizeof(float) * attnw::bwd_lds_floats(Dk, Dv) <= (size_t)attnw::LW_LDS_LIMIT && sizeof(float) * attnw::fwd_lds_floats(Dk, Dv) <= (size_t)attnw::LW_LDS_LIMIT;
}

hipError_t linattn_wide_fwd(const void* qpre, const void* kpre, const void* v, const void* pe, void* out, int B, int n, int Cqk, int Cv, int heads,
                            int dtype, hipStream_t s)
{
    switch (dtype) {
        case 0: return attnw::launch_wide_fwd<float>(qpre, kpre, v, pe, out, B, n, Cqk, Cv, heads, s);
        case 1: return attnw::launch_wide_fwd<bf16_t>(qpre, kpre, v, pe, out, B, n, Cqk, Cv, heads, s);
        default: return attnw::launch_wide_fwd<f16_t>(qpre, kpre, v, pe, out, B, n, Cqk, Cv, heads, s);
    }
}

hipError_t linattn_wide_bwd(const void* qpre, const void* kpre, const void* v, const void* gout, void* gq, void* gk, void* gv, int B, int n, int Cqk,
                            int Cv, int heads, int dtype, hipStream_t s)
{
    switch (dtype) {
        case 0: return attnw::launch_wide_bwd<float>(qpre, kpre, v, gout, gq, gk, gv, B, n, Cqk, Cv, heads, s);
        case 1: return attnw::launch_wide_bwd<bf16_t>(qpre, kpre, v, gout, gq, gk, gv, B, n, Cqk, Cv, heads, s);
        default: return attnw::launch_wide_bwd<f16_t>(qpre, kpre, v, gout, gq, gk, gv, B, n, Cqk, Cv, heads, s);
    }
}

}  // namespace rcx

// The token half of the LSNet-style RecNeXt-T / S / B blocks at ANY plane size (lsnet/model/recattn.py:8-15, :37-127, :226-237): the function of
// rcx_lsmix.hip's k_ls_slice<T, 1> (RecAttn2d on the slice) and k_ls_slice<T, 0> (LinearAttention3), cut into chunks of tokens so that any number
// of workgroups work on one image.  The attention is global over tokens, so k^T v and sum(k) cross the chunks through the caller's float32 workspace:
//   k_lt_rep   r = RepVGGDW(x) on every channel, a wide grid: r (rounded once), the passthrough channels to t, the slice in float32 to ws_r;
//   k_lt_kv    one workgroup per (image, chunk of Tb attention tokens): v (RecAttn2d: d = dw5 stride 2 of ws_r, kept in ws_d; LinearAttention3: the
//              slice itself), k = elu(W_k v + b_k) + 1 in LDS, then ONE partial k^T v and ONE partial sum(k) per chunk to ws_p;
//   k_lt_out   per (image, chunk): the partials summed chunk 0, 1, 2 ... (a fixed order), q, the normaliser, q kv / (q . mean(k) + 1e-6) + pe(v);
//              LinearAttention3 stores t's slice, RecAttn2d keeps the half-size result in ws_a;
//   k_lt_conv  RecAttn2d only, a wide grid: t's slice = conv5(ws_r + nearest(ws_a)).
// The chunk length Tb depends on the slice width alone (lt_plan), so a batch and its shards run the same schedule on every image; float32
// arithmetic, the elu(.)+1 and the normaliser of k_ls_slice, each of r and t rounded once at its store, no atomics.  The chunks are runs of the
// flattened token index, not rows: no LDS buffer grows with H or W, so every H x W >= 1 x 1 has the same kernels.
#include "rcx_common.h"
#include "rcx_launch.h"

namespace rcx {
namespace {

constexpr int kTileThreads = 256;
constexpr int kTileLdsLimit = 160 * 1024;

__device__ __forceinline__ float elu1(float a) { return a > 0.f ? a + 1.f : expm1f(a) + 1.f; }       // as rcx_lsmix.hip

struct TileArgs {
    const float *w_rep, *b_rep;     // (3, 3, C), (C): the folded RepVGGDW
    const float *w_dn, *b_dn;       // (5, 5, Cs), (Cs): RecAttn2d's stride-2 conv (RecAttn2d only)
    const float *wqT, *bq;          // (Kin, Cq), (Cq): the q projection, transposed; reads v's channels [0, Kin)
    const float *wkT, *bk;          // (Kin, Cq), (Cq): the k projection, transposed; reads v's channels [k_off, k_off + Kin)
    const float *w_pe, *b_pe;       // (3, 3, Cs), (Cs)
    const float *w_cv, *b_cv;       // (5, 5, Cs), (Cs): RecAttn2d's final conv (RecAttn2d only)
    float *ws_r, *ws_d, *ws_a, *ws_p;   // workspace: the fine slice (N HW Cs), d and the attention result (N n Cs each, RecAttn2d only), partials (N nchunk P)
    int N, H, W, C, Cs, heads, Cq, Kin, k_off;
    int hc, wc, n;                  // the attention plane (half size for RecAttn2d, the fine plane for LinearAttention3) and its token count
    int Tb, nchunk, P;              // tokens per chunk, chunks per image, floats of one partial (Cq x dv of k^T v, then Cq of sum(k))
};

// The schedule of a shape; never a function of the batch.
struct TilePlan {
    int hc, wc, n, Tb, nchunk, P;
    size_t lds_kv, lds_out;         // bytes
    size_t off_d, off_a, off_p, ws_floats;   // workspace layout for a batch of B
};

inline int round4(int v) { return (v + 3) & ~3; }

bool lt_plan(int attn, int B, int H, int W, int C, int split, int heads, int dtype, TilePlan& p)
{
    if (!(B > 0 && H > 0 && W > 0 && C > 0 && split > 0 && split <= C && C % 4 == 0 && split % 4 == 0 && dtype >= 0 && dtype <= 2
          && (size_t)B * H * W * C < ((size_t)1 << 31)))
        return false;
    if (attn ? heads != 1 : (heads <= 0 || split % (2 * heads) || (split / heads) % 4)) return false;
    const int Cq = attn ? split : split / 2, dv = split / heads;
    p.hc = attn ? (H + 1) / 2 : H;
    p.wc = attn ? (W + 1) / 2 : W;
    p.n = p.hc * p.wc;
    p.Tb = split <= 64 ? 64 : 32;                       // the band rule: 64 tokens a chunk for slices up to 64 channels, 32 for wider ones
    p.nchunk = (p.n + p.Tb - 1) / p.Tb;
    p.P = Cq * dv + Cq;
    p.lds_kv = sizeof(float) * (size_t)p.Tb * (split + Cq);
    p.lds_out = sizeof(float) * ((size_t)round4(p.P) + (size_t)p.Tb * (split + Cq + heads));
    if (p.lds_kv > (size_t)kTileLdsLimit || p.lds_out > (size_t)kTileLdsLimit) return false;
    const size_t fine = (size_t)B * H * W * split, coarse = attn ? (size_t)B * p.n * split : 0;
    p.off_d = fine;
    p.off_a = fine + coarse;
    p.off_p = fine + 2 * coarse;
    p.ws_floats = p.off_p + (size_t)B * p.nchunk * p.P;
    return p.ws_floats < ((size_t)1 << 31);
}

// r = RepVGGDW(x) on every channel (taps in k_ls_slice's order: the same bits); the slice also in float32 to ws_r, the rest also to t
template <typename T>
__global__ void __launch_bounds__(kTileThreads) k_lt_rep(const T* __restrict__ x, T* __restrict__ r, T* __restrict__ t, TileArgs a)
{
    const int H = a.H, W = a.W, C = a.C;
    const int cv = C >> 2;
    const size_t total = (size_t)a.N * H * W * cv;
    const size_t i = (size_t)blockIdx.x * kTileThreads + threadIdx.x;
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
    if (c < a.Cs) store_vec<4>(a.ws_r + pix * a.Cs + c, acc);
    else store_vec<4>(t + pix * C + c, acc);
}

// out[m][o] = elu(b[o] + sum_c wT[c][o] in[m][off + c]) + 1 for the chunk's tb tokens, `in` and `out` in LDS; four tokens a thread (one weight
// load feeds four FMAs).  `in` has Tb (a multiple of 4) rows, so the rows past tb that a ragged last group reads exist; they are not stored.
__device__ __forceinline__ void project(const float* __restrict__ wT, const float* __restrict__ b, const float* in, float* out, int tb, int Cs, int Cq,
                                        int Kin, int off, int tid)
{
    const int groups = (tb + 3) >> 2;
    for (int e = tid; e < groups * Cq; e += kTileThreads) {
        const int g = e / Cq, o = e - g * Cq;
        const int ml = 4 * g;
        const float* vm = in + (size_t)ml * Cs + off;
        const float b0 = b[o];
        float acc[4] = {b0, b0, b0, b0};
        for (int c = 0; c < Kin; ++c) {
            const float w = wT[(size_t)c * Cq + o];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fmaf(w, vm[i * Cs + c], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (ml + i < tb) out[(size_t)(ml + i) * Cq + o] = elu1(acc[i]);
    }
}

// ATTN = 1: RecAttn2d; ATTN = 0: LinearAttention3
template <int ATTN>
__global__ void __launch_bounds__(kTileThreads) k_lt_kv(TileArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = a.H, W = a.W, Cs = a.Cs, Cq = a.Cq, heads = a.heads, wc = a.wc, n = a.n;
    const int dq = Cq / heads, dv = Cs / heads;
    const int img = blockIdx.x / a.nchunk, ch = blockIdx.x - img * a.nchunk;
    const int m0 = ch * a.Tb;
    const int tb = min(a.Tb, n - m0);
    const int tid = threadIdx.x;
    float* vL = lds;                                   // Tb x Cs
    float* kL = vL + (size_t)a.Tb * Cs;                // Tb x Cq
    const float* rs = a.ws_r + (size_t)img * H * W * Cs;
    const int cs4 = Cs >> 2;

    // 1. v of the chunk: d = dw5 stride 2 (padding 2) of the fine slice, or the fine slice itself
    for (int e = tid; e < tb * cs4; e += kTileThreads) {
        const int ml = e / cs4, c = 4 * (e - ml * cs4);
        const int m = m0 + ml;
        float acc[4];
        if constexpr (ATTN) {
            const int qy = m / wc, qx = m - qy * wc;
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
            store_vec<4>(a.ws_d + ((size_t)img * n + m) * Cs + c, acc);
        } else {
            load_vec<4>(rs + (size_t)m * Cs + c, acc);
        }
        store_vec<4>(vL + (size_t)ml * Cs + c, acc);
    }
    __syncthreads();

    // 2. k = elu(W_k v + b_k) + 1
    project(a.wkT, a.bk, vL, kL, tb, Cs, Cq, a.Kin, a.k_off, tid);
    __syncthreads();

    // 3. the chunk's partial k^T v (unscaled; k_lt_out applies n^-1) and partial sum(k), tokens in order
    float* part = a.ws_p + ((size_t)img * a.nchunk + ch) * a.P;
    const int dv4 = dv >> 2;
    for (int e = tid; e < Cq * dv4; e += kTileThreads) {
        const int hi = e / dv4, j = 4 * (e - hi * dv4);        // hi = h dq + i
        const int h = hi / dq;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int m = 0; m < tb; ++m) {
            const float kk = kL[(size_t)m * Cq + hi];
            float v4[4];
            load_vec<4>(vL + (size_t)m * Cs + h * dv + j, v4);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fmaf(kk, v4[i], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) part[(size_t)hi * dv + j + i] = acc[i];
    }
    for (int o = tid; o < Cq; o += kTileThreads) {
        float acc = 0.f;
        for (int m = 0; m < tb; ++m) acc += kL[(size_t)m * Cq + o];
        part[(size_t)Cq * dv + o] = acc;
    }
}

template <typename T, int ATTN>
__global__ void __launch_bounds__(kTileThreads) k_lt_out(T* __restrict__ t, TileArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int C = a.C, Cs = a.Cs, Cq = a.Cq, heads = a.heads, hc = a.hc, wc = a.wc, n = a.n, P = a.P;
    const int dq = Cq / heads, dv = Cs / heads;
    const int img = blockIdx.x / a.nchunk, ch = blockIdx.x - img * a.nchunk;
    const int m0 = ch * a.Tb;
    const int tb = min(a.Tb, n - m0);
    const int tid = threadIdx.x;
    float* kv = lds;                                   // heads x dq x dv, then mean(k) (Cq)
    float* km = kv + (size_t)Cq * dv;
    float* vL = lds + ((P + 3) & ~3);                  // Tb x Cs
    float* qL = vL + (size_t)a.Tb * Cs;                // Tb x Cq
    float* den = qL + (size_t)a.Tb * Cq;               // Tb x heads
    const float* vp = (ATTN ? a.ws_d : a.ws_r) + (size_t)img * n * Cs;
    const int cs4 = Cs >> 2;

    // 1. the image's k^T v n^-1 and mean(k): the chunks' partials in chunk order
    const float* part = a.ws_p + (size_t)img * a.nchunk * P;
    const float s = 1.0f / sqrtf((float)n);
    const float s2 = s * s;
    for (int e = tid; e < P; e += kTileThreads) {
        float acc = 0.f;
        for (int b = 0; b < a.nchunk; ++b) acc += part[(size_t)b * P + e];
        kv[e] = e < Cq * dv ? acc * s2 : acc / (float)n;
    }
    // 2. v of the chunk
    for (int e = tid; e < tb * cs4; e += kTileThreads) {
        float v4[4];
        load_vec<4>(vp + (size_t)m0 * Cs + 4 * (size_t)e, v4);
        store_vec<4>(vL + 4 * (size_t)e, v4);
    }
    __syncthreads();
    // 3. q = elu(W_q v + b_q) + 1 and the normaliser q . mean(k) + 1e-6 per token and head
    project(a.wqT, a.bq, vL, qL, tb, Cs, Cq, a.Kin, 0, tid);
    __syncthreads();
    for (int e = tid; e < tb * heads; e += kTileThreads) {
        const int m = e / heads, h = e - m * heads;
        float acc = 0.f;
        for (int i = 0; i < dq; ++i) acc = fmaf(qL[(size_t)m * Cq + h * dq + i], km[h * dq + i], acc);
        den[e] = acc + 1e-6f;
    }
    __syncthreads();
    // 4. o = q kv / den + pe(v), pe's neighbours from the workspace plane
    for (int e = tid; e < tb * cs4; e += kTileThreads) {
        const int ml = e / cs4, j = 4 * (e - ml * cs4);
        const int h = j / dv, jj = j - h * dv;
        const float* qm = qL + (size_t)ml * Cq + h * dq;
        const float* kvh = kv + (size_t)h * dq * dv + jj;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < dq; ++i) {
            float k4[4];
            load_vec<4>(kvh + (size_t)i * dv, k4);
            const float qv = qm[i];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = fmaf(qv, k4[u], acc[u]);
        }
        const int m = m0 + ml;
        const int my = m / wc, mx = m - my * wc;
        float pe[4];
        load_vec<4>(a.b_pe + j, pe);
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = my + ky - 1;
            if (yy < 0 || yy >= hc) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = mx + kx - 1;
                if (xx < 0 || xx >= wc) continue;
                float sv[4], wt[4];
                load_vec<4>(vp + (size_t)(yy * wc + xx) * Cs + j, sv);
                load_vec<4>(a.w_pe + (ky * 3 + kx) * Cs + j, wt);
#pragma unroll
                for (int u = 0; u < 4; ++u) pe[u] = fmaf(wt[u], sv[u], pe[u]);
            }
        }
        const float dn = den[ml * heads + h];
        float o[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) o[u] = acc[u] / dn + pe[u];
        if constexpr (ATTN) store_vec<4>(a.ws_a + ((size_t)img * n + m) * Cs + j, o);
        else store_vec<4>(t + ((size_t)img * n + m) * C + j, o);
    }
}

// RecAttn2d: t's slice = conv5(r_s + nearest(o)) (padding 2); each fine pixel has one nearest source
template <typename T>
__global__ void __launch_bounds__(kTileThreads) k_lt_conv(T* __restrict__ t, TileArgs a)
{
    const int H = a.H, W = a.W, C = a.C, Cs = a.Cs, hc = a.hc, wc = a.wc;
    const int cs4 = Cs >> 2;
    const size_t total = (size_t)a.N * H * W * cs4;
    const size_t i = (size_t)blockIdx.x * kTileThreads + threadIdx.x;
    if (i >= total) return;
    const int c = 4 * (int)(i % cs4);
    const size_t pix = i / cs4;
    const int px = (int)(pix % W);
    const int py = (int)((pix / W) % H);
    const size_t img = pix / ((size_t)H * W);
    const float* rs = a.ws_r + img * H * W * Cs;
    const float* as = a.ws_a + img * a.n * Cs;
    const float sy = (float)hc / (float)H, sx = (float)wc / (float)W;
    float acc[4];
    load_vec<4>(a.b_cv + c, acc);
    for (int ky = 0; ky < 5; ++ky) {
        const int yy = py + ky - 2;
        if (yy < 0 || yy >= H) continue;
        const int ny = nearest_src(yy, hc, sy);
        for (int kx = 0; kx < 5; ++kx) {
            const int xx = px + kx - 2;
            if (xx < 0 || xx >= W) continue;
            const int nx = nearest_src(xx, wc, sx);
            float rv[4], av[4], wt[4];
            load_vec<4>(rs + (size_t)(yy * W + xx) * Cs + c, rv);
            load_vec<4>(as + (size_t)(ny * wc + nx) * Cs + c, av);
            load_vec<4>(a.w_cv + (ky * 5 + kx) * Cs + c, wt);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(wt[j], rv[j] + av[j], acc[j]);
        }
    }
    store_vec<4>(t + pix * C + c, acc);
}

template <typename T, int ATTN>
hipError_t launch_lt(const void* x, void* r, void* t, const TileArgs& a, const TilePlan& p, hipStream_t s)
{
    const T* xp = (const T*)x;
    T* rp = (T*)r;
    T* tp = (T*)t;
    const size_t pix = (size_t)a.N * a.H * a.W;
    const size_t rep = pix * (a.C >> 2);
    hipLaunchKernelGGL((k_lt_rep<T>), dim3((unsigned)((rep + kTileThreads - 1) / kTileThreads)), dim3(kTileThreads), 0, s, xp, rp, tp, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned chunks = (unsigned)a.N * (unsigned)a.nchunk;
    RCX_SET_LDS_ONCE((k_lt_kv<ATTN>), p.lds_kv);
    hipLaunchKernelGGL((k_lt_kv<ATTN>), dim3(chunks), dim3(kTileThreads), p.lds_kv, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    RCX_SET_LDS_ONCE((k_lt_out<T, ATTN>), p.lds_out);
    hipLaunchKernelGGL((k_lt_out<T, ATTN>), dim3(chunks), dim3(kTileThreads), p.lds_out, s, tp, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if constexpr (ATTN) {
        const size_t cv = pix * (a.Cs >> 2);
        hipLaunchKernelGGL((k_lt_conv<T>), dim3((unsigned)((cv + kTileThreads - 1) / kTileThreads)), dim3(kTileThreads), 0, s, tp, a);
        e = hipGetLastError();
    }
    return e;
}

template <int ATTN>
hipError_t launch_lt_dt(const void* x, void* r, void* t, const TileArgs& a, const TilePlan& p, int dt, hipStream_t s)
{
    switch (dt) {
        case 0: return launch_lt<float, ATTN>(x, r, t, a, p, s);
        case 1: return launch_lt<bf16_t, ATTN>(x, r, t, a, p, s);
        case 2: return launch_lt<f16_t, ATTN>(x, r, t, a, p, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

// RecAttn2d on the slice, one head, any plane
bool ls_recattn_tiled_applicable(int B, int H, int W, int C, int split, int heads, int dtype)
{
    TilePlan p;
    return lt_plan(1, B, H, W, C, split, heads, dtype, p);
}

// LinearAttention3 on the slice (`heads` = the module's own num_heads), any plane; heads of v in fours
bool ls_la3_tiled_applicable(int B, int H, int W, int C, int split, int heads, int dtype)
{
    TilePlan p;
    return lt_plan(0, B, H, W, C, split, heads, dtype, p);
}

size_t ls_recattn_tiled_workspace_bytes(int B, int H, int W, int C, int split, int heads, int dtype)
{
    TilePlan p;
    return lt_plan(1, B, H, W, C, split, heads, dtype, p) ? sizeof(float) * p.ws_floats : 0;
}

size_t ls_la3_tiled_workspace_bytes(int B, int H, int W, int C, int split, int heads, int dtype)
{
    TilePlan p;
    return lt_plan(0, B, H, W, C, split, heads, dtype, p) ? sizeof(float) * p.ws_floats : 0;
}

hipError_t ls_recattn_tiled_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const float* w_dn, const float* b_dn,
                                const float* wqT, const float* bq, const float* wkT, const float* bk, const float* w_pe, const float* b_pe,
                                const float* w_cv, const float* b_cv, void* workspace, int B, int H, int W, int C, int split, int dtype, hipStream_t s)
{
    TilePlan p;
    if (!lt_plan(1, B, H, W, C, split, 1, dtype, p)) return hipErrorInvalidValue;
    float* ws = (float*)workspace;
    const TileArgs a{w_rep, b_rep, w_dn, b_dn, wqT, bq, wkT, bk, w_pe, b_pe, w_cv, b_cv, ws, ws + p.off_d, ws + p.off_a, ws + p.off_p,
                     B, H, W, C, split, 1, split, split / 2, split / 2, p.hc, p.wc, p.n, p.Tb, p.nchunk, p.P};
    return launch_lt_dt<1>(x, r, t, a, p, dtype, s);
}

hipError_t ls_la3_tiled_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const float* wqT, const float* bq,
                            const float* wkT, const float* bk, const float* w_pe, const float* b_pe, void* workspace, int B, int H, int W, int C,
                            int split, int heads, int dtype, hipStream_t s)
{
    TilePlan p;
    if (!lt_plan(0, B, H, W, C, split, heads, dtype, p)) return hipErrorInvalidValue;
    float* ws = (float*)workspace;
    const TileArgs a{w_rep, b_rep, nullptr, nullptr, wqT, bq, wkT, bk, w_pe, b_pe, nullptr, nullptr, ws, nullptr, nullptr, ws + p.off_p,
                     B, H, W, C, split, heads, split / 2, split, 0, p.hc, p.wc, p.n, p.Tb, p.nchunk, p.P};
    return launch_lt_dt<0>(x, r, t, a, p, dtype, s);
}

}  // namespace rcx

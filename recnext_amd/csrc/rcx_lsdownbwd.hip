// Backward of Downsample.token_mixer of the LSNet-style RecNeXt-T / S / B and of their share-channel variants (lsnet/model/recattn.py:254-263,
// recattn_share_channel.py:223-232; the forward is rcx_lsdown.hip): the grouped 5x5 stride-2 conv with 1 .. 4 channels a group in and out, NHWC.
//     gx[n, iy, ix, g ci + j] = sum_{ky, kx, u} wpack[((ky 5 + kx) ci + j) Cout + g co + u] * gy[n, (iy + 2 - ky) / 2, (ix + 2 - kx) / 2, g co + u]
//     gw[((ky 5 + kx) ci + j) Cout + g co + u] = sum_{n, oy, ox} gy[n, oy, ox, g co + u] * x[n, 2 oy + ky - 2, 2 ox + kx - 2, g ci + j],   gb[o] = sum gy
// (the quotients integral and inside the plane).  float32 arithmetic on the vector pipe, no atomics.
//
// k_ls_down_gx, the forward's mirror, a gather: a workgroup takes one image, a band of 8 input rows, a tile of 4 ns input columns and gb groups and
// stages the (6, 2 ns + 2) gy pixels under the tile in LDS (zeros outside the plane).  One thread owns one group and a strip of 4 input columns.  An
// input row takes the taps ky of its own parity only, so the thread runs the even rows of the band against ky = 0, 2, 4 and then the odd rows against
// ky = 1, 3, each time with 4 x 4 x ci sums and one ky's 5 ci co weights in registers.  Every gx element is one thread's fmaf chain in the order
// (ky, kx, u), rounded once at the store; the tiling is a function of (H, W, Cin, Cout, groups, dtype) alone.
//
// k_ls_down_gw + k_ls_down_gw_reduce, two stages through the caller's workspace: the units (image, band of output rows, tile of output columns) of a
// channel block are cut into P contiguous chunks, one workgroup each.  Per unit the workgroup stages the x pixels and the gy pixels in LDS; a
// thread owns (group, ky), walks the unit's output pixels row by row with a sliding window of 5 ci inputs and keeps its 5 ci co sums (and co sums
// of gy for the bias) in registers across the units of its chunk: no cross-lane reduction.  It leaves one partial (25 ci + 1, Cout) a chunk; the second
// kernel sums the P partials in index order.  P is a function of the call's arguments, so repeat launches give the same bits.
#include "rcx_common.h"
#include "rcx_launch.h"
#include "rcx_lsdown.h"

namespace rcx {
namespace {

constexpr size_t kLdsBudget = 64 * 1024;

// ---- input gradient ----
constexpr int kGxRows = 8;                 // input rows a workgroup takes (4 of each parity)
constexpr int kGxStrip = 4;                // input columns a thread takes (2 of each parity)
constexpr int kGxTileRows = kGxRows / 2 + 2;   // gy rows under a band

struct GxPlan {
    int gb, ns;                            // groups and column strips a workgroup takes: gb ns threads
    int cols;                              // gy columns in LDS: 2 ns + 2
    int bands, tiles, cblocks;
    size_t lds;
};

struct GxArgs {
    const float* w;
    int N, H, W, Ho, Wo, Cin, Cout, G;
    int gb, ns, cols, bands, tiles;
    int vb;                                // bytes of one staging access: 2, 4, 8 or 16
    int pairs;                             // 16-bit outputs leave as 32-bit pairs (ci even, gx aligned to 4 bytes)
};

bool make_gx_plan(int H, int W, int Cin, int Cout, int G, int dtype, GxPlan& p)
{
    const int co = Cout / G;
    const size_t es = dtype == 0 ? 4 : 2;
    p.gb = G > 32 ? 64 : 32;
    p.ns = W >= 4 * kGxStrip ? 4 : (W + kGxStrip - 1) / kGxStrip;
    p.cols = 2 * p.ns + 2;
    p.lds = (size_t)kGxTileRows * p.cols * p.gb * co * es;       // at most 6 x 10 x 64 x 4 x 4 = 61440 bytes
    if (p.lds > kLdsBudget) return false;
    p.bands = (H + kGxRows - 1) / kGxRows;
    p.tiles = (W + kGxStrip * p.ns - 1) / (kGxStrip * p.ns);
    p.cblocks = (G + p.gb - 1) / p.gb;
    return true;
}

template <typename T, int CI, int CO>
__global__ void __launch_bounds__(256) k_ls_down_gx(const T* __restrict__ gy, T* __restrict__ gx, GxArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nthreads = a.gb * a.ns;
    const int cb = blockIdx.y;
    int b = blockIdx.x;
    const int tx = b % a.tiles; b /= a.tiles;
    const int by = b % a.bands;
    const int n = b / a.bands;
    const int iy0 = by * kGxRows, ix0 = tx * kGxStrip * a.ns;
    const int groups_here = min(a.gb, a.G - cb * a.gb);
    const int chans = a.gb * CO;                         // LDS pixel pitch in elements

    {
        const unsigned char* src = reinterpret_cast<const unsigned char*>(gy + (size_t)n * a.Ho * a.Wo * a.Cout + (size_t)cb * a.gb * CO);
        const int run = groups_here * CO * (int)sizeof(T);
        const size_t pix = (size_t)a.Cout * sizeof(T);
        const int lp = chans * (int)sizeof(T);
        const int oy0 = iy0 / 2 - 1, ox0 = ix0 / 2 - 1;
        switch (a.vb) {
            case 16: stage<uint4>(smem, src, kGxTileRows, a.cols, run, lp, pix, oy0, ox0, a.Ho, a.Wo, nthreads); break;
            case 8: stage<uint2>(smem, src, kGxTileRows, a.cols, run, lp, pix, oy0, ox0, a.Ho, a.Wo, nthreads); break;
            case 4: stage<uint32_t>(smem, src, kGxTileRows, a.cols, run, lp, pix, oy0, ox0, a.Ho, a.Wo, nthreads); break;
            default: stage<uint16_t>(smem, src, kGxTileRows, a.cols, run, lp, pix, oy0, ox0, a.Ho, a.Wo, nthreads); break;
        }
    }
    __syncthreads();

    const int gl = threadIdx.x % a.gb, strip = threadIdx.x / a.gb;
    const int ix_s = ix0 + strip * kGxStrip;
    if (gl >= groups_here || ix_s >= a.W) return;
    const int g = cb * a.gb + gl;
    const T* tile = reinterpret_cast<const T*>(smem) + (size_t)(2 * strip) * chans + gl * CO;

#pragma unroll 1
    for (int par = 0; par < 2; ++par) {                  // the rows iy0 + 2 q + par take the taps ky = par, par + 2, ...
        float acc[4][kGxStrip][CI];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < kGxStrip; ++c)
#pragma unroll
                for (int j = 0; j < CI; ++j) acc[q][c][j] = 0.f;

#pragma unroll 1
        for (int ky = par; ky < 5; ky += 2) {
            float wt[5][CI][CO];
#pragma unroll
            for (int kx = 0; kx < 5; ++kx)
#pragma unroll
                for (int j = 0; j < CI; ++j)
#pragma unroll
                    for (int u = 0; u < CO; ++u) wt[kx][j][u] = a.w[(size_t)((ky * 5 + kx) * CI + j) * a.Cout + g * CO + u];
            const int row0 = 2 + (par - ky) / 2;         // gy row of q = 0 in the tile: (2 q + par + 2 - ky) / 2 + 1, par - ky even
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const T* row = tile + (size_t)(row0 + q) * a.cols * chans;
                float in[4][CO];
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int u = 0; u < CO; ++u) in[c][u] = elem_to_f32(row[c * chans + u]);
#pragma unroll
                for (int c = 0; c < kGxStrip; ++c)
#pragma unroll
                    for (int kx = c & 1; kx < 5; kx += 2)          // gy column (c + 2 - kx) / 2 + 1 of the strip's four
#pragma unroll
                        for (int j = 0; j < CI; ++j)
#pragma unroll
                            for (int u = 0; u < CO; ++u) acc[q][c][j] = fmaf(wt[kx][j][u], in[(c + 2 - kx) / 2 + 1][u], acc[q][c][j]);
            }
        }

#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int iy = iy0 + 2 * q + par;
            if (iy >= a.H) break;
#pragma unroll
            for (int c = 0; c < kGxStrip; ++c) {
                if (ix_s + c >= a.W) break;
                T* out = gx + (((size_t)n * a.H + iy) * a.W + ix_s + c) * a.Cin + g * CI;
                if constexpr (sizeof(T) == 2 && CI % 2 == 0) {
                    if (a.pairs) {
#pragma unroll
                        for (int j = 0; j < CI; j += 2) {
                            const float two[2] = {acc[q][c][j], acc[q][c][j + 1]};
                            store_vec<2>(out + j, two);
                        }
                        continue;
                    }
                }
#pragma unroll
                for (int j = 0; j < CI; ++j) out[j] = from_f32<T>(acc[q][c][j]);
            }
        }
    }
}

// ---- weight and bias gradient ----
struct GwPlan {
    int gb;                                // groups a workgroup takes: 5 gb threads, one per (group, ky)
    int rows, tw;                          // output rows and columns of a unit
    int bands, tiles, cblocks;
    long long units;                       // N bands tiles
    int P;                                 // chunks of units = partials
    size_t lds_x, lds;                     // bytes of the x tile (the gy tile follows it), both
};

struct GwArgs {
    float* part;
    int N, H, W, Ho, Wo, Cin, Cout, G;
    int gb, rows, tw, bands, tiles, P;
    long long units;
    int lds_x;
    int vbx, vbg;                          // bytes of one staging access of x and of gy
};

constexpr int kGwTargetWgs = 512;          // two workgroups for each of the 256 CUs where the batch has the units

bool make_gw_plan(int N, int H, int W, int Cin, int Cout, int G, int dtype, GwPlan& p)
{
    const int ci = Cin / G, co = Cout / G;
    const size_t es = dtype == 0 ? 4 : 2;
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    p.gb = G > 32 ? 64 : 32;
    p.rows = Ho < 4 ? Ho : 4;
    p.tw = Wo < 16 ? Wo : 16;
    auto xbytes = [&]() { return ((size_t)(2 * p.rows + 3) * (2 * p.tw + 3) * p.gb * ci * es + 15) & ~(size_t)15; };
    auto bytes = [&]() { return xbytes() + (size_t)p.rows * p.tw * p.gb * co * es; };
    while (bytes() > kLdsBudget) {
        if (p.gb == 64) p.gb = 32;
        else if (p.tw > 4) --p.tw;
        else if (p.rows > 1) --p.rows;
        else return false;
    }
    p.lds_x = xbytes();
    p.lds = bytes();
    p.bands = (Ho + p.rows - 1) / p.rows;
    p.tiles = (Wo + p.tw - 1) / p.tw;
    p.cblocks = (G + p.gb - 1) / p.gb;
    p.units = (long long)N * p.bands * p.tiles;
    const long long want = (kGwTargetWgs + p.cblocks - 1) / p.cblocks;
    p.P = (int)(p.units < want ? p.units : want);
    return true;
}

template <typename T, int CI, int CO>
__global__ void __launch_bounds__(320) k_ls_down_gw(const T* __restrict__ x, const T* __restrict__ gy, GwArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nthreads = 5 * a.gb;
    const int cb = blockIdx.y, chunk = blockIdx.x;
    const int groups_here = min(a.gb, a.G - cb * a.gb);
    const int chx = a.gb * CI, chg = a.gb * CO;          // LDS pixel pitches in elements
    const int gl = threadIdx.x % a.gb, ky = threadIdx.x / a.gb;
    const bool live = gl < groups_here;
    const T* xt = reinterpret_cast<const T*>(smem) + gl * CI;
    const T* gt = reinterpret_cast<const T*>(smem + a.lds_x) + gl * CO;

    float acc[5][CI][CO], bsum[CO];
#pragma unroll
    for (int u = 0; u < CO; ++u) {
        bsum[u] = 0.f;
#pragma unroll
        for (int kx = 0; kx < 5; ++kx)
#pragma unroll
            for (int j = 0; j < CI; ++j) acc[kx][j][u] = 0.f;
    }

    const long long u0 = a.units * chunk / a.P, u1 = a.units * (chunk + 1) / a.P;
#pragma unroll 1
    for (long long unit = u0; unit < u1; ++unit) {
        long long b = unit;
        const int tx = (int)(b % a.tiles); b /= a.tiles;
        const int by = (int)(b % a.bands);
        const int n = (int)(b / a.bands);
        const int oy0 = by * a.rows, ox0 = tx * a.tw;
        const int rows_here = min(a.rows, a.Ho - oy0), cols_here = min(a.tw, a.Wo - ox0);
        const int xcols = 2 * cols_here + 3;
        __syncthreads();                                 // the previous unit's tiles have been read
        {
            const unsigned char* src = reinterpret_cast<const unsigned char*>(x + (size_t)n * a.H * a.W * a.Cin + (size_t)cb * a.gb * CI);
            const int run = groups_here * CI * (int)sizeof(T), lp = chx * (int)sizeof(T);
            const size_t pix = (size_t)a.Cin * sizeof(T);
            const int rows = 2 * rows_here + 3, iy0 = 2 * oy0 - 2, ix0 = 2 * ox0 - 2;
            switch (a.vbx) {
                case 16: stage<uint4>(smem, src, rows, xcols, run, lp, pix, iy0, ix0, a.H, a.W, nthreads); break;
                case 8: stage<uint2>(smem, src, rows, xcols, run, lp, pix, iy0, ix0, a.H, a.W, nthreads); break;
                case 4: stage<uint32_t>(smem, src, rows, xcols, run, lp, pix, iy0, ix0, a.H, a.W, nthreads); break;
                default: stage<uint16_t>(smem, src, rows, xcols, run, lp, pix, iy0, ix0, a.H, a.W, nthreads); break;
            }
        }
        {
            const unsigned char* src = reinterpret_cast<const unsigned char*>(gy + (size_t)n * a.Ho * a.Wo * a.Cout + (size_t)cb * a.gb * CO);
            const int run = groups_here * CO * (int)sizeof(T), lp = chg * (int)sizeof(T);
            const size_t pix = (size_t)a.Cout * sizeof(T);
            unsigned char* dst = smem + a.lds_x;
            switch (a.vbg) {
                case 16: stage<uint4>(dst, src, rows_here, cols_here, run, lp, pix, oy0, ox0, a.Ho, a.Wo, nthreads); break;
                case 8: stage<uint2>(dst, src, rows_here, cols_here, run, lp, pix, oy0, ox0, a.Ho, a.Wo, nthreads); break;
                case 4: stage<uint32_t>(dst, src, rows_here, cols_here, run, lp, pix, oy0, ox0, a.Ho, a.Wo, nthreads); break;
                default: stage<uint16_t>(dst, src, rows_here, cols_here, run, lp, pix, oy0, ox0, a.Ho, a.Wo, nthreads); break;
            }
        }
        __syncthreads();
        if (!live) continue;
#pragma unroll 1
        for (int r = 0; r < rows_here; ++r) {
            const T* xr = xt + (size_t)(2 * r + ky) * xcols * chx;
            const T* gr = gt + (size_t)r * cols_here * chg;
            float win[5][CI];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int j = 0; j < CI; ++j) win[kx][j] = elem_to_f32(xr[kx * chx + j]);
#pragma unroll 1
            for (int c = 0; c < cols_here; ++c) {
#pragma unroll
                for (int kx = 3; kx < 5; ++kx)
#pragma unroll
                    for (int j = 0; j < CI; ++j) win[kx][j] = elem_to_f32(xr[(2 * c + kx) * chx + j]);
                float gv[CO];
#pragma unroll
                for (int u = 0; u < CO; ++u) {
                    gv[u] = elem_to_f32(gr[c * chg + u]);
                    bsum[u] += gv[u];
                }
#pragma unroll
                for (int kx = 0; kx < 5; ++kx)
#pragma unroll
                    for (int j = 0; j < CI; ++j)
#pragma unroll
                        for (int u = 0; u < CO; ++u) acc[kx][j][u] = fmaf(gv[u], win[kx][j], acc[kx][j][u]);
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int j = 0; j < CI; ++j) win[kx][j] = win[kx + 2][j];
            }
        }
    }

    if (!live) return;
    const int g = cb * a.gb + gl;
    float* part = a.part + (size_t)chunk * (25 * CI + 1) * a.Cout + g * CO;
#pragma unroll
    for (int kx = 0; kx < 5; ++kx)
#pragma unroll
        for (int j = 0; j < CI; ++j)
#pragma unroll
            for (int u = 0; u < CO; ++u) part[(size_t)((ky * 5 + kx) * CI + j) * a.Cout + u] = acc[kx][j][u];
    if (ky == 0) {
#pragma unroll
        for (int u = 0; u < CO; ++u) part[(size_t)(25 * CI) * a.Cout + u] = bsum[u];
    }
}

// gw[e] / gb[e - nw] = the sum over the P partials, in index order; nw = 25 ci Cout, a partial has nw + Cout elements
__global__ void __launch_bounds__(256) k_ls_down_gw_reduce(const float* __restrict__ part, float* __restrict__ gw, float* __restrict__ gb, int P, int nw, int cout)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int ne = nw + cout;
    if (e >= ne) return;
    if (e < nw ? gw == nullptr : gb == nullptr) return;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += part[(size_t)p * ne + e];
    if (e < nw) gw[e] = s;
    else gb[e - nw] = s;
}

template <typename T, int CI, int CO>
hipError_t launch(const void* x, const void* gy, void* gx, bool want_gw, const GxArgs& ax, const GxPlan& px, const GwArgs& aw, const GwPlan& pw, hipStream_t s)
{
    if (gx) {
        hipLaunchKernelGGL((k_ls_down_gx<T, CI, CO>), dim3((unsigned)((size_t)ax.N * px.bands * px.tiles), (unsigned)px.cblocks), dim3(px.gb * px.ns), px.lds, s,
                           (const T*)gy, (T*)gx, ax);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (want_gw) {
        hipLaunchKernelGGL((k_ls_down_gw<T, CI, CO>), dim3((unsigned)pw.P, (unsigned)pw.cblocks), dim3(5 * pw.gb), pw.lds, s, (const T*)x, (const T*)gy, aw);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename T, int CI, typename... A>
hipError_t launch_co(int co, A... args)
{
    switch (co) {
        case 1: return launch<T, CI, 1>(args...);
        case 2: return launch<T, CI, 2>(args...);
        case 3: return launch<T, CI, 3>(args...);
        case 4: return launch<T, CI, 4>(args...);
        default: return hipErrorInvalidValue;
    }
}

template <typename T, typename... A>
hipError_t launch_ci(int ci, int co, A... args)
{
    switch (ci) {
        case 1: return launch_co<T, 1>(co, args...);
        case 2: return launch_co<T, 2>(co, args...);
        case 3: return launch_co<T, 3>(co, args...);
        case 4: return launch_co<T, 4>(co, args...);
        default: return hipErrorInvalidValue;
    }
}

// the widest access that divides a pixel's pitch, a channel block's offset and run, and the tensor's own address
int stage_bytes(const void* p, int C, int block_chans, int es)
{
    int vb = 16;
    while (vb > es && (((size_t)C * es) % vb || ((size_t)block_chans * es) % vb || (size_t)p % vb)) vb >>= 1;
    return vb;
}

}  // namespace

bool ls_down_bwd_applicable(int N, int H, int W, int Cin, int Cout, int groups, int k, int stride, int dtype)
{
    if (!ls_down_applicable(N, H, W, Cin, Cout, groups, k, stride, dtype)) return false;
    GxPlan px;
    GwPlan pw;
    if (!make_gx_plan(H, W, Cin, Cout, groups, dtype, px) || !make_gw_plan(N, H, W, Cin, Cout, groups, dtype, pw)) return false;
    const size_t lim = (size_t)1 << 31;
    return (size_t)N * px.bands * px.tiles < lim && px.cblocks < 65536 && pw.cblocks < 65536 && pw.P >= 1;
}

size_t ls_down_bwd_workspace_bytes(int N, int H, int W, int Cin, int Cout, int groups, int k, int stride, int dtype)
{
    if (!ls_down_bwd_applicable(N, H, W, Cin, Cout, groups, k, stride, dtype)) return 0;
    GwPlan pw;
    make_gw_plan(N, H, W, Cin, Cout, groups, dtype, pw);
    return sizeof(float) * (size_t)pw.P * (25 * (Cin / groups) + 1) * Cout;
}

hipError_t ls_down_bwd(const void* x, const void* gy, const float* wpack, void* gx, float* gw, float* gb, void* workspace, int N, int H, int W, int Cin,
                       int Cout, int groups, int dtype, hipStream_t s)
{
    if (!ls_down_bwd_applicable(N, H, W, Cin, Cout, groups, 5, 2, dtype)) return hipErrorInvalidValue;
    const bool want_gw = gw || gb;
    if (want_gw && !workspace) return hipErrorInvalidValue;
    GxPlan px;
    GwPlan pw;
    make_gx_plan(H, W, Cin, Cout, groups, dtype, px);
    make_gw_plan(N, H, W, Cin, Cout, groups, dtype, pw);
    const int ci = Cin / groups, co = Cout / groups;
    const int es = dtype == 0 ? 4 : 2;
    GxArgs ax{};
    ax.w = wpack;
    ax.N = N; ax.H = H; ax.W = W; ax.Ho = (H + 1) / 2; ax.Wo = (W + 1) / 2; ax.Cin = Cin; ax.Cout = Cout; ax.G = groups;
    ax.gb = px.gb; ax.ns = px.ns; ax.cols = px.cols; ax.bands = px.bands; ax.tiles = px.tiles;
    ax.vb = stage_bytes(gy, Cout, px.gb * co, es);
    ax.pairs = es == 2 && ci % 2 == 0 && (size_t)gx % 4 == 0;
    GwArgs aw{};
    aw.part = (float*)workspace;
    aw.N = N; aw.H = H; aw.W = W; aw.Ho = ax.Ho; aw.Wo = ax.Wo; aw.Cin = Cin; aw.Cout = Cout; aw.G = groups;
    aw.gb = pw.gb; aw.rows = pw.rows; aw.tw = pw.tw; aw.bands = pw.bands; aw.tiles = pw.tiles; aw.P = pw.P; aw.units = pw.units;
    aw.lds_x = (int)pw.lds_x;
    aw.vbx = stage_bytes(x, Cin, pw.gb * ci, es);
    aw.vbg = stage_bytes(gy, Cout, pw.gb * co, es);
    hipError_t e;
    switch (dtype) {
        case 0: e = launch_ci<float>(ci, co, x, gy, gx, want_gw, ax, px, aw, pw, s); break;
        case 1: e = launch_ci<bf16_t>(ci, co, x, gy, gx, want_gw, ax, px, aw, pw, s); break;
        case 2: e = launch_ci<f16_t>(ci, co, x, gy, gx, want_gw, ax, px, aw, pw, s); break;
        default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess || !want_gw) return e;
    const int nw = 25 * ci * Cout, ne = nw + Cout;
    hipLaunchKernelGGL(k_ls_down_gw_reduce, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, (const float*)workspace, gw, gb, pw.P, nw, Cout);
    return hipGetLastError();
}

}  // namespace rcx

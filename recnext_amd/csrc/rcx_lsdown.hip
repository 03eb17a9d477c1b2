// Downsample.token_mixer of the LSNet-style RecNeXt-T / S / B and of their share-channel variants (lsnet/model/recattn.py:254-263,
// recattn_share_channel.py:223-232): the grouped 5x5 stride-2 conv with groups = gcd(Cin, Cout), eval-mode BatchNorm folded into the pack.
//     y[n, oy, ox, g co + u] = bias[g co + u] + sum_{ky, kx, j} wpack[((ky 5 + kx) ci + j) Cout + g co + u] * x[n, 2 oy + ky - 2, 2 ox + kx - 2, g ci + j]
// One launch, no workspace.  A workgroup takes one image, a band of kRows output rows, a tile of at most 4 ns output columns and gb groups.  It
// copies the (11, 8 ns + 3) input pixels under the tile, gb ci channels of each, from global memory into LDS in the widest aligned accesses the
// pointer and the channel counts allow (up to 16 bytes a lane, a pixel's channels being one contiguous run), zeros outside the image.  Then
// one thread owns one group and one strip of 4 output columns: it keeps the kRows x 4 x co sums in registers, walks the taps row by row with
// that row's 5 ci co weights in registers (read once a row from the pack, neighbouring lanes neighbouring addresses) and reads each input row of
// the strip from LDS once.  Every sum is one thread's fmaf chain in the order (ky, kx, j) from the bias, so the result is bitwise repeatable, and
// the tiling is a function of (H, W, Cin, Cout, groups, dtype) alone, so an image's result does not depend on the batch it came in.
#include "rcx_common.h"
#include "rcx_launch.h"
#include "rcx_lsdown.h"

namespace rcx {
namespace {

constexpr int kRows = 4;                   // output rows a workgroup (and a thread) takes
constexpr int kStrip = 4;                  // output columns a thread takes
constexpr int kTileRows = 2 * kRows + 3;   // input rows under a band
constexpr int kStripCols = 2 * kStrip + 3; // input columns under a strip
constexpr size_t kLdsBudget = 64 * 1024;

struct DownPlan {
    int gb, ns;                            // groups and column strips a workgroup takes: gb ns threads
    int cols;                              // input columns in LDS: 8 ns + 3
    int bands, tiles, cblocks;
    size_t lds;
};

struct DownArgs {
    const float *w, *bias;
    int N, H, W, Ho, Wo, Cin, Cout, G;
    int gb, ns, cols, bands, tiles;
    int vb;                                // bytes of one staging access: 2, 4, 8 or 16
    int pairs;                             // 16-bit outputs leave as 32-bit pairs (co even, y aligned to 4 bytes)
};

bool make_plan(int H, int W, int Cin, int Cout, int G, int dtype, DownPlan& p)
{
    const int ci = Cin / G;
    const size_t es = dtype == 0 ? 4 : 2;
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    p.gb = G > 32 ? 64 : 32;
    p.ns = Wo >= 4 * kStrip ? 4 : (Wo + kStrip - 1) / kStrip;
    auto bytes = [&]() { return (size_t)kTileRows * (2 * kStrip * p.ns + 3) * p.gb * ci * es; };
    while (bytes() > kLdsBudget) {
        if (p.gb == 64) p.gb = 32;
        else if (p.ns > 1) --p.ns;
        else return false;
    }
    p.cols = 2 * kStrip * p.ns + 3;
    p.lds = bytes();
    p.bands = (Ho + kRows - 1) / kRows;
    p.tiles = (Wo + kStrip * p.ns - 1) / (kStrip * p.ns);
    p.cblocks = (G + p.gb - 1) / p.gb;
    return true;
}

template <typename T, int CI, int CO>
__global__ void __launch_bounds__(256) k_ls_down(const T* __restrict__ x, T* __restrict__ y, DownArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nthreads = a.gb * a.ns;
    const int cb = blockIdx.y;
    int b = blockIdx.x;
    const int tx = b % a.tiles; b /= a.tiles;
    const int by = b % a.bands;
    const int n = b / a.bands;
    const int oy0 = by * kRows, ox0 = tx * kStrip * a.ns;
    const int rows_here = min(kRows, a.Ho - oy0);
    const int groups_here = min(a.gb, a.G - cb * a.gb);
    const int chans = a.gb * CI;                         // LDS pixel pitch in elements (the last channel block fills only a part)

    {
        const unsigned char* src = reinterpret_cast<const unsigned char*>(x + (size_t)n * a.H * a.W * a.Cin + (size_t)cb * a.gb * CI);
        const int run = groups_here * CI * (int)sizeof(T);
        const int rows = 2 * rows_here + 3;
        const size_t pix = (size_t)a.Cin * sizeof(T);
        const int lp = chans * (int)sizeof(T);
        const int iy0 = 2 * oy0 - 2, ix0 = 2 * ox0 - 2;
        switch (a.vb) {
            case 16: stage<uint4>(smem, src, rows, a.cols, run, lp, pix, iy0, ix0, a.H, a.W, nthreads); break;
            case 8: stage<uint2>(smem, src, rows, a.cols, run, lp, pix, iy0, ix0, a.H, a.W, nthreads); break;
            case 4: stage<uint32_t>(smem, src, rows, a.cols, run, lp, pix, iy0, ix0, a.H, a.W, nthreads); break;
            default: stage<uint16_t>(smem, src, rows, a.cols, run, lp, pix, iy0, ix0, a.H, a.W, nthreads); break;
        }
    }
    __syncthreads();

    const int gl = threadIdx.x % a.gb, strip = threadIdx.x / a.gb;
    const int ox_s = ox0 + strip * kStrip;
    if (gl >= groups_here || ox_s >= a.Wo) return;
    const int g = cb * a.gb + gl;
    const T* tile = reinterpret_cast<const T*>(smem) + (size_t)(2 * kStrip * strip) * chans + gl * CI;

    float acc[kRows][kStrip][CO];
#pragma unroll
    for (int u = 0; u < CO; ++u) {
        const float bv = a.bias ? a.bias[g * CO + u] : 0.f;
#pragma unroll
        for (int r = 0; r < kRows; ++r)
#pragma unroll
            for (int p = 0; p < kStrip; ++p) acc[r][p][u] = bv;
    }

#pragma unroll 1
    for (int ky = 0; ky < 5; ++ky) {
        float wt[5][CI][CO];
#pragma unroll
        for (int kx = 0; kx < 5; ++kx)
#pragma unroll
            for (int j = 0; j < CI; ++j)
#pragma unroll
                for (int u = 0; u < CO; ++u) wt[kx][j][u] = a.w[(size_t)((ky * 5 + kx) * CI + j) * a.Cout + g * CO + u];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            if (r < rows_here) {
                const T* row = tile + (size_t)(2 * r + ky) * a.cols * chans;
                float in[kStripCols][CI];
#pragma unroll
                for (int c = 0; c < kStripCols; ++c)
#pragma unroll
                    for (int j = 0; j < CI; ++j) in[c][j] = elem_to_f32(row[c * chans + j]);
#pragma unroll
                for (int p = 0; p < kStrip; ++p)
#pragma unroll
                    for (int kx = 0; kx < 5; ++kx)
#pragma unroll
                        for (int j = 0; j < CI; ++j)
#pragma unroll
                            for (int u = 0; u < CO; ++u) acc[r][p][u] = fmaf(wt[kx][j][u], in[2 * p + kx][j], acc[r][p][u]);
            }
        }
    }

#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        if (r >= rows_here) break;
#pragma unroll
        for (int p = 0; p < kStrip; ++p) {
            if (ox_s + p >= a.Wo) break;
            T* out = y + (((size_t)n * a.Ho + oy0 + r) * a.Wo + ox_s + p) * a.Cout + g * CO;
            if constexpr (sizeof(T) == 2 && CO % 2 == 0) {
                if (a.pairs) {
#pragma unroll
                    for (int u = 0; u < CO; u += 2) {
                        const float two[2] = {acc[r][p][u], acc[r][p][u + 1]};
                        store_vec<2>(out + u, two);
                    }
                    continue;
                }
            }
#pragma unroll
            for (int u = 0; u < CO; ++u) out[u] = from_f32<T>(acc[r][p][u]);
        }
    }
}

template <typename T, int CI, int CO>
hipError_t launch(const void* x, void* y, const DownArgs& a, const DownPlan& p, hipStream_t s)
{
    hipLaunchKernelGGL((k_ls_down<T, CI, CO>), dim3((unsigned)((size_t)a.N * p.bands * p.tiles), (unsigned)p.cblocks), dim3(p.gb * p.ns), p.lds, s,
                       (const T*)x, (T*)y, a);
    return hipGetLastError();
}

template <typename T, int CI>
hipError_t launch_co(int co, const void* x, void* y, const DownArgs& a, const DownPlan& p, hipStream_t s)
{
    switch (co) {
        case 1: return launch<T, CI, 1>(x, y, a, p, s);
        case 2: return launch<T, CI, 2>(x, y, a, p, s);
        case 3: return launch<T, CI, 3>(x, y, a, p, s);
        case 4: return launch<T, CI, 4>(x, y, a, p, s);
        default: return hipErrorInvalidValue;
    }
}

template <typename T>
hipError_t launch_ci(int ci, int co, const void* x, void* y, const DownArgs& a, const DownPlan& p, hipStream_t s)
{
    switch (ci) {
        case 1: return launch_co<T, 1>(co, x, y, a, p, s);
        case 2: return launch_co<T, 2>(co, x, y, a, p, s);
        case 3: return launch_co<T, 3>(co, x, y, a, p, s);
        case 4: return launch_co<T, 4>(co, x, y, a, p, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

bool ls_down_applicable(int N, int H, int W, int Cin, int Cout, int groups, int k, int stride, int dtype)
{
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || groups <= 0 || k != 5 || stride != 2 || dtype < 0 || dtype > 2) return false;
    if (Cin % groups || Cout % groups) return false;
    const int ci = Cin / groups, co = Cout / groups;
    if (ci > 4 || co > 4) return false;
    DownPlan p;
    if (!make_plan(H, W, Cin, Cout, groups, dtype, p)) return false;
    const size_t lim = (size_t)1 << 31;
    return (size_t)N * H * W * Cin < lim && (size_t)N * ((H + 1) / 2) * ((W + 1) / 2) * Cout < lim && (size_t)N * p.bands * p.tiles < lim && p.cblocks < 65536;
}

hipError_t ls_down_fwd(const void* x, void* y, const float* wpack, const float* bias, int N, int H, int W, int Cin, int Cout, int groups, int dtype,
                       hipStream_t s)
{
    if (!ls_down_applicable(N, H, W, Cin, Cout, groups, 5, 2, dtype)) return hipErrorInvalidValue;
    DownPlan p;
    make_plan(H, W, Cin, Cout, groups, dtype, p);
    const int ci = Cin / groups, co = Cout / groups;
    const int es = dtype == 0 ? 4 : 2;
    DownArgs a{};
    a.w = wpack; a.bias = bias;
    a.N = N; a.H = H; a.W = W; a.Ho = (H + 1) / 2; a.Wo = (W + 1) / 2; a.Cin = Cin; a.Cout = Cout; a.G = groups;
    a.gb = p.gb; a.ns = p.ns; a.cols = p.cols; a.bands = p.bands; a.tiles = p.tiles;
    // the widest access that divides a pixel's pitch, a channel block's offset and run, and x's own address
    a.vb = 16;
    while (a.vb > es && (((size_t)Cin * es) % a.vb || ((size_t)p.gb * ci * es) % a.vb || (size_t)x % a.vb)) a.vb >>= 1;
    a.pairs = es == 2 && co % 2 == 0 && (size_t)y % 4 == 0;
    switch (dtype) {
        case 0: return launch_ci<float>(ci, co, x, y, a, p, s);
        case 1: return launch_ci<bf16_t>(ci, co, x, y, a, p, s);
        case 2: return launch_ci<f16_t>(ci, co, x, y, a, p, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rcx

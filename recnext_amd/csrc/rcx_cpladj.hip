// Channel-per-lane INPUT adjoint of the RecConv2d block (model/recnext.py:24-34) for the 14x14 / level 2 and 7x7 / level 1 blocks: dL/dx
// alone, for a block whose parameters want no gradient (frozen, or folded for inference).  The block is linear in x, so gx = A^T gy needs
// the taps and gy only -- no x, no saved pyramid, no weight-gradient partial rows (so no batch limit).  One lane owns one (image, channel)
// plane, as in rcx_cplbwd.hip, and the pieces are the same (rcx_cplbwd_pieces.h); the weight-gradient half of that kernel is simply absent.
//
//   level 1:  gT = conv_b^T(gY);  gC = R^T(gT);  gF = conv_a^T(gC);  gX = gT + down^T(gF)
//   level 2:  gT0 = conv_2^T(gY);  gC1 = R^T(gT0);  G1 = the level-1 adjoint of gC1 (conv_1, conv_0);  gX = gT0 + down^T(G1)
// float32 throughout, one rounding at the gx store, a fixed order of operations: deterministic.  gy: float32 or the block's 16-bit type;
// gx: the block's type, or float32 when the launch is the 14x14 tail of a larger block (gy = dL/dC_m, gx = G_m of rcx_api.hip).
#include "rcx_cplbwd_pieces.h"
#include "rcx_opts.h"

namespace rcx {
namespace cpladj {

using namespace cplbwd;

struct AdjArgs {
    const void* gy;                // N x W x W x C of TG
    const float* wpack;            // (level+2, 25, C): the down conv's taps
    const float* wflip;            // the same pack with every 5x5 flipped: conv^T = conv with these
    void* gx;                      // N x W x W x C of TO
    int N, C;
};

// out = gT + down^T(conv_a^T(R^T(gT))), gT = conv_b^T(G): the level-1 block's input adjoint on resident planes (conv_b = pack 2, conv_a =
// pack 1, down = pack 0 -- the whole 7x7 block, or the inner block of the 14x14 one).  Every tap set is requested up front.
template <int MODE, int CT, int NW, int NC>
__device__ __forceinline__ void level1_adj(const f32x2 (&G)[NW][(NW + 1) / 2], f32x2 (&out)[NW][(NW + 1) / 2], const float* wpack,
                                           const float* wflip, int C, unsigned vow)
{
    constexpr int PW = (NW + 1) / 2, PC = (NC + 1) / 2;
    Taps tfb, tfa, td;
    load_taps<CT>(tfb, wflip, nullptr, 2, C, vow, 0);
    load_taps<CT>(tfa, wflip, nullptr, 1, C, vow, 0);
    load_taps<CT>(td, wpack, nullptr, 0, C, vow, 0);
    conv5_plane<NW>(G, out, tfb);                           // gT = conv_b^T(G)
    f32x2 gF[NC][PC];
    {
        f32x2 gC[NC][PC];
#pragma unroll
        for (int i = 0; i < NC; ++i)
#pragma unroll
            for (int j = 0; j < PC; ++j) gC[i][j] = f32x2{0.f, 0.f};
#pragma unroll
        for (int d = 0; d < NW; ++d) resizeT_row<MODE, NC, NW>(out[d], d, gC);
        pin(gC);
        RCX_FENCE;
        conv5_plane<NC>(gC, gF, tfa);                       // gF = conv_a^T(gC)
    }
#pragma unroll
    for (int r = 0; r < NW; ++r) {
        downT_row<NW, NC>(gF, r, td, out[r]);               // gX = gT + down^T(gF)
        if (NW & 1) out[r][PW - 1].y = 0.f;
        pin(out[r]);
        RCX_FENCE;
    }
}

// the workgroup's image (uniform: the row bases stay scalar) and the lane's channel.  XCD-aware order (rcx_cpl14.hip).
__device__ __forceinline__ int plane_of(int C, int& c)
{
    const int nb = (C + 63) / 64;
    unsigned b = blockIdx.x;
    const unsigned G = gridDim.x;
    if ((G & 7u) == 0) b = (b & 7u) * (G >> 3) + (b >> 3);
    const int n = (int)(b / (unsigned)nb), cb = (int)(b - (unsigned)n * (unsigned)nb);
    c = cb * 64 + (int)threadIdx.x;
    return n;
}

// ---- 7x7 / level 1: gy in, the whole adjoint on resident planes, gx out
template <int MODE, int CT, typename TG, typename TO>
__global__ __launch_bounds__(64)
void k_recconv_adj_cpl7(AdjArgs A)
{
    constexpr int W = 7, P = 4, W1 = 4;
    const int C = CT > 0 ? CT : A.C;
    int c;
    const int n = plane_of(C, c);
    if (n >= A.N || c >= C) return;
    const gcptr gyb = (gcptr)A.gy + (size_t)n * W * W * (size_t)C * sizeof(TG);
    const gcptr gxb = (gcptr)A.gx + (size_t)n * W * W * (size_t)C * sizeof(TO);
    const RowAddr<W, CT, TG> rg((unsigned)c * (unsigned)sizeof(TG), (size_t)C * sizeof(TG));
    const RowAddr<W, CT, TO> ro((unsigned)c * (unsigned)sizeof(TO), (size_t)C * sizeof(TO));
    uint32_t rawg[W][W];
    sfor<W>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        rg.row(gyb, r, [&](auto qc, gcptr base, unsigned voff, auto immc) {
            rawg[r][decltype(qc)::value] = SafeLd<TG>::ld(base + decltype(immc)::value + voff);
        });
    });
    RCX_FENCE;
    f32x2 GY[W][P], X[W][P];
#pragma unroll
    for (int r = 0; r < W; ++r) {
        pin_raw(rawg[r]);
#pragma unroll
        for (int j = 0; j < P; ++j) GY[r][j] = f32x2{SafeLd<TG>::cvt(rawg[r][2 * j]), 2 * j + 1 < W ? SafeLd<TG>::cvt(rawg[r][2 * j + 1]) : 0.f};
    }
    RCX_FENCE;
    level1_adj<MODE, CT, W, W1>(GY, X, A.wpack, A.wflip, C, (unsigned)c * 4u);
    sfor<W>([&](auto rc) {
        constexpr int o = decltype(rc)::value;
        typename PixSt<TO>::packed pk[P];
#pragma unroll
        for (int j = 0; j < P; ++j) pk[j] = PixSt<TO>::prep(X[o][j]);
        ro.row(gxb, o, [&](auto qc, gcptr base, unsigned voff, auto immc) {
            constexpr int q = decltype(qc)::value;
            PixSt<TO>::st(base + decltype(immc)::value + voff, pk[q >> 1], q & 1);
        });
    });
}

// ---- 14x14 / level 2.  Three sweeps.  (1) gT0 = conv_2^T(gy): gy rows stream in, input-row stationary; a finished row is parked in the
// accumulator half of the register file (196 values) and folded into gC1 = R^T(gT0).  (2) the level-1 adjoint on the resident 7x7 plane:
// gC1 -> G1.  (3) gx = gT0 + down^T(G1) leaves row by row.  No x, so nothing is streamed a second time; one wave per plane (no split: the
// training kernel's split hands its independent weight-gradient sweep to a second wave, and this kernel has no independent sweep).
template <int MODE, int CT, typename TG, typename TO>
__global__ __launch_bounds__(64)
void k_recconv_adj_cpl14(AdjArgs A)
{
    constexpr int W = 14, P = 7, W1 = 7, P1 = 4, W2 = 4;
    const int C = CT > 0 ? CT : A.C;
    int c;
    const int n = plane_of(C, c);
    if (n >= A.N || c >= C) return;
    const unsigned vow = (unsigned)c * 4u;
    const gcptr gyb = (gcptr)A.gy + (size_t)n * W * W * (size_t)C * sizeof(TG);
    const gcptr gxb = (gcptr)A.gx + (size_t)n * W * W * (size_t)C * sizeof(TO);
    const RowAddr<W, CT, TG> rg((unsigned)c * (unsigned)sizeof(TG), (size_t)C * sizeof(TG));
    const RowAddr<W, CT, TO> ro((unsigned)c * (unsigned)sizeof(TO), (size_t)C * sizeof(TO));
    uint32_t rgy[W][W];                                     // rows as loaded; only the rows in flight are live
    auto ld_g = [&](auto rc) {
        constexpr int r = decltype(rc)::value;
        rg.row(gyb, r, [&](auto qc, gcptr base, unsigned voff, auto immc) {
            rgy[r][decltype(qc)::value] = SafeLd<TG>::ld(base + decltype(immc)::value + voff);
        });
    };

    // ---- (1) gT0 = conv_2^T(gy) -> the stash, and gC1 = R^T(gT0)
    float S[W][W];
    f32x2 gC1[W1][P1];
#pragma unroll
    for (int i = 0; i < W1; ++i)
#pragma unroll
        for (int j = 0; j < P1; ++j) gC1[i][j] = f32x2{0.f, 0.f};
    {
        constexpr int AHEAD = 3;
        sfor<AHEAD>([&](auto rc) { ld_g(rc); });
        Taps tf;
        load_taps<CT>(tf, A.wflip, nullptr, 3, C, vow, 0);
        f32x2 acc[5][P];
        sfor<W>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
#pragma unroll
            for (int s_ = 0; s_ < 5; ++s_) {
                const bool enters = (t == 0) ? (s_ <= 2) : (s_ == (t + 2) % 5 && t + 2 < W);
                if (enters) {
#pragma unroll
                    for (int j = 0; j < P; ++j) acc[s_][j] = f32x2{0.f, 0.f};
                }
            }
            if constexpr (t + AHEAD < W) ld_g(IC<t + AHEAD>{});
            pin_raw(rgy[t]);
            f32x2 row[P];
#pragma unroll
            for (int j = 0; j < P; ++j) row[j] = f32x2{SafeLd<TG>::cvt(rgy[t][2 * j]), SafeLd<TG>::cvt(rgy[t][2 * j + 1])};
            conv5_row<W>(row, t, tf, [&](int o) -> f32x2(&)[P] { return acc[o % 5]; });
#pragma unroll
            for (int d = 2; d >= 0; --d) {                  // output row t - 2 is complete (all three at the last row)
                const int o = t - d;
                if (o < 0 || (d < 2 && t != W - 1)) continue;
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    S[o][2 * j] = stash(acc[o % 5][j].x);
                    S[o][2 * j + 1] = stash(acc[o % 5][j].y);
                }
                resizeT_row<MODE, W1, W>(acc[o % 5], o, gC1);
            }
#pragma unroll
            for (int o = 0; o < W; ++o) if (o > t - 2 && o <= t + 2 && t != W - 1) pin(acc[o % 5]);
            pin(gC1);
            RCX_FENCE;
        });
    }

    // ---- (2) the level-1 block's adjoint on the 7x7 plane: gC1 -> G1
    f32x2 G1[W1][P1];
    level1_adj<MODE, CT, W1, W2>(gC1, G1, A.wpack, A.wflip, C, vow);

    // ---- (3) gx = gT0 + down^T(G1)
    Taps td;
    load_taps<CT>(td, A.wpack, nullptr, 0, C, vow, 0);
    sfor<W>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        f32x2 out[P];
#pragma unroll
        for (int j = 0; j < P; ++j) out[j] = f32x2{unstash(S[r][2 * j]), unstash(S[r][2 * j + 1])};
        downT_row<W, W1>(G1, r, td, out);
        typename PixSt<TO>::packed pk[P];
#pragma unroll
        for (int j = 0; j < P; ++j) pk[j] = PixSt<TO>::prep(out[j]);
        ro.row(gxb, r, [&](auto qc, gcptr base, unsigned voff, auto immc) {
            constexpr int q = decltype(qc)::value;
            PixSt<TO>::st(base + decltype(immc)::value + voff, pk[q >> 1], q & 1);
        });
        RCX_FENCE;
    });
}

// the 14x14 (H = 14) or the 7x7 block's input adjoint; a compile-time channel pitch for RecNeXt's stage (256 / 512 channels), else a run-time one
template <int H, int MODE, int CT, typename TG, typename TO>
static hipError_t launch(const AdjArgs& A, hipStream_t s)
{
    const unsigned planes = (unsigned)(A.N * ((A.C + 63) / 64));
    if constexpr (H == 14) hipLaunchKernelGGL((k_recconv_adj_cpl14<MODE, CT, TG, TO>), dim3(planes), dim3(64), 0, s, A);
    else hipLaunchKernelGGL((k_recconv_adj_cpl7<MODE, CT, TG, TO>), dim3(planes), dim3(64), 0, s, A);
    return hipGetLastError();
}
template <int H, int MODE, typename TG, typename TO>
static hipError_t launch_c(const AdjArgs& A, hipStream_t s)
{
    constexpr int CT = H == 14 ? 256 : 512;
    return A.C == CT ? launch<H, MODE, CT, TG, TO>(A, s) : launch<H, MODE, 0, TG, TO>(A, s);
}
template <int H, int MODE>
static hipError_t launch_dt(const AdjArgs& A, int gy_dt, int gx_dt, hipStream_t s)
{
    if (gy_dt == 0 && gx_dt == 0) return launch_c<H, MODE, float, float>(A, s);
    if (gy_dt == 0 && gx_dt == 1) return launch_c<H, MODE, float, bf16_t>(A, s);
    if (gy_dt == 0 && gx_dt == 2) return launch_c<H, MODE, float, f16_t>(A, s);
    if (gy_dt == 1 && gx_dt == 1) return launch_c<H, MODE, bf16_t, bf16_t>(A, s);
    if (gy_dt == 2 && gx_dt == 2) return launch_c<H, MODE, f16_t, f16_t>(A, s);
    return hipErrorInvalidValue;
}

}  // namespace cpladj

// the input adjoint applies where the fused training forward does; it keeps no partial rows, so the batch is bounded by the grid alone
bool cpladj_applicable(int N, int C, int H, int W, int level, int k, int dtype)
{
    if (rcx::opt::off(rcx::opt::BWD_FUSED) || rcx::opt::hand_kernels_off() || (long long)N * ((C + 63) / 64) >= (1LL << 31)) return false;
    return cpl7b_applicable(N, C, H, W, level, k, dtype) || cpl14_applicable(N, C, H, W, level, k, dtype);
}

hipError_t cpladj_recconv(const void* gy, int gy_dt, const float* wpack, const float* wflip, void* gx, int gx_dt, int N, int C, int H, int mode,
                          hipStream_t s)
{
    cpladj::AdjArgs A{};
    A.gy = gy; A.wpack = wpack; A.wflip = wflip; A.gx = gx; A.N = N; A.C = C;
    if (H == 14) return mode == 1 ? cpladj::launch_dt<14, 1>(A, gy_dt, gx_dt, s) : cpladj::launch_dt<14, 0>(A, gy_dt, gx_dt, s);
    return mode == 1 ? cpladj::launch_dt<7, 1>(A, gy_dt, gx_dt, s) : cpladj::launch_dt<7, 0>(A, gy_dt, gx_dt, s);
}

}  // namespace rcx

// RecNextStem in ONE launch (bf16 inference): y = conv3x3_s2(gelu(conv3x3_s2(x) + b1)) + b2, both convs BN-folded (model/recnext.py:134-146 `RecNextStem`,
// :75-97 ConvNorm.fuse).  As library calls the stem is two convs, two bias adds and a GELU (0.39 ms of RecNeXt-M3's 2.9 ms step): the intermediate
// 112 x 112 x C/2 tensor -- twice the size of the stem's output -- is written once and read three times.  Here it exists only as a 17 x 17 tile in LDS:
//   a persistent workgroup (4 waves; two per compute unit at RecNeXt-M3's 32 / 64 channels) walks 8 x 8 tiles of output pixels, the weights in LDS once;
//   x. the tile's 35 rows of x (36 pixels x 3 channels = 216 bytes each, from image pixel 32 tx - 4) are requested a tile ahead into registers and written to LDS at
//      the top of the tile: as 27 aligned 8-byte pieces a row where the rows of the image allow it (W % 4 == 0, x 8-byte aligned: 4 loads a thread), else as single
//      bf16 (15 loads a thread) -- the same LDS image either way;
//   A. conv1 + bias + GELU for the 17 x 17 pixels of the intermediate the tile needs, ALSO on the matrix cores (K = 27 taps padded to 32; the im2col operand gathered
//      from the x tile in LDS: a pixel's inputs are three runs of nine contiguous bf16), rounded to bf16 into LDS (zeros outside the intermediate's plane:
//      the second conv's padding).  (A first version ran it on the vector pipe, a pixel per thread with the weights as scalar operands: 488 us, no faster than the library.)
//      A wave's pixel tiles are software-pipelined (round 23): the LDS reads of the next one go out before the GELU of this one, its products are issued between the
//      two halves of that GELU (each half four pairs in lockstep), the biases sit in registers, and the last two of the ten pixel tiles are shared by the waves of a
//      pair (both multiply, each takes every other channel group through the GELU): 2.5 epilogues a wave instead of 3 | 3 | 2 | 2.  Same operations, same bits.
//   B. conv2 as an implicit GEMM on the matrix cores: D (32 out channels x 32 pixels) = sum over (tap, 16-channel group) of W2 fragment x h1 fragment, the h1
//      fragment read straight from the LDS tile at the tap's offset (8 consecutive channels of one pixel = 16 bytes), the W2 fragments packed on the host
//      (ops.pack_stem); + b2 -> bf16 -> the wave's own 32 pixel x 32 channel image in LDS -> y, 16 bytes a lane with a pixel's 64 bytes contiguous across four lanes
//      (a pixel per lane straight to memory -- 8 bytes of each of 32 pixels a request -- cost this kernel 0.9 k of a tile's 15.7 k cycles per wave in the store itself
//      and another 1.1 k in the x requests queued behind it: profiles/r09_stem_timeline.txt).
// -DRCX_STEM_STAMPS is the diagnostic build of this file alone (tools/stem_timeline.py): s_memtime at the phase boundaries, summed per wave into a buffer of its own.
// Numerics: float32 accumulation, the intermediate rounded to bf16 once (as the library path does), exact GELU (rcx_gelu.h).
// The same kernel with a GELU after the second conv's bias as well (template flag GO; CM = 16 | 32) is the front launch of the T / S / B stem, whose third conv is
// rcx_conv3s2.hip (stem_front_fwd below; lsnet/model/recattn.py:208-223).
#include "rcx_common.h"
#include "rcx_launch.h"
#include "rcx_gelu.h"
#include <type_traits>


#ifdef RCX_STEM_STAMPS
#define RCX_STAMP(k)                                                                                            \
    {                                                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                      \
        unsigned long long t_;                                                                                  \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                              \
        __builtin_amdgcn_sched_barrier(0);                                                                      \
        tsum[k] += t_ - tlast;                                                                                  \
        tlast = t_;                                                                                             \
    }
#define RCX_STAMP_ARG , unsigned long long* __restrict__ stamps
#define RCX_STAMP_VAL , g_stamps
namespace rcx {
static unsigned long long* g_stamps = nullptr;
}
#else
#define RCX_STAMP(k)
#define RCX_STAMP_ARG
#define RCX_STAMP_VAL
#endif

namespace rcx {
namespace stem {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4q __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4q __attribute__((ext_vector_type(4)));
typedef unsigned u32x2q __attribute__((ext_vector_type(2)));
constexpr int YIMG = 32 * 64;              // bytes of a wave's output image in LDS

// what a wave wrote to its LDS image is read by its other lanes (and the other way round)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// CM = channels of the intermediate, KC = CM rounded up to a multiple of 16 (the k-steps of a tap), M1 = ceil(CM / 32) tiles of the first product, MT = output tiles,
// XW = x rows move as 8-byte pieces (W % 4 == 0 and an 8-byte aligned x: every piece lies wholly inside or outside a row of the image), else as single bf16,
// GO = an exact GELU after the second conv's bias as well (the front of the T / S / B stem, rcx_conv3s2.hip; the M / A stem has none)
// (two waves per SIMD wherever the LDS footprint lets two workgroups share a compute unit, KC <= 32: the registers must then fit 256)
template <int CM, int KC, int MT, bool XW, bool GO = false>
__global__ void __launch_bounds__(256, KC <= 32 ? 2 : 1)
k_stem(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, const u32x4q* __restrict__ w1frag, const float* __restrict__ b1, const u32x4q* __restrict__ w2frag,
       const float* __restrict__ b2, int N, int H, int W, int H1, int W1, int H2, int W2, int CO, int tiles_x, int tiles_y, int y16 RCX_STAMP_ARG)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    constexpr int KS = 9 * (KC / 16), NF = MT * KS, PIX = 2 * KC + 16, R = 17;      // k-steps, W2 fragments, bytes per pixel of the h1 tile (16 of padding: banks)
    constexpr int M1 = (CM + 31) / 32, XR = 35, XE = 105, XP = 216, XROWS = 38;      // x tile: 35 rows of 36 pixels x 3 channels (216 bytes: image pixels 32 tx - 4 ..; the first is not read)
    constexpr int NPT = (R * R + 31) / 32;                                           // pixel tiles of the first product; the h1 tile holds 32 NPT pixels, the x tile 38 rows: no guarded LDS writes
    const u32x4q* const Lf = reinterpret_cast<const u32x4q*>(lds_raw);               // [NF] W2 fragments, then [2 M1] W1 fragments
    const u32x4q* const Lf1 = Lf + NF * 64;
    unsigned char* const Lh = lds_raw + (size_t)(NF + 2 * M1) * 1024;                // h1 tile [17 x 17][PIX]
    unsigned char* const Lx = Lh + (size_t)32 * NPT * PIX;                           // x tile [38][XP]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    unsigned char* const Ly = Lx + (size_t)XROWS * XP + (size_t)wave * YIMG;         // this wave's output image: [32 pixels][32 channels] bf16
    {                                                                                // the weights: once per workgroup (it walks tiles blockIdx.x, + gridDim.x, ...)
        u32x4q* Lw = reinterpret_cast<u32x4q*>(lds_raw);
        for (int i = threadIdx.x; i < NF * 64; i += 256) Lw[i] = w2frag[i];
        for (int i = threadIdx.x; i < 2 * M1 * 64; i += 256) Lw[NF * 64 + i] = w1frag[i];
    }
    // the biases a lane adds, in registers for the whole walk (they depend on neither the pixel tile, the tile nor the image): of the first product's channel groups
    // g (channels 32 m1 + 8 g + 4 h ..+3 below KC), and of the (output tile, pixel tile) pairs pr = wave + 4 pi this wave takes in phase B.  Both packs are padded to 32s.
    constexpr int NPR = (2 * MT + 3) / 4;
    f32x4q b1r[M1][4], b2r[NPR][4];
#pragma unroll
    for (int m1 = 0; m1 < M1; ++m1)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float* const bp = b1 + 32 * m1 + 8 * g + 4 * h;
            b1r[m1][g] = 32 * m1 + 8 * g < KC ? f32x4q{bp[0], bp[1], bp[2], bp[3]} : f32x4q{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
    for (int pi = 0; pi < NPR; ++pi)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int pr = wave + 4 * pi;
            const float* const bp = b2 + 32 * ((pr < 2 * MT ? pr : 0) >> 1) + 8 * g + 4 * h;
            b2r[pi][g] = f32x4q{bp[0], bp[1], bp[2], bp[3]};
        }
    const unsigned xbytes = (unsigned)H * (unsigned)W * 6u;                          // one image of x (3 channels, bf16); checked < 2^31 by the launcher
    // the x tile of a tile: rows 32 ty - 3 + i of the image, bytes 6 (32 tx - 4) .. + 216 of each (zeros outside the image: the first conv's padding).  The tile starts
    // a pixel left of the first one read so that, with XW, its rows are 27 aligned 8-byte pieces of the image: piece e of the tile (row e / 27) lands at LDS byte 8 e,
    // four pieces a thread.  Without XW: 35 pixels a row from 32 tx - 3 as single bf16, fifteen a thread.  Either way a thread's pieces are requested a tile ahead
    // (during the previous tile's second product) and written to LDS at the top of the tile.
    constexpr int XN = XW ? 4 : (XR * XE + 255) / 256;
    static_assert(4 * 256 * 8 <= XROWS * XP && ((XR * XE + 255) / 256 * 256 + XE - 1) / XE <= XROWS, "the spare x-tile rows take the last round's overshoot");
    unsigned xgo[XN], xlo[XN], xij[XN];               // piece u of this thread: offset within the image relative to the tile's first byte, LDS offset, (row, pixel | piece) of the tile
#pragma unroll
    for (int u = 0; u < XN; ++u) {
        const int e = threadIdx.x + 256 * u;
        if constexpr (XW) {
            const int i = e / 27, k = e - 27 * i;
            xgo[u] = (unsigned)(i * W) * 6u + 8u * (unsigned)k;
            xlo[u] = 8u * (unsigned)e;
            xij[u] = (unsigned)i | ((unsigned)k << 8) | (e < XR * 27 ? 0u : 0x10000u);
        } else {
            const int i = e / XE, q = e - i * XE, px = q / 3;
            xgo[u] = ((unsigned)(i * W + px) * 3u + (unsigned)(q - 3 * px)) * 2u + 6u;
            xlo[u] = (unsigned)(i * XP + 2 * q + 6);
            xij[u] = (unsigned)i | ((unsigned)px << 8) | (e < XR * XE ? 0u : 0x10000u);
        }
    }
    typename std::conditional<XW, u32x2q, bf16_t>::type xq[XN];
    auto request_x = [&](int t) {
        const int nn = t / (tiles_x * tiles_y), trr = t - nn * tiles_x * tiles_y, tyy = trr / tiles_x, txx = trr - tyy * tiles_x;
        const __amdgpu_buffer_rsrc_t xsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (size_t)nn * H * W * 3), 0, xbytes, 0x00020000);
        const int y0 = 32 * tyy - 3, x0 = 32 * txx - 4;
        const unsigned base = (unsigned)((y0 * W + x0) * 6);                       // (may wrap below zero: only added to offsets of pieces inside the image)
#pragma unroll
        for (int u = 0; u < XN; ++u) {
            const int yy = y0 + (int)(xij[u] & 0xff);
            if constexpr (XW) {
                const int cb = 6 * x0 + 8 * (int)((xij[u] >> 8) & 0xff);            // the piece's first byte within the row
                const bool ok = xij[u] < 0x10000u && yy >= 0 && yy < H && cb >= 0 && cb < 6 * W;
                xq[u] = __builtin_amdgcn_raw_buffer_load_b64(xsrc, (int)(ok ? base + xgo[u] : 0x80000000u), 0, 0);           // outside the image: past the buffer, reads 0
            } else {
                const int xx = x0 + 1 + (int)((xij[u] >> 8) & 0xff);
                const bool ok = xij[u] < 0x10000u && yy >= 0 && yy < H && xx >= 0 && xx < W;
                xq[u] = (bf16_t)__builtin_amdgcn_raw_buffer_load_b16(xsrc, (int)(ok ? base + xgo[u] : 0x80000000u), 0, 0);
            }
        }
    };
    const int ntiles = N * tiles_x * tiles_y;
    if ((int)blockIdx.x < ntiles) request_x(blockIdx.x);
#ifdef RCX_STEM_STAMPS
    unsigned long long tsum[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tlast = 0;      // ten phases (tools/stem_timeline.py names them) and the tiles walked
    RCX_STAMP(10)
    tsum[10] = 0;
#endif
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = tile / (tiles_x * tiles_y), tr = tile - n * tiles_x * tiles_y, ty = tr / tiles_x, tx = tr - ty * tiles_x;
#pragma unroll
    for (int u = 0; u < XN; ++u) *reinterpret_cast<decltype(&xq[0])>(Lx + xlo[u]) = xq[u];
    RCX_STAMP(0)
    __syncthreads();
    RCX_STAMP(1)
    //                                  // the x tile (and, the first time, the weights) is in LDS; every wave has left the previous tile's second product

    // ---- A. the intermediate's 17 x 17 pixels (rows 16 ty - 1 + i, columns 16 tx - 1 + j) on the matrix cores: D (32 channels x 32 pixels) = W1 (channel x 27 taps,
    // padded to 32) x im2col.  Pixel (i, j) reads x-tile rows 2 i + dy, elements 6 j .. 6 j + 8: its 27 inputs are three runs of nine contiguous bf16, k = 9 dy + e.
    unsigned koff[2][8];                                                            // byte offset of input k = 16 ks + 8 h + jj from the pixel's first element
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int kk = 16 * ks + 8 * h + jj, dy = (kk * 57) >> 9;
            koff[ks][jj] = kk < 27 ? (unsigned)(dy * XP + 2 * (kk - 9 * dy)) : 0u;         // (k = 27 .. 31: zero weights; any input of the pixel's own window will do)
        }
    bf16x8 w1f[2 * M1];                                                             // the W1 fragments: the same for the wave's three pixel tiles
#pragma unroll
    for (int q = 0; q < 2 * M1; ++q) w1f[q] = __builtin_bit_cast(bf16x8, Lf1[q * 64 + lane]);
    // The ten pixel tiles in three rounds: wave w takes pixel tiles w and w + 4 whole; the last two, 8 and 9, are each gathered and multiplied by BOTH waves of a pair
    // (w >> 1), and each wave of the pair takes every other channel group of it through bias, GELU and the write: 2.5 epilogues a wave instead of 3 | 3 | 2 | 2.
    static_assert(NPT == 10, "three rounds of pixel tiles: 4 + 4 + 2");
    int pp[3];
    bool pin[3];
    const unsigned char* pxp[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int pt = t < 2 ? wave + 4 * t : 8 + (wave >> 1);
        const int p = 32 * pt + r, pc = p < R * R ? p : R * R - 1, i = pc / R, j = pc - i * R;
        const int r1 = 16 * ty - 1 + i, c1 = 16 * tx - 1 + j;
        pp[t] = p;
        pin[t] = p < R * R && r1 >= 0 && r1 < H1 && c1 >= 0 && c1 < W1;
        pxp[t] = Lx + (2 * i) * XP + 12 * j + 6;
    }
    // a pixel tile in three pieces, so that the next one's LDS reads and products are in flight under this one's GELU:
    auto gather = [&](const unsigned char* xp, unsigned (&v)[16]) {                  // the 16 im2col inputs of this lane: requests only
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) v[8 * ks + jj] = *reinterpret_cast<const unsigned short*>(xp + koff[ks][jj]);
    };
    auto products = [&](const unsigned (&v)[16], f32x16 (&d)[M1]) {                  // (waits for the inputs) pack, then the 2 M1 products
        bf16x8 bfr[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const unsigned* const w = v + 8 * ks;
            const u32x4q pk = {w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16)};
            bfr[ks] = __builtin_bit_cast(bf16x8, pk);
        }
#pragma unroll
        for (int m1 = 0; m1 < M1; ++m1) {
#pragma unroll
            for (int q = 0; q < 16; ++q) d[m1][q] = 0.f;
            d[m1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1f[2 * m1 + 0], bfr[0], d[m1], 0, 0, 0);
            d[m1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1f[2 * m1 + 1], bfr[1], d[m1], 0, 0, 0);
        }
#ifdef RCX_STEM_STAMPS
        asm volatile("" ::"s"(__builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, d[M1 - 1][15]))));       // the products have landed
        RCX_STAMP(3)
#endif
    };
    // + b1, gelu, bf16 -> the h1 tile (pixels outside the intermediate's plane: zeros, the second conv's padding; channels past CM: zero weights and bias), for the
    // channel groups g = G0, G0 + GS, .. < GE of product tile m1 that lie below KC: their GELUs in lockstep (rcx_gelu.h), then the converts, selects and writes as a block
    auto epilogue = [&](auto M1I, auto G0, auto GS, auto GE, const f32x16& d, int p, bool inside) {
        constexpr int m1 = decltype(M1I)::value, g0 = decltype(G0)::value, gs = decltype(GS)::value, ge = decltype(GE)::value;
        constexpr int GA = KC - 32 * m1 >= 32 ? 4 : (KC - 32 * m1) / 8, GL = GA < ge ? GA : ge, NG = GL > g0 ? (GL - g0 + gs - 1) / gs : 0;
        if constexpr (NG > 0) {
            gelu_f32x2 v[2 * NG];
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                const int g = g0 + gs * k;
                const f32x4q bb = b1r[m1][g];
                v[2 * k] = gelu_f32x2{d[4 * g] + bb.x, d[4 * g + 1] + bb.y};
                v[2 * k + 1] = gelu_f32x2{d[4 * g + 2] + bb.z, d[4 * g + 3] + bb.w};
            }
            gelu2_batch<2 * NG>(v);
            RCX_STAMP(4)
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                const int c0 = 32 * m1 + 8 * (g0 + gs * k) + 4 * h;
                const gelu_f32x2 a = v[2 * k], b = v[2 * k + 1];
                bf16x4 o;
                o[0] = (__bf16)(inside ? a.x : 0.f); o[1] = (__bf16)(inside ? a.y : 0.f); o[2] = (__bf16)(inside ? b.x : 0.f); o[3] = (__bf16)(inside ? b.y : 0.f);
                *reinterpret_cast<u32x2q*>(Lh + (size_t)p * PIX + 2 * c0) = __builtin_bit_cast(u32x2q, o);
            }
            RCX_STAMP(5)
        }
    };
    using C0 = std::integral_constant<int, 0>;
    using C1 = std::integral_constant<int, 1>;
    using C2 = std::integral_constant<int, 2>;
    using C4 = std::integral_constant<int, 4>;
    auto epilogue_half = [&](auto HF, const f32x16 (&d)[M1], int p, bool inside) {   // groups 2 HF, 2 HF + 1 of every product tile
        constexpr int hf = decltype(HF)::value;
        epilogue(C0{}, std::integral_constant<int, 2 * hf>{}, C1{}, std::integral_constant<int, 2 * hf + 2>{}, d[0], p, inside);
        if constexpr (M1 == 2) epilogue(C1{}, std::integral_constant<int, 2 * hf>{}, C1{}, std::integral_constant<int, 2 * hf + 2>{}, d[M1 - 1], p, inside);
    };
    auto epilogue_every_other = [&](auto PAR, const f32x16 (&d)[M1], int p, bool inside) {      // groups PAR, PAR + 2
        epilogue(C0{}, PAR, C2{}, C4{}, d[0], p, inside);
        if constexpr (M1 == 2) epilogue(C1{}, PAR, C2{}, C4{}, d[M1 - 1], p, inside);
    };
    // The schedule (sched_barrier: the compiler keeps the pieces in this order; the waits it places are counted, the h1 writes behind a gather stay in flight):
    // the requests of pixel tile t + 1 go out before the GELU of pixel tile t, its products are issued between the two halves of that GELU and run under the second.
    f32x16 dA[M1], dB[M1];
    unsigned va[16], vb[16];
    gather(pxp[0], va);
    RCX_STAMP(2)
    products(va, dA);
    gather(pxp[1], vb);
    RCX_STAMP(2)
    __builtin_amdgcn_sched_barrier(0);
    epilogue_half(C0{}, dA, pp[0], pin[0]);
    __builtin_amdgcn_sched_barrier(0);
    products(vb, dB);
    __builtin_amdgcn_sched_barrier(0);
    epilogue_half(C1{}, dA, pp[0], pin[0]);
    __builtin_amdgcn_sched_barrier(0);
    gather(pxp[2], va);
    RCX_STAMP(2)
    __builtin_amdgcn_sched_barrier(0);
    epilogue_half(C0{}, dB, pp[1], pin[1]);
    __builtin_amdgcn_sched_barrier(0);
    products(va, dA);
    __builtin_amdgcn_sched_barrier(0);
    epilogue_half(C1{}, dB, pp[1], pin[1]);
    __builtin_amdgcn_sched_barrier(0);
    if (wave & 1) epilogue_every_other(C1{}, dA, pp[2], pin[2]);
    else epilogue_every_other(C0{}, dA, pp[2], pin[2]);
    __syncthreads();
    RCX_STAMP(6)
    if (tile + (int)gridDim.x < ntiles) request_x(tile + gridDim.x);
    RCX_STAMP(7)

    // ---- B. conv2: wave w takes the (output tile mt, pixel tile nt) pairs w, w + 4, ...; pixel q of the 8 x 8 tile = (q / 8, q % 8)
#pragma unroll
    for (int pi = 0; pi < NPR; ++pi) {
        const int pr = wave + 4 * pi;
        if (pr >= 2 * MT) break;
        const int mt = pr >> 1, nt = pr & 1;
        const int q = 32 * nt + r, py = q >> 3, px = q & 7;      // (the product's pixel of this lane)
        const unsigned char* const hp = Lh + (size_t)((2 * py) * R + 2 * px) * PIX + 16 * h;
        f32x16 d0, d1;
#pragma unroll
        for (int i = 0; i < 16; ++i) { d0[i] = 0.f; d1[i] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            constexpr int KG = KC / 16;
            const int t = ks / KG, cg = ks - t * KG, dy = t / 3, dx = t - 3 * dy;
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(hp + (size_t)(dy * R + dx) * PIX + 32 * cg);
            const bf16x8 a = __builtin_bit_cast(bf16x8, Lf[(mt * KS + ks) * 64 + lane]);
            if (ks & 1) d1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, d1, 0, 0, 0);
            else d0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, d0, 0, 0, 0);
        }
#ifdef RCX_STEM_STAMPS
        asm volatile("" ::"s"(__builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, d0[15]))), "s"(__builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, d1[15]))));
        RCX_STAMP(8)
#endif
        // + b2 -> bf16 -> this wave's LDS image (pixel r: 64 bytes, its 8-byte pieces XOR-ed with (r >> 1) & 7: a store's 16 lanes hit 16 bank pairs), then out with a
        // pixel's 64 bytes contiguous across 4 lanes (16 bytes each; 8 lanes of 8 bytes where 2 CO or y is not 16-byte aligned): a request covers whole 64-byte runs of y
        // instead of 8 bytes of each of 32 pixels.  GO: the eight pairs' GELUs in lockstep, then the converts and the four writes as a block
        gelu_f32x2 v[8];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4q bb = b2r[pi][g];
            v[2 * g] = gelu_f32x2{d0[4 * g + 0] + d1[4 * g + 0] + bb.x, d0[4 * g + 1] + d1[4 * g + 1] + bb.y};
            v[2 * g + 1] = gelu_f32x2{d0[4 * g + 2] + d1[4 * g + 2] + bb.z, d0[4 * g + 3] + d1[4 * g + 3] + bb.w};
        }
        if constexpr (GO) gelu2_batch<8>(v);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x4 o;
            o[0] = (__bf16)v[2 * g].x; o[1] = (__bf16)v[2 * g].y; o[2] = (__bf16)v[2 * g + 1].x; o[3] = (__bf16)v[2 * g + 1].y;
            *reinterpret_cast<u32x2q*>(Ly + 64 * r + 8 * ((2 * g + h) ^ ((r >> 1) & 7))) = __builtin_bit_cast(u32x2q, o);
        }
        wave_sync();
        if (y16) {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int ql = 16 * it + (lane >> 2), ck = lane & 3, sw = (ql >> 1) & 7, q2 = 32 * nt + ql, oy = 8 * ty + (q2 >> 3), ox = 8 * tx + (q2 & 7), c0 = 32 * mt + 8 * ck;
                const u32x2q lo = *reinterpret_cast<const u32x2q*>(Ly + 64 * ql + 8 * ((2 * ck) ^ sw)), hi = *reinterpret_cast<const u32x2q*>(Ly + 64 * ql + 8 * ((2 * ck + 1) ^ sw));
                if (oy < H2 && ox < W2 && c0 < CO) *reinterpret_cast<u32x4q*>(y + ((size_t)(n * H2 + oy) * W2 + ox) * CO + c0) = u32x4q{lo.x, lo.y, hi.x, hi.y};
            }
        } else {
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int ql = 8 * it + (lane >> 3), ck = lane & 7, sw = (ql >> 1) & 7, q2 = 32 * nt + ql, oy = 8 * ty + (q2 >> 3), ox = 8 * tx + (q2 & 7), c0 = 32 * mt + 4 * ck;
                const u32x2q v = *reinterpret_cast<const u32x2q*>(Ly + 64 * ql + 8 * (ck ^ sw));
                if (oy < H2 && ox < W2 && c0 < CO) *reinterpret_cast<u32x2q*>(y + ((size_t)(n * H2 + oy) * W2 + ox) * CO + c0) = v;
            }
        }
        wave_sync();                                   // (MT = 3: the wave's next pair writes the image again)
        RCX_STAMP(9)
    }
#ifdef RCX_STEM_STAMPS
    tsum[10] += 1;
#endif
    }
#ifdef RCX_STEM_STAMPS
    if (lane == 0)
        for (int k = 0; k < 11; ++k) stamps[((size_t)blockIdx.x * 4 + wave) * 11 + k] = tsum[k];
#endif
}

}  // namespace stem

// CM (even, <= 40), CO (multiple of 4, <= 96), bf16; one image of x below 2^31 bytes
static bool stem_shape(int CM, int CO, int* kc, int* mt)
{
    if (CM <= 0 || CM > 40 || (CM & 1) || CO <= 0 || CO > 96 || CO % 4) return false;
    *kc = (CM + 15) / 16 * 16;
    *mt = (CO + 31) / 32;
    return CM == 20 || CM == 24 || CM == 28 || CM == 32 || CM == 40;
}

bool stem_applicable(int N, int H, int W, int CM, int CO, int dtype)
{
    int kc, mt;
    return dtype == 1 && N > 0 && H > 0 && W > 0 && (unsigned long long)H * W * 6 < (1ull << 31) && stem_shape(CM, CO, &kc, &mt);
}

size_t stem_pack_bytes(int CM, int CO)
{
    int kc, mt;
    if (!stem_shape(CM, CO, &kc, &mt)) return 0;
    return (size_t)mt * 9 * (kc / 16) * 1024;
}

// GO: see k_stem; ONLY = the one MT the caller has (0: all three) -- the T / S / B front needs one per channel set
template <int CM, int KC, bool GO = false, int ONLY = 0>
static hipError_t launch_stem(const void* x, void* y, const void* w1, const float* b1, const void* w2frag, const float* b2, int N, int H, int W, int CO, int MT, int ncu, hipStream_t s)
{
    const int H1 = (H + 1) / 2, W1 = (W + 1) / 2, H2 = (H1 + 1) / 2, W2 = (W1 + 1) / 2, tx = (W2 + 7) / 8, ty = (H2 + 7) / 8;
    constexpr int KS = 9 * (KC / 16), PIX = 2 * KC + 16;
    constexpr int M1 = (CM + 31) / 32;
    const size_t lds = (size_t)(MT * KS + 2 * M1) * 1024 + (size_t)320 * PIX + (size_t)38 * 216 + (size_t)4 * stem::YIMG;      // (the biases live in registers)
    // rows of x as 8-byte pieces where every row of every image starts on one (else as single bf16); 16-byte stores where every pixel of y does (else 8-byte)
    const bool xw = W % 4 == 0 && ((size_t)x & 7) == 0;
    const int y16 = CO % 8 == 0 && ((size_t)y & 15) == 0;
    const long long ntiles = (long long)N * tx * ty;
    if (ntiles > 0x7fffffffLL || lds > 160 * 1024) return hipErrorInvalidConfiguration;
    const long long per_cu = (long long)(160 * 1024 / lds) > 0 ? (long long)(160 * 1024 / lds) : 1;
    const long long grid = ntiles < ncu * per_cu ? ntiles : ncu * per_cu;          // persistent: the weights go to LDS once per workgroup
#define RCX_STEM_GO(MT_, XW_)                                                                                                              \
    {                                                                                                                                      \
        auto kfn = stem::k_stem<CM, KC, MT_, XW_, GO>;                                                                                     \
        RCX_SET_LDS_ONCE(kfn, lds);                                                                                                        \
        hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(256), lds, s, (const bf16_t*)x, (bf16_t*)y, (const stem::u32x4q*)w1, b1, (const stem::u32x4q*)w2frag, b2, \
                           N, H, W, H1, W1, H2, W2, CO, tx, ty, y16 RCX_STAMP_VAL);                                                        \
        return hipGetLastError();                                                                                                          \
    }
    if constexpr (ONLY == 0 || ONLY == 1) {
        if (MT == 1 && xw) RCX_STEM_GO(1, true)
        if (MT == 1) RCX_STEM_GO(1, false)
    }
    if constexpr (ONLY == 0 || ONLY == 2) {
        if (MT == 2 && xw) RCX_STEM_GO(2, true)
        if (MT == 2) RCX_STEM_GO(2, false)
    }
    if constexpr (ONLY == 0 || ONLY == 3) {
        if (MT == 3 && xw) RCX_STEM_GO(3, true)
        if (MT == 3) RCX_STEM_GO(3, false)
    }
#undef RCX_STEM_GO
    return hipErrorInvalidConfiguration;
}

// compute units of the current device, asked once per device (the persistent grids of this file and of rcx_conv3s2.hip)
int stem_device_cus()
{
    static std::atomic<int> cus[RCX_MAX_DEVICES];
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < RCX_MAX_DEVICES) {
        ncu = cus[dev].load(std::memory_order_relaxed);
        if (ncu <= 0) {
            int v = 0;
            ncu = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0 ? v : 256;
            cus[dev].store(ncu, std::memory_order_relaxed);
        }
    }
    return ncu;
}

hipError_t stem_fwd(const void* x, void* y, const void* w1, const float* b1, const void* w2frag, const float* b2, int N, int H, int W, int CM, int CO, int dtype, hipStream_t s)
{
    int kc, mt;
    if (!stem_applicable(N, H, W, CM, CO, dtype) || !stem_shape(CM, CO, &kc, &mt)) return hipErrorInvalidConfiguration;
    const int ncu = stem_device_cus();
    switch (CM) {
        case 20: return launch_stem<20, 32>(x, y, w1, b1, w2frag, b2, N, H, W, CO, mt, ncu, s);
        case 24: return launch_stem<24, 32>(x, y, w1, b1, w2frag, b2, N, H, W, CO, mt, ncu, s);
        case 28: return launch_stem<28, 32>(x, y, w1, b1, w2frag, b2, N, H, W, CO, mt, ncu, s);
        case 32: return launch_stem<32, 32>(x, y, w1, b1, w2frag, b2, N, H, W, CO, mt, ncu, s);
        case 40: return launch_stem<40, 48>(x, y, w1, b1, w2frag, b2, N, H, W, CO, mt, ncu, s);
        default: return hipErrorInvalidConfiguration;
    }
}

// The front of the T / S / B stem (lsnet/model/recattn.py:208-223): y = gelu(conv2(gelu(conv1(x) + b1)) + b2), (CM, CO) = (16, 32) for T and (32, 64) for S / B;
// rcx_conv3s2.hip takes y through the third conv.  The same kernel as above with the GELU in its output epilogue; the packs are ops.pack_stem's.
hipError_t stem_front_fwd(const void* x, void* y, const void* w1, const float* b1, const void* w2frag, const float* b2, int N, int H, int W, int CM, hipStream_t s)
{
    if (N <= 0 || H <= 0 || W <= 0 || (unsigned long long)H * W * 6 >= (1ull << 31)) return hipErrorInvalidConfiguration;
    if (CM == 16) return launch_stem<16, 16, true, 1>(x, y, w1, b1, w2frag, b2, N, H, W, 32, 1, stem_device_cus(), s);
    if (CM == 32) return launch_stem<32, 32, true, 2>(x, y, w1, b1, w2frag, b2, N, H, W, 64, 2, stem_device_cus(), s);
    return hipErrorInvalidConfiguration;
}

}  // namespace rcx

#ifdef RCX_STEM_STAMPS
// the diagnostic build: this translation unit alone as a shared object (tools/stem_timeline.py); stamps = [grid][4 waves][11] cycle sums
extern "C" int rcx_stem_diag_fwd(const void* x, void* y, const void* w1frag, const float* b1, const void* w2frag, const float* b2, int N, int H, int W, int CM, int CO, void* stamps, void* stream)
{
    rcx::g_stamps = (unsigned long long*)stamps;
    return (int)rcx::stem_fwd(x, y, w1frag, b1, w2frag, b2, N, H, W, CM, CO, 1, (hipStream_t)stream);
}
#endif

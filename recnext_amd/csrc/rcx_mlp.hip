// The channel mixer of a MetaNeXtBlock and the residual add around it in ONE launch (inference, bf16 activations):
//     y = x + W2 gelu(W1 z + b1) + b2          (model/recnext.py:125-132 `mlp`, :157-158 `x + drop_path(channel_mixer(norm(token_mixer(x))))`, :169-171 Downsample;
//                                               model/recattn.py:171, :184)
// z = the token mixer's output (its BatchNorm already folded into the mixer's last conv), x = the block's input, W1 (H x C) / W2 (C x H) the two BN-folded 1x1
// convs.  As four library launches (GEMM + bias, GELU, GEMM + bias, add) the hidden tensor -- 2 x the size of x -- is written and read twice and y once more:
// 7 S of traffic where x, z in and y out are 3 S; at the 56 x 56 and 28 x 28 stages (C = 64 / 128) these GEMMs are memory-bound, so that is most of the cost.
//
// ONE WAVE = 32 tokens at a time, the hidden layer streamed through its registers 32 units at a time, never in memory:
//   D1  (32 hidden units x 32 tokens) = W1[32 ht ..][:] z^T      v_mfma_f32_32x32x16_bf16: A = a W1 fragment (LDS), B = the tokens' channels (registers, loaded
//                                                               once per tile straight from memory: 16 bytes per lane and k-step)
//   h   = 2 gelu(D1 + b1) in float32, rounded to bf16 (W2 is packed halved: exact)   the accumulator layout (token on the lane, units in the registers) IS the B operand of ...
//   D2 += W2[:][32 ht ..] h                                      ... the second product, with W2's columns stored in the order the registers imply
//   y   = D2 + b2 + x                                            8-byte loads / stores of four channels per lane (token on the lane)
// The weights are ready-made fragments (one conflict-free 16-byte LDS read per lane and product), packed once on the host (ops.pack_channel_mlp), hidden tile by
// hidden tile: resident in LDS for C <= 128 (k_channel_mlp; C = 128: k_channel_mlp_res128, free-running waves), streamed through a two-slot LDS ring for
// C = 160 .. 320 (k_channel_mlp_stream; C = 256: k_channel_mlp_pair, two waves per SIMD), read straight from global memory by the wave that owns them for
// C = 384 / 512 (k_channel_mlp_wide).  Global accesses are whole-wave contiguous kilobytes, transposed to / from the token-on-lane layouts in per-wave LDS
// images (measurements: profiles/r05_channel_mlp.txt).
// GELU is the exact form 0.5 v (1 + erf(v / sqrt 2)) with erf as an odd degree-15 polynomial of the argument clamped to +-2.8: |error| < 7.7e-5 in erf, i.e. 4e-5 |v|
// in gelu -- a fiftieth of a bf16 ulp; the library's erff would be most of this kernel's vector work.
// The file: the text all forms share and each form's LDS layout (one struct, read by the kernel and by its launcher); the hidden step; the five kernels, each its
// schedule and nothing else; a launcher per form; MLP_ROWS, the one table of the shapes that have a kernel, which channel_mlp_applicable and channel_mlp both read.
// No kernel-side piece is shared at the cost of a kernel's schedule: the compiler's schedule for these kernels depends on how the source is factored, so a piece
// is a function where the device listing stayed the same and a macro where a function moved it.
#include "rcx_common.h"
#include "rcx_launch.h"
#include "rcx_gelu.h"
#include <type_traits>

// -DRCX_MLP_STAMPS is the diagnostic build of this file alone (tools/mlp_timeline.py): s_memtime at the phase boundaries of a hidden step, summed per wave into a
// buffer of the tool's own -- [wave slot][8]: 0 ring preload, 1 D1, 2 b1 + GELU, 3 D2, 4 barrier / DMA wait, 5 the tile's prologue and epilogue, 6 hidden steps.
// Each stamp drains the wave's LDS reads (s_memtime returns through the same counter), so a request that the product build keeps in flight across a phase
// boundary lands in the phase that issued it; a product's own latency shows in the phase that first reads its result.  Without the macro all of it expands to nothing.
#ifdef RCX_MLP_STAMPS
#define RCX_MLP_STAMP(k)                                                                                        \
    {                                                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                      \
        unsigned long long t_;                                                                                  \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                              \
        __builtin_amdgcn_sched_barrier(0);                                                                      \
        tsum[k] += t_ - tlast;                                                                                  \
        tlast = t_;                                                                                             \
    }
#define RCX_MLP_STAMP_BEGIN                                                                                     \
    unsigned long long tsum[7] = {0, 0, 0, 0, 0, 0, 0}, tlast;                                                  \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tlast)::"memory");
#define RCX_MLP_STAMP_STEP tsum[6] += 1;
#define RCX_MLP_STAMP_END(slot)                                                                                 \
    if (stamps && (threadIdx.x & 63) == 0) {                                                                    \
        _Pragma("unroll") for (int k_ = 0; k_ < 7; ++k_) stamps[(size_t)(slot) * 8 + k_] = tsum[k_];            \
    }
#define RCX_MLP_STAMP_PARM , unsigned long long (&tsum)[7], unsigned long long& tlast
#define RCX_MLP_STAMP_PASS , tsum, tlast
#define RCX_MLP_STAMP_ARG , unsigned long long* __restrict__ stamps
#define RCX_MLP_STAMP_VAL , g_stamps
namespace rcx {
static unsigned long long* g_stamps = nullptr;
}
#else
#define RCX_MLP_STAMP(k)
#define RCX_MLP_STAMP_BEGIN
#define RCX_MLP_STAMP_STEP
#define RCX_MLP_STAMP_END(slot)
#define RCX_MLP_STAMP_PARM
#define RCX_MLP_STAMP_PASS
#define RCX_MLP_STAMP_ARG
#define RCX_MLP_STAMP_VAL
#endif

// k_channel_mlp_pair runs the hidden step in its pinned form (hidden_tile_pinned); -DRCX_MLP_PINNED=false builds it in hidden_tile_ring's, as the compiler
// schedules it: the "before" of tools/mlp_timeline.py
#ifndef RCX_MLP_PINNED
#define RCX_MLP_PINNED true
#endif

namespace rcx {
namespace mlp {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4q __attribute__((ext_vector_type(4)));
typedef float f32x2q __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4q __attribute__((ext_vector_type(4)));
typedef unsigned u32x2q __attribute__((ext_vector_type(2)));

// LDS operations of one wave execute in order; this only keeps the compiler from moving accesses across a hand-off within the wave
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// (row of accumulator register i in lane half h of a 32 x 32 tile: (i & 3) + 8 (i >> 2) + 4 h -- ops.py::_mlp_acc_unit orders W2's columns by it)

// ---- the text every kernel form shares.  Each piece is here only because the device listing of every kernel stayed the same, instruction for instruction, when
// the in-place text became a call (or, where a call moved the schedule, a macro)

// z, x and y as buffers of M token rows (nbytes < 2^31, checked by the launcher): a token past M reads 0 and its stores are dropped; an offset with bit 31 set is
// out of range whatever the token
__device__ __forceinline__ __amdgpu_buffer_rsrc_t token_rows(const void* p, unsigned nbytes) { return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, nbytes, 0x00020000); }

// Accumulators D[N] = 0.  A macro: as a function it moved the listings of the stream, pair and wide kernels (other registers, another order)
#define RCX_MLP_ZERO(D, N)                                                                                                                \
    _Pragma("unroll") for (int n_ = 0; n_ < N; ++n_) _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) D[n_][i_] = 0.f;

// The tokens' channels zq[KS1] -> the first product's B operands zb[KS1] through the wave's image Lt (rows of ZP bytes), in ZH column parts of KH = KS1 / ZH
// k-steps: request i of part q goes to byte ZA (an expression in q and i) of the image, then lane (r, h) reads k-step k of its token's row back.  A macro over
// the kernel's own names: as a function taking ZA as a lambda it moved the listings of the pair kernel and two stream kernels
#define RCX_MLP_STAGE_Z(ZA)                                                                                                               \
    _Pragma("unroll") for (int q = 0; q < ZH; ++q) {                                                                                      \
        _Pragma("unroll") for (int i = 0; i < KH; ++i) *reinterpret_cast<u32x4q*>(Lt + (ZA)) = zq[q * KH + i];                            \
        wave_sync();                                                                                                                      \
        _Pragma("unroll") for (int k = 0; k < KH; ++k)                                                                                    \
            zb[q * KH + k] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4q*>(Lt + r * ZP + 32 * k + 16 * h));                 \
        wave_sync();                                                                                                                      \
    }

// Four accumulators of a lane (register group g of D2: its token's channels 8 g + 4 h .. + 3 of an output tile) + b2 -> the float32 image.  A macro: as a function
// it moved the listings of the stream, pair and wide kernels
#define RCX_MLP_IMAGE_QUAD(D2, B2, DST)                                                                                                   \
    {                                                                                                                                     \
        const f32x4q bb = *reinterpret_cast<const f32x4q*>(B2);                                                                           \
        *reinterpret_cast<f32x4q*>(DST) = f32x4q{D2[4 * g] + bb.x, D2[4 * g + 1] + bb.y, D2[4 * g + 2] + bb.z, D2[4 * g + 3] + bb.w};     \
    }

// 8 channels of a token's row: the float32 image's (lo, hi) + the residual's (bf16 pairs), rounded once
__device__ __forceinline__ bf16x8 rows_plus_x(f32x4q lo, f32x4q hi, u32x4q xv)
{
    bf16x8 o;
    o[0] = (__bf16)(lo.x + __uint_as_float(xv.x << 16)); o[1] = (__bf16)(lo.y + __uint_as_float(xv.x & 0xffff0000u));
    o[2] = (__bf16)(lo.z + __uint_as_float(xv.y << 16)); o[3] = (__bf16)(lo.w + __uint_as_float(xv.y & 0xffff0000u));
    o[4] = (__bf16)(hi.x + __uint_as_float(xv.z << 16)); o[5] = (__bf16)(hi.y + __uint_as_float(xv.z & 0xffff0000u));
    o[6] = (__bf16)(hi.z + __uint_as_float(xv.w << 16)); o[7] = (__bf16)(hi.w + __uint_as_float(xv.w & 0xffff0000u));
    return o;
}

// ---- the dynamic LDS of every form, ONE statement for the kernel (offsets) and its launcher (bytes):
//     [weights: the resident pack | the ring of chunks | wide: the B operands]  [b1: 32 HT floats] [b2: 32 CT floats]  [NW per-wave images of IMG bytes]
// The pack: per hidden tile its KS1 W1 fragments and 2 CT W2 fragments (1 KB each: 64 lanes x 16 bytes; ops.pack_channel_mlp).  An image holds a wave's 32 tokens
// as rows, the bf16 z (pitch ZP) and then the float32 output (pitch OP) -- 16 bytes of padding a row: banks
constexpr int imax(int a, int b) { return a > b ? a : b; }
constexpr size_t bias_bytes(int HT, int CT) { return sizeof(float) * 32 * (HT + CT); }

// k_channel_mlp: the pack resident; images of whole rows, only where STAGED
template <int KS1, int HT, int CT, int NW, bool STAGED>
struct SmallLds {
    static constexpr int NF = HT * (KS1 + 2 * CT), ZP = 32 * KS1 + 16, OP = 128 * CT + 16, IMG = STAGED ? 32 * imax(ZP, OP) : 0;
    static constexpr size_t b1 = (size_t)NF * 1024, images = b1 + bias_bytes(HT, CT), bytes = images + (size_t)NW * IMG;
};
// k_channel_mlp_stream: a ring of two chunks; z rows in ZH column parts, the output in halves of two tiles (64 channels)
template <int KS1, int HT, int CT, int NW, int ZH>
struct StreamLds {
    static constexpr int NCH = KS1 + 2 * CT, ZP = 32 * KS1 / ZH + 16, OP = 256 + 16, IMG = 32 * imax(ZP, OP);
    static constexpr size_t b1 = (size_t)2 * NCH * 1024, images = b1 + bias_bytes(HT, CT), bytes = images + (size_t)NW * IMG;
};
// k_channel_mlp_pair: a ring of NS = 3 chunks, 8 waves; z in four column parts, the output one tile (32 channels) at a time
template <int KS1, int HT, int CT>
struct PairLds {
    static constexpr int NW = 8, NS = 3, ZH = 4, NCH = KS1 + 2 * CT, ZP = 32 * KS1 / ZH + 16, OP = 128 + 16, IMG = 32 * imax(ZP, OP);
    static constexpr size_t b1 = (size_t)NS * NCH * 1024, images = b1 + bias_bytes(HT, CT), bytes = images + (size_t)NW * IMG;
};
// k_channel_mlp_res128: the pack resident, 8 waves; z in four column parts, the output in pieces of OC = 16 channels of all 32 tokens
template <int KS1, int HT, int CT>
struct Res128Lds {
    static constexpr int NW = 8, ZH = 4, NCH = KS1 + 2 * CT, NF = HT * NCH, ZP = 32 * KS1 / ZH + 16, OC = 16, OP = 4 * OC + 16, IMG = 32 * imax(ZP, OP);
    static constexpr size_t b1 = (size_t)NF * 1024, images = b1 + bias_bytes(HT, CT), bytes = images + (size_t)NW * IMG;
};
// k_channel_mlp_wide: z as B fragments (two token tiles x KS1 KB), then two exchange buffers of NW hidden tiles x 4 KB; the output images (32 tokens x 64 channels
// per wave, from offset 0) alias the z fragments and exchange buffer 0, so they add nothing to the total
template <int KS1, int HT, int CT, int NW>
struct WideLds {
    static constexpr int ZBYTES = 2 * KS1 * 1024, XBYTES = NW * 4 * 1024, OP = 256 + 16, IMG = 32 * OP;
    static constexpr size_t xchg = ZBYTES, b1 = (size_t)ZBYTES + 2 * XBYTES, bytes = b1 + bias_bytes(HT, CT);
    static_assert(NW * IMG <= ZBYTES + XBYTES, "the output images alias the z fragments and exchange buffer 0");
};

// The middle of a hidden tile, ONE text for both forms of the step below and for k_channel_mlp_wide, so that they cannot drift apart: h = 2 gelu(D1 + b1) in float32, rounded to bf16 -- with
// D1's accumulator layout already the second product's two B operands.  Declares hb[2]; D1: the first product's accumulators; QUAD: the lane's b1 quad g (units 8 g + 4 h ..), read from LDS on the spot
// (hidden_tile_ring) or requested earlier (hidden_tile_pinned).  A macro, not a function: through a helper the compiler scheduled the kernels that keep
// hidden_tile_ring's form differently from the parent's listing; expanded in place their code is the parent's, instruction for instruction.
// The tile's 16 values go four pairs in lockstep at a time (eight: the kernels at their register limit spill); TWICE the GELU -- W2 is stored halved (ops.pack_channel_mlp).
#define RCX_MLP_HIDDEN_GELU(D1, QUAD)                                                                                                     \
    bf16x8 hb[2];                                                                                                                         \
    gelu_f32x2 gv[8];                                                                                                                     \
    _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                                                       \
        const f32x4q bb = QUAD;                                                                                                           \
        gv[2 * g] = gelu_f32x2{D1[4 * g] + bb.x, D1[4 * g + 1] + bb.y};                                                                   \
        gv[2 * g + 1] = gelu_f32x2{D1[4 * g + 2] + bb.z, D1[4 * g + 3] + bb.w};                                                           \
    }                                                                                                                                     \
    {                                                                                                                                     \
        gelu_f32x2 ga[4] = {gv[0], gv[1], gv[2], gv[3]}, gb[4] = {gv[4], gv[5], gv[6], gv[7]};                                            \
        gelu2x_batch<4>(ga);                                                                                                              \
        gelu2x_batch<4>(gb);                                                                                                              \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) { gv[i] = ga[i]; gv[4 + i] = gb[i]; }                                               \
    }                                                                                                                                     \
    _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                                                       \
        hb[g >> 1][4 * (g & 1) + 0] = (__bf16)gv[2 * g].x; hb[g >> 1][4 * (g & 1) + 1] = (__bf16)gv[2 * g].y;                             \
        hb[g >> 1][4 * (g & 1) + 2] = (__bf16)gv[2 * g + 1].x; hb[g >> 1][4 * (g & 1) + 3] = (__bf16)gv[2 * g + 1].y;                     \
    }

// One 32-unit tile of the hidden layer from its chunk of fragments in LDS (Lc: KS1 W1 fragments, then 2 CT W2 fragments in (ct, q) order):
//   D1 = W1 tile x z^T, h = gelu(D1 + b1) -> bf16 (already the second product's B operand), D2 += W2 columns x h.
// The fragments go through register rings RD deep, requested RD products ahead -- and the second product's first RD before the GELU: a read issued right in
// front of its product costs the LDS latency per product (measured: 13 % of the matrix-core peak whatever the shape).
// AS WRITTEN the compiler does not emit that: its scheduler regroups the requests into batches that each end in a full drain (lgkmcnt(0)) right behind the newest
// request, fetches the four b1 quads one dependent round trip at a time behind the last D1 product, and -- in the kernels at their register limit -- sinks the
// second product's first fragments below the GELU (tools/check_mlp_waits.py counts it in the listing).  This is the form of k_channel_mlp, k_channel_mlp_res128,
// k_channel_mlp_stream and the non-staged path; hidden_tile_pinned below is the same arithmetic with the order pinned.
template <int KS1, int CT, int RD>
__device__ __forceinline__ void hidden_tile_ring(const u32x4q* Lc, const float* b1t, int lane, int h, const bf16x8 (&zb)[KS1], f32x16 (&d2)[CT] RCX_MLP_STAMP_PARM)
{
    constexpr int R1 = KS1 < RD ? KS1 : RD, N2 = 2 * CT, R2 = N2 < RD ? N2 : RD;
    u32x4q ring[RD];
#pragma unroll
    for (int j = 0; j < R1; ++j) ring[j] = Lc[j * 64 + lane];
    RCX_MLP_STAMP(0)
    f32x16 d1;
#pragma unroll
    for (int i = 0; i < 16; ++i) d1[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
        const bf16x8 a = __builtin_bit_cast(bf16x8, ring[ks % R1]);
        if (ks + R1 < KS1) ring[ks % R1] = Lc[(ks + R1) * 64 + lane];
        d1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, zb[ks], d1, 0, 0, 0);
    }
    RCX_MLP_STAMP(1)
    // the second product's fragments in use order: f = q CT + ct  ->  pack slot KS1 + 2 ct + q
#ifndef RCX_MLP_STAMPS                                // (the diagnostic build requests them behind the GELU, where the product build's scheduler puts all but one:
                                                      // fenced in here by the stamps they would spill in the kernels at their register limit)
#pragma unroll
    for (int f = 0; f < R2; ++f) ring[f] = Lc[(KS1 + 2 * (f % CT) + f / CT) * 64 + lane];
#endif
    RCX_MLP_HIDDEN_GELU(d1, *reinterpret_cast<const f32x4q*>(b1t + 8 * g + 4 * h))
#ifdef RCX_MLP_STAMPS
#pragma unroll
    for (int f = 0; f < R2; ++f) ring[f] = Lc[(KS1 + 2 * (f % CT) + f / CT) * 64 + lane];
#endif
    RCX_MLP_STAMP(2)
#pragma unroll
    for (int f = 0; f < N2; ++f) {
        const bf16x8 a = __builtin_bit_cast(bf16x8, ring[f % R2]);
        if (f + R2 < N2) ring[f % R2] = Lc[(KS1 + 2 * ((f + R2) % CT) + (f + R2) / CT) * 64 + lane];
        d2[f % CT] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, hb[f / CT], d2[f % CT], 0, 0, 0);
    }
    RCX_MLP_STAMP(3)
}

// The same tile -- every float32 operation and its order are hidden_tile_ring's, so the result is bit-identical -- with the ORDER of the LDS requests pinned:
// a scheduling barrier behind every product keeps each request where it is written (k_channel_mlp_wide's remedy), and the compiler's own wait insertion then
// counts: LDS reads of a wave return in order, so a product waits for lgkmcnt(requests issued after its fragment's), not for 0.
//   D1     request ks + R1 goes out in front of product ks; the last R1 products have nothing left to request and drain the ring.
//   b1     all four quads are requested together in front of the B1AT-th product from the end of D1 (B1AT <= R1: behind the ring's last request) -- one wait, under
//          D1's last products.
//   W2     its first P2 fragments are requested behind D1's last product, in front of the b1 adds and the GELU; P2 < R2 where the GELU's batch leaves no more
//          registers (the rest of the ring follows right behind the GELU).  Then as D1: R2 ahead, the last R2 products drain.
// PRE2 / B1AT are per kernel: the budget is its registers, and the only guard of that budget is the build's scratch scan (_obj/scratch.ok) -- the values were
// found by compiling, so a compiler that allocates differently may ask for smaller ones.
// Only k_channel_mlp_pair takes this form.  (The resident 128-channel kernel with the ring carried from step to step -- D2's last products requesting the next
// chunk's first W1 fragments, no drain at all -- and k_channel_mlp measured no faster than in hidden_tile_ring's form: profiles/r15_mlp_ring.txt.)
template <int KS1, int CT, int RD, int PRE2, int B1AT>
__device__ __forceinline__ void hidden_tile_pinned(const u32x4q* Lc, const float* b1t, int lane, int h, const bf16x8 (&zb)[KS1], f32x16 (&d2)[CT] RCX_MLP_STAMP_PARM)
{
    constexpr int R1 = KS1 < RD ? KS1 : RD, N2 = 2 * CT, R2 = N2 < RD ? N2 : RD, P2 = PRE2 < R2 ? PRE2 : R2;
    static_assert(B1AT >= 1 && B1AT <= KS1 && P2 >= 1, "b1 is requested inside D1, W2 before the GELU");
    u32x4q ring[RD];
#pragma unroll
    for (int j = 0; j < R1; ++j) ring[j] = Lc[j * 64 + lane];
    RCX_MLP_STAMP(0)
    f32x16 d1;
#pragma unroll
    for (int i = 0; i < 16; ++i) d1[i] = 0.f;
    f32x4q bq[4];
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
        const bf16x8 a = __builtin_bit_cast(bf16x8, ring[ks % R1]);
        if (ks + R1 < KS1) ring[ks % R1] = Lc[(ks + R1) * 64 + lane];
        if (ks == KS1 - B1AT) {
#pragma unroll
            for (int g = 0; g < 4; ++g) bq[g] = *reinterpret_cast<const f32x4q*>(b1t + 8 * g + 4 * h);
        }
        d1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, zb[ks], d1, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    RCX_MLP_STAMP(1)
    // the second product's fragments in use order: f = q CT + ct  ->  pack slot KS1 + 2 ct + q
#pragma unroll
    for (int f = 0; f < P2; ++f) ring[f] = Lc[(KS1 + 2 * (f % CT) + f / CT) * 64 + lane];
    __builtin_amdgcn_sched_barrier(0);
    RCX_MLP_HIDDEN_GELU(d1, bq[g])
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int f = P2; f < R2; ++f) ring[f] = Lc[(KS1 + 2 * (f % CT) + f / CT) * 64 + lane];
    __builtin_amdgcn_sched_barrier(0);                // (without it the scheduler issues these behind D2's first product, in another order, and drains)
    RCX_MLP_STAMP(2)
#pragma unroll
    for (int f = 0; f < N2; ++f) {
        const bf16x8 a = __builtin_bit_cast(bf16x8, ring[f % R2]);
        if (f + R2 < N2) ring[f % R2] = Lc[(KS1 + 2 * ((f + R2) % CT) + (f + R2) / CT) * 64 + lane];
        d2[f % CT] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, hb[f / CT], d2[f % CT], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    RCX_MLP_STAMP(3)
}

// KS1 = ceil(C / 16) k-steps of the first product, HT = H / 32 hidden tiles, CT = ceil(C / 32) output tiles; C % 8 == 0 (a lane's 8 channels of a k-step are
// all there or all padding).  NW waves per workgroup share the LDS weights; each takes every (grid x NW)-th 32-token tile.
// KX / OX: C == 16 KS1 / C == 32 CT exactly -- no padding lanes, so a lane's offsets are one register plus immediates
template <int KS1, int HT, int CT, int NW, int WPS, bool KX, bool OX, bool STAGED>
__global__ void __launch_bounds__(64 * NW, WPS)
k_channel_mlp(const bf16_t* __restrict__ z, const bf16_t* __restrict__ xres, bf16_t* __restrict__ y, const u32x4q* __restrict__ wfrag, const float* __restrict__ bias,
              int M, int C, int ntiles RCX_MLP_STAMP_ARG)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    using L = SmallLds<KS1, HT, CT, NW, STAGED>;
    constexpr int NF = L::NF;
    const u32x4q* const Lf = reinterpret_cast<const u32x4q*>(lds_raw);
    const float* const Lb1 = reinterpret_cast<const float*>(lds_raw + L::b1);
    const float* const Lb2 = Lb1 + 32 * HT;
    {
        u32x4q* Lw = reinterpret_cast<u32x4q*>(lds_raw);
        for (int i = threadIdx.x; i < NF * 64; i += 64 * NW) Lw[i] = wfrag[i];
        float* Lb = reinterpret_cast<float*>(lds_raw + L::b1);
        for (int i = threadIdx.x; i < 32 * (HT + CT); i += 64 * NW) Lb[i] = bias[i];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const unsigned nbytes = (unsigned)M * (unsigned)C * 2u;
    const __amdgpu_buffer_rsrc_t zsrc = token_rows(z, nbytes), xsrc = token_rows(xres, nbytes), ysrc = token_rows(y, nbytes);
    // the lane's part of its offsets: 8 channels of k-step ks (reads of z), 4 channels of output group (ct, g) (reads of x, stores of y); padding: bit 31
    unsigned zk[KS1], oc[CT][4];
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) zk[ks] = KX || 16 * ks + 8 * h < C ? 2u * (16 * ks + 8 * h) : 0x80000000u;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int g = 0; g < 4; ++g) oc[ct][g] = OX || 32 * ct + 8 * g + 4 * h < C ? 2u * (32 * ct + 8 * g + 4 * h) : 0x80000000u;

    RCX_MLP_STAMP_BEGIN
    auto hidden_tile = [&](int ht, const bf16x8 (&zb)[KS1], f32x16 (&d2)[CT]) {
        // (hidden_tile_ring's form: pinned, the 56 x 56 kernel measured 73.0 against 74.5 - 75.0 us, inside its own run-to-run spread -- it is memory-bound)
        hidden_tile_ring<KS1, CT, 4>(Lf + (size_t)ht * (KS1 + 2 * CT) * 64, Lb1 + 32 * ht, lane, h, zb, d2 RCX_MLP_STAMP_PASS);
        RCX_MLP_STAMP_STEP
    };
    const int stride = gridDim.x * NW;
    int tile = blockIdx.x * NW + wave;
    if constexpr (STAGED) {
        // ---- two output tiles or fewer (C <= 64): every global access is a whole-wave contiguous kilobyte, the token-on-lane layouts the products need are made in
        // LDS.  (Reading z / x and writing y a token per lane costs the CU's address path 64 cycles a request -- 32 lines touched, 16 or 8 bytes each: 77 us of the
        // 114 us this kernel took that way at 256 x 64 x 56 x 56, profiles/r05_channel_mlp.txt.)  A wave's tile: 32 tokens = 32 RB contiguous bytes.
        constexpr int ZP = L::ZP, OP = L::OP;                                 // bytes per token row: bf16 z image, float32 output image
        unsigned char* const Lt = lds_raw + L::images + (size_t)wave * L::IMG;
        const unsigned RB = 2u * (unsigned)C;
        unsigned go[KS1], za[KS1], oa[KS1];                                   // request i of a tile: bytes [1024 i + 16 lane, + 16) of it -> token t, byte b of its row
        bool live[KS1];
#pragma unroll
        for (int i = 0; i < KS1; ++i) {
            const unsigned o = 1024u * i + 16u * lane, t = o / RB, bb = o - t * RB;
            live[i] = o < 32u * RB;
            go[i] = live[i] ? o : 0x80000000u;
            za[i] = t * ZP + bb;
            oa[i] = t * OP + 2u * bb;
        }
        u32x4q zq[KS1];
        auto load_z = [&](int t) {
#pragma unroll
            for (int i = 0; i < KS1; ++i) zq[i] = __builtin_bit_cast(u32x4q, __builtin_amdgcn_raw_buffer_load_b128(zsrc, (int)((unsigned)t * 32u * RB + go[i]), 0, 0));
        };
        if (tile < ntiles) load_z(tile);
        for (; tile < ntiles; tile += stride) {
            const unsigned base = (unsigned)tile * 32u * RB;
#pragma unroll
            for (int i = 0; i < KS1; ++i)
                if (live[i]) *reinterpret_cast<u32x4q*>(Lt + za[i]) = zq[i];
            wave_sync();
            bf16x8 zb[KS1];
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) {
                u32x4q v = *reinterpret_cast<const u32x4q*>(Lt + r * ZP + 32 * ks + 16 * h);
                if (!KX && ks == KS1 - 1 && !(16 * ks + 8 * h < C)) v = u32x4q{0u, 0u, 0u, 0u};      // channels past C: whatever the image held last (their weights are zeros, but 0 x NaN is not)
                zb[ks] = __builtin_bit_cast(bf16x8, v);
            }
            wave_sync();
            if (tile + stride < ntiles) load_z(tile + stride);                // the next tile and this tile's residual: in flight during the products
            u32x4q xq[KS1];
#pragma unroll
            for (int i = 0; i < KS1; ++i) xq[i] = __builtin_bit_cast(u32x4q, __builtin_amdgcn_raw_buffer_load_b128(xsrc, (int)(base + go[i]), 0, 0));
            f32x16 d2[CT];
            RCX_MLP_ZERO(d2, CT)
            RCX_MLP_STAMP(5)
#pragma unroll 1
            for (int ht = 0; ht < HT; ++ht) hidden_tile(ht, zb, d2);
            // D2 + b2 (token on the lane) -> the float32 image -> rows
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int g = 0; g < 4; ++g) RCX_MLP_IMAGE_QUAD(d2[ct], Lb2 + 32 * ct + 8 * g + 4 * h, Lt + r * OP + 4 * (32 * ct + 8 * g + 4 * h))
            wave_sync();
#pragma unroll
            for (int i = 0; i < KS1; ++i) {
                if (!live[i]) continue;
                const f32x4q lo = *reinterpret_cast<const f32x4q*>(Lt + oa[i]), hi = *reinterpret_cast<const f32x4q*>(Lt + oa[i] + 16);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4q, rows_plus_x(lo, hi, xq[i])), ysrc, (int)(base + go[i]), 0, 0);
            }
            wave_sync();
        }
        RCX_MLP_STAMP(5)
        RCX_MLP_STAMP_END(blockIdx.x * NW + wave)
        return;
    }
    // ---- three output tiles or more (C = 80, 96): the weights take the LDS the images would need; a token per lane straight from / to memory
    u32x4q zf[KS1];
    auto load_z = [&](int t) {
        const unsigned row = (unsigned)(32 * t + r) * (unsigned)C * 2u;       // (a token past M: past the buffer, reads 0)
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) zf[ks] = __builtin_bit_cast(u32x4q, __builtin_amdgcn_raw_buffer_load_b128(zsrc, (int)(row + zk[ks]), 0, 0));
    };
    if (tile < ntiles) load_z(tile);
    for (; tile < ntiles; tile += stride) {
        const unsigned row = (unsigned)(32 * tile + r) * (unsigned)C * 2u;
        bf16x8 zb[KS1];
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) zb[ks] = __builtin_bit_cast(bf16x8, zf[ks]);
        if (tile + stride < ntiles) load_z(tile + stride);                    // the next tile's channels: in flight during this tile's products
        f32x16 d2[CT];
        RCX_MLP_ZERO(d2, CT)
#pragma unroll 1
        for (int ht = 0; ht < HT; ++ht) hidden_tile(ht, zb, d2);
        u32x2q xr[CT][4];                                                    // the residual (requested after the products: until here its registers are the accumulators')
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) xr[ct][g] = __builtin_bit_cast(u32x2q, __builtin_amdgcn_raw_buffer_load_b64(xsrc, (int)(row + oc[ct][g]), 0, 0));
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4q bb = *reinterpret_cast<const f32x4q*>(Lb2 + 32 * ct + 8 * g + 4 * h);
                const unsigned x0 = xr[ct][g].x, x1 = xr[ct][g].y;
                bf16x4 o;
                o[0] = (__bf16)(d2[ct][4 * g + 0] + bb.x + __uint_as_float(x0 << 16));
                o[1] = (__bf16)(d2[ct][4 * g + 1] + bb.y + __uint_as_float(x0 & 0xffff0000u));
                o[2] = (__bf16)(d2[ct][4 * g + 2] + bb.z + __uint_as_float(x1 << 16));
                o[3] = (__bf16)(d2[ct][4 * g + 3] + bb.w + __uint_as_float(x1 & 0xffff0000u));
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2q, o), ysrc, (int)(row + oc[ct][g]), 0, 0);
            }
    }
}


// ---------------------------------------------------------------------------------------------------------------------------------------------
// The same block for channel counts whose weights do not fit the LDS (C = 256, H = 512: 512 KB): the hidden-tile chunks of the pack (KS1 + 2 CT fragments, 32 KB at
// C = 256) are STREAMED through a two-deep LDS ring while the products of the previous chunk run -- every workgroup walks the same chunks in the same order, so they
// come from the L2.  NW waves per workgroup, 32 tokens each, hold their tokens' channels (B fragments, 4 KS1 registers) and the output accumulators (16 CT) for the
// whole block; one barrier per hidden tile.  With NW = 4 (one wave per SIMD) a wave has 512 registers: the accumulators sit in the AGPRs.
// CT: output tiles rounded up to even (the pack pads W2 / b2 with zero rows); ZH: the z image is staged in ZH column parts (2: 320 channels, whose whole rows would
// not leave room for the ring); ZPF: request the next block's z during this block (off where its registers are needed)
template <int KS1, int HT, int CT, int NW, int WPS, int ZH, bool ZPF>
__global__ void __launch_bounds__(64 * NW, WPS)
k_channel_mlp_stream(const bf16_t* __restrict__ z, const bf16_t* __restrict__ xres, bf16_t* __restrict__ y, const u32x4q* __restrict__ wfrag, const float* __restrict__ bias,
                     int M, int C, int nblocks)
{
    RCX_MLP_STAMP_BEGIN                                                               // (the diagnostic build: never written out for this kernel)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    using L = StreamLds<KS1, HT, CT, NW, ZH>;
    constexpr int NCH = L::NCH, NT = 64 * NW, PER = (NCH * 64 + NT - 1) / NT;                // fragments per chunk; 16-byte pieces of a chunk per thread (the last one ragged)
    constexpr bool RAG = NCH * 64 % NT != 0;
    u32x4q* const Lring = reinterpret_cast<u32x4q*>(lds_raw);                        // [2][NCH * 64]
    float* const Lb1 = reinterpret_cast<float*>(lds_raw + L::b1);
    float* const Lb2 = Lb1 + 32 * HT;
    for (int i = threadIdx.x; i < 32 * (HT + CT); i += NT) Lb1[i] = bias[i];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const unsigned nbytes = (unsigned)M * (unsigned)C * 2u;
    const __amdgpu_buffer_rsrc_t zsrc = token_rows(z, nbytes), xsrc = token_rows(xres, nbytes), ysrc = token_rows(y, nbytes);
    // chunk 0 -> ring slot 0; chunk 1 -> the registers of set 1.  In step ht (chunk ht in slot ht & 1) the requests for chunk ht + 2 go out first and land in
    // register set ht & 1, the products run, then set (ht + 1) & 1 -- chunk ht + 1, requested a whole step earlier -- is written to the other slot: the L2 round
    // trip (1.5 - 2 us under this load, longer than a step's products) has two steps to complete.  The chunk sequence is periodic, so it runs across blocks.
    static_assert(HT % 2 == 0, "the ring alternates two register sets");
    u32x4q cp[2][PER];
    auto request = [&](u32x4q (&dst)[PER], int chunk) {
#pragma unroll
        for (int i = 0; i < PER; ++i)
            if (!RAG || i + 1 < PER || threadIdx.x + i * NT < NCH * 64) dst[i] = wfrag[(size_t)chunk * NCH * 64 + threadIdx.x + i * NT];
    };
    auto deposit = [&](const u32x4q (&src)[PER], int slot) {
        u32x4q* const Ln = Lring + slot * NCH * 64;
#pragma unroll
        for (int i = 0; i < PER; ++i)
            if (!RAG || i + 1 < PER || threadIdx.x + i * NT < NCH * 64) Ln[threadIdx.x + i * NT] = src[i];
    };
    request(cp[0], 0);
    deposit(cp[0], 0);
    request(cp[1], 1 % HT);
    __syncthreads();
    // Global accesses: whole-wave contiguous kilobytes (as the small shapes' STAGED path).  A wave's 32 tokens are 32 RB = 1024 KS1 contiguous bytes: request i =
    // bytes [1024 i + 16 lane, + 16) -> token t, byte bz of its row in the wave's bf16 z image.  The output leaves in halves of 64 channels (two output tiles): a
    // float32 image of 32 x 64, read back as rows -- request j of half hf = the 128-byte pieces [128 hf, + 128) of 8 token rows.
    static_assert(CT % 2 == 0, "output in halves of two tiles");
    static_assert(KS1 % ZH == 0, "column parts of whole k-steps");
    constexpr int RB = 32 * KS1, RBH = RB / ZH, KH = KS1 / ZH, ZP = L::ZP, OP = L::OP, NH = CT / 2;
    unsigned char* const Lt = lds_raw + L::images + (size_t)wave * L::IMG;
    unsigned zo[KS1], za[KS1];                                                  // request i of column part q = i / KH: piece 1024 (i % KH) + 16 lane of that part
#pragma unroll
    for (int i = 0; i < KS1; ++i) {
        const unsigned o = 1024u * (i % KH) + 16u * lane, t = o / RBH, bz = o % RBH;
        zo[i] = t * RB + (i / KH) * RBH + bz;
        za[i] = t * ZP + bz;
    }
    // half hf, request j (4 per half): token t = 8 j + lane / 8, bytes 128 hf + 16 (lane % 8) of its row
    const unsigned ht_tok = lane >> 3, ht_b = 16u * (lane & 7);
    u32x4q zq[KS1];
    auto load_z = [&](int blk) {
        const unsigned base = (unsigned)(32 * (blk * NW + wave)) * (unsigned)RB;      // (tokens past M: past the buffer -- reads 0, stores dropped)
#pragma unroll
        for (int i = 0; i < KS1; ++i) zq[i] = __builtin_bit_cast(u32x4q, __builtin_amdgcn_raw_buffer_load_b128(zsrc, (int)(base + zo[i]), 0, 0));
    };
    if (ZPF && (int)blockIdx.x < nblocks) load_z(blockIdx.x);
    for (int block = blockIdx.x; block < nblocks; block += gridDim.x) {
        const unsigned base = (unsigned)(32 * (block * NW + wave)) * (unsigned)RB;
        if constexpr (!ZPF) load_z(block);
        bf16x8 zb[KS1];
        RCX_MLP_STAGE_Z(za[q * KH + i])
        if (ZPF && block + (int)gridDim.x < nblocks) load_z(block + gridDim.x);    // the next block's channels: in flight during this block
        f32x16 d2[CT];
        RCX_MLP_ZERO(d2, CT)
        u32x4q xq[NH][4];                                                          // the residual: requested in the last step but one
#pragma unroll 1
        for (int ht = 0; ht < HT; ht += 2) {
            request(cp[0], (ht + 2) % HT);
            if (ht == HT - 2) {
#pragma unroll
                for (int hf = 0; hf < NH; ++hf)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        xq[hf][j] = __builtin_bit_cast(u32x4q, __builtin_amdgcn_raw_buffer_load_b128(xsrc, (int)(128u * hf + ht_b < RB ? base + (8u * j + ht_tok) * RB + 128u * hf + ht_b : 0x80000000u), 0, 0));
            }
            hidden_tile_ring<KS1, CT, (NW > 4 || KS1 > 16 ? 4 : 8)>(Lring, Lb1 + 32 * ht, lane, h, zb, d2 RCX_MLP_STAMP_PASS);                               // chunk ht: slot 0
            deposit(cp[1], 1);                                                                                  // chunk ht + 1
            __syncthreads();                      // every wave is done with slot 0; slot 1 is complete
            request(cp[1], (ht + 3) % HT);
            hidden_tile_ring<KS1, CT, (NW > 4 || KS1 > 16 ? 4 : 8)>(Lring + NCH * 64, Lb1 + 32 * (ht + 1), lane, h, zb, d2 RCX_MLP_STAMP_PASS);              // chunk ht + 1: slot 1
            deposit(cp[0], 0);                                                                                  // chunk ht + 2 (the next block's chunk 0 after the last)
            __syncthreads();
        }
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) {
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
                for (int g = 0; g < 4; ++g) RCX_MLP_IMAGE_QUAD(d2[2 * hf + c2], Lb2 + 32 * (2 * hf + c2) + 8 * g + 4 * h, Lt + r * OP + 4 * (32 * c2 + 8 * g + 4 * h))
            wave_sync();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned char* src = Lt + (8 * j + ht_tok) * OP + 2 * ht_b;
                const f32x4q lo = *reinterpret_cast<const f32x4q*>(src), hi = *reinterpret_cast<const f32x4q*>(src + 16);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4q, rows_plus_x(lo, hi, xq[hf][j])), ysrc, (int)(128u * hf + ht_b < RB ? base + (8u * j + ht_tok) * RB + 128u * hf + ht_b : 0x80000000u), 0, 0);   // (a half past the row's channels: dropped)
            }
            wave_sync();
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------------------------------
// C = 256, H = 512 (the 14 x 14 stage of M3 / A3): the streamed block of k_channel_mlp_stream with TWO waves per SIMD.  At 4 waves (128 tokens) a workgroup the
// 1 568 token tiles of batch 256 were 1.53 rounds on 256 CUs, paid as two, and a wave alone on its SIMD left its GELU, fragment waits and barriers exposed between
// its matrix products (profiles/r05_channel_mlp.txt).  Here 8 waves x 32 tokens = 256 tokens a workgroup: one round at batch 256, and one wave's vector work runs
// under its partner's products.  That takes <= 256 registers a wave: d2 (128) + the z fragments (64) + d1, the hidden bf16 values, the fragment ring and the GELU
// batch; so the chunks move global -> LDS by LDS-DMA (no staging registers) and the residual is requested only after the products.  The arithmetic is
// hidden_tile_ring's, so y is bit-identical to k_channel_mlp_stream's.
// LDS: a three-slot ring of chunks (3 x 32 KB), b1 / b2, and per wave a 32-token image of 144-byte rows: z staged in four column parts of 64 channels, the output
// in quarters of one output tile (32 channels).  Ring: chunk ht lands in slot (step % 3) two steps ahead of its use; each step waits for its own chunk's DMAs
// (counted vmcnt: the next chunk's stay in flight), then one barrier -- every wave's pieces have landed and every wave is done with the slot of the step before,
// which then takes the chunk two ahead.  Raw s_barrier: __syncthreads() would wait for the DMAs in flight as well.
template <int KS1, int HT, int CT, bool PIN>
__global__ void __launch_bounds__(512, 2)
k_channel_mlp_pair(const bf16_t* __restrict__ z, const bf16_t* __restrict__ xres, bf16_t* __restrict__ y, const u32x4q* __restrict__ wfrag, const float* __restrict__ bias,
                   int M, int C, int nblocks RCX_MLP_STAMP_ARG)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    using L = PairLds<KS1, HT, CT>;
    constexpr int NW = L::NW, NT = 64 * NW, NS = L::NS, NCH = L::NCH, PER = NCH * 64 / NT;   // PER: 1-KB DMA pieces of a chunk per wave
    static_assert(NCH * 64 % NT == 0 && HT >= 2, "whole pieces per wave");
    constexpr int ZH = L::ZH, RB = 32 * KS1, RBH = RB / ZH, KH = KS1 / ZH, ZP = L::ZP, OP = L::OP;
    static_assert(KS1 % ZH == 0 && RBH == 128, "column parts of 64 channels: a request = 8 token rows of 128 bytes");
    u32x4q* const Lring = reinterpret_cast<u32x4q*>(lds_raw);                        // [NS][NCH * 64]
    float* const Lb1 = reinterpret_cast<float*>(lds_raw + L::b1);
    const float* const Lb2 = Lb1 + 32 * HT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    unsigned char* const Lt = lds_raw + L::images + (size_t)wv * L::IMG;
    // chunk -> ring slot: piece i of wave w = bytes [1024 (8 i + w), + 1024) of the chunk, lane-linear in LDS as in the pack.
    // PIN: the DMA instruction is issued from inline asm (M0 = the piece's LDS address, saved and restored).  The compiler's wait insertion books the builtin as
    // a FLAT access that may touch LDS and, while one is in flight -- here: always, the next chunk's -- turns EVERY wait for an LDS read into lgkmcnt(0): the full
    // drains of hidden_tile_ring's listing.  Out of its sight the waits are counted.  Its vmcnt for the z / x loads only grows stricter by DMAs it does not see
    // (memory operations complete in order), and the ring's own waits are the counted ones below, as before.
    auto fill = [&](int chunk, int slot) {
        const u32x4q* src = wfrag + (size_t)chunk * NCH * 64 + threadIdx.x;
        u32x4q* dst = Lring + (size_t)slot * NCH * 64 + wv * 64;
        if constexpr (PIN) {
            const unsigned l0 = (unsigned)(size_t)(__attribute__((address_space(3))) void*)dst;
            unsigned m0_;
#pragma unroll
            for (int i = 0; i < PER; ++i)
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" : "=&s"(m0_) : "v"(src + i * NT), "s"(l0 + 16u * i * NT) : "memory");
        } else {
#pragma unroll
            for (int i = 0; i < PER; ++i)
                __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(src + i * NT), (__attribute__((address_space(3))) void*)(dst + i * NT), 16, 0, 0);
        }
    };
    constexpr int VM_ALL = 0x70, VM_NEXT = 0x70 | (PER & 15) | ((PER >> 4) << 14);   // s_waitcnt: lgkmcnt(0) with vmcnt(0) / vmcnt(PER)
    fill(0, 0);
    fill(1, 1);
    for (int i = threadIdx.x; i < 32 * (HT + CT); i += NT) Lb1[i] = bias[i];
    const unsigned nbytes = (unsigned)M * (unsigned)C * 2u;
    const __amdgpu_buffer_rsrc_t zsrc = token_rows(z, nbytes), xsrc = token_rows(xres, nbytes), ysrc = token_rows(y, nbytes);
    // z request i of column part q = i / KH: bytes 1024 (i % KH) + 16 lane of that part = token 8 (i % KH) + lane / 8, byte 16 (lane % 8) of its 128 bytes --
    // a lane base plus constants (no per-request address registers: they would be live through the products)
    const unsigned zo0 = (unsigned)(lane >> 3) * RB + 16u * (lane & 7), za0 = (unsigned)(lane >> 3) * ZP + 16u * (lane & 7);
    // output tile ct, request j (2 per tile): token 16 j + lane / 4, bytes 64 ct + 16 (lane % 4) of its row
    const unsigned ot = lane >> 2, ob = 16u * (lane & 3);
    // The two waves of a SIMD leave each barrier in the same phase; at equal priority they would run their first products side by side, then both GELUs with the
    // matrix pipe idle.  One of them at a higher priority takes the pipe first, so the other's first product runs under its GELU and its second product under the
    // other's GELU.  (Waves 0, 3, 5, 6: one of each pair whether the SIMDs take the waves round robin -- pairs w, w + 4 -- or in pairs -- 2 i, 2 i + 1.)
    if (!(__builtin_popcount(wv) & 1)) __builtin_amdgcn_s_setprio(1);
    RCX_MLP_STAMP_BEGIN
    int slot = 0;                                                              // the ring slot of the current step's chunk
    for (int block = blockIdx.x; block < nblocks; block += gridDim.x) {
        const unsigned base = (unsigned)(32 * (block * NW + wave)) * (unsigned)RB;    // (tokens past M: past the buffer -- reads 0, stores dropped)
        const bool more = block + (int)gridDim.x < nblocks;
        bf16x8 zb[KS1];
        {
            u32x4q zq[KS1];
#pragma unroll
            for (int i = 0; i < KS1; ++i)
                zq[i] = __builtin_bit_cast(u32x4q, __builtin_amdgcn_raw_buffer_load_b128(zsrc, (int)(base + zo0 + 8u * RB * (i % KH) + RBH * (i / KH)), 0, 0));
            RCX_MLP_STAGE_Z(za0 + 8 * ZP * i)
        }
        f32x16 d2[CT];
        RCX_MLP_ZERO(d2, CT)
        RCX_MLP_STAMP(5)
#pragma unroll 1
        for (int ht = 0; ht < HT; ++ht) {
            // chunk ht + 1's pieces (requested in the step before) are the only younger ones -- unless that step had no chunk to request
            if (ht + 1 < HT || more) __builtin_amdgcn_s_waitcnt(VM_NEXT);
            else __builtin_amdgcn_s_waitcnt(VM_ALL);
            __builtin_amdgcn_s_barrier();
            if (ht + 2 < HT || more) fill((ht + 2) % HT, slot == 0 ? 2 : slot - 1);   // the chunk two ahead (the next block's first two after the last), into the slot of the step before
            RCX_MLP_STAMP(4)
            if constexpr (PIN) {
                // the registers are the budget: next to d2 (128) and the z fragments (64) the GELU's batch of four pairs leaves room for ONE W2 fragment in
                // flight across it (two: 16 bytes of scratch, four: 48), and the b1 quads go out in front of D1's last three products, when a ring slot is
                // free (four: 8 bytes of scratch).  The chunk of step ht + 1 lands only at the barrier, so the ring starts empty in every step.
                hidden_tile_pinned<KS1, CT, 4, 1, 3>(Lring + (size_t)slot * NCH * 64, Lb1 + 32 * ht, lane, h, zb, d2 RCX_MLP_STAMP_PASS);
            } else
                hidden_tile_ring<KS1, CT, 4>(Lring + (size_t)slot * NCH * 64, Lb1 + 32 * ht, lane, h, zb, d2 RCX_MLP_STAMP_PASS);
            RCX_MLP_STAMP_STEP
            slot = slot == NS - 1 ? 0 : slot + 1;
        }
        u32x4q xq[CT][2];                                                          // the residual: requested after the products (its registers were the z fragments')
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                xq[ct][j] = __builtin_bit_cast(u32x4q, __builtin_amdgcn_raw_buffer_load_b128(xsrc, (int)(base + (16u * j + ot) * RB + 64u * ct + ob), 0, 0));
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
            for (int g = 0; g < 4; ++g) RCX_MLP_IMAGE_QUAD(d2[ct], Lb2 + 32 * ct + 8 * g + 4 * h, Lt + r * OP + 4 * (8 * g + 4 * h))
            wave_sync();
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const unsigned char* src = Lt + (16 * j + ot) * OP + 2 * ob;
                const f32x4q lo = *reinterpret_cast<const f32x4q*>(src), hi = *reinterpret_cast<const f32x4q*>(src + 16);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4q, rows_plus_x(lo, hi, xq[ct][j])), ysrc, (int)(base + (16u * j + ot) * RB + 64u * ct + ob), 0, 0);
            }
            wave_sync();
        }
    }
    RCX_MLP_STAMP(5)
    RCX_MLP_STAMP_END(blockIdx.x * NW + wv)
}


// ---------------------------------------------------------------------------------------------------------------------------------------------
// C = 128, H = 256 (the 28 x 28 stage of M3 / A3 and its Downsample mixer): the whole pack is 128 KB and stays RESIDENT in LDS next to per-wave images of a few
// KB -- k_channel_mlp_pair's column parts: z staged in four parts of 32 channels, the output in pieces of OC = 16 channels of the tile's 32 tokens (a float32
// image of 32 rows, written by every lane).  With no ring there is nothing for a workgroup's waves to meet at: after the prologue (pack -> LDS by
// LDS-DMA, the biases, ONE barrier) each of the 8 waves (two per SIMD) walks its own 32-token tiles, tile t on wave slot t mod (8 gridDim.x), slots wave-major so
// that a last partial round spreads over the CUs a wave each.  The next tile's z is in flight during the current tile; the residual is requested after the
// products (its registers were the z fragments').  The arithmetic is hidden_tile_ring's on the same fragments in the same order, so y is bit-identical to
// k_channel_mlp_stream's.
// Two questions are closed (tools/bench_mlp.py, profiles/r12_channel_mlp128.txt).  Output pieces of 16 / 32 / 64 channels: 56.8 / 57.3 / 60.7 us at batch 256 and
// 15.2 / 17.2 / 18.2 us at batch 16 (the streamed kernel this form replaced: 66.8 and 15.1) -- 16 is no slower than the streamed kernel at any token count of the
// sweep, so there is no threshold.  A raised priority on one wave of each SIMD's pair: 57.2 against 57.3 us, no gain without a barrier to align them.
template <int KS1, int HT, int CT>
__global__ void __launch_bounds__(512, 2)
k_channel_mlp_res128(const bf16_t* __restrict__ z, const bf16_t* __restrict__ xres, bf16_t* __restrict__ y, const u32x4q* __restrict__ wfrag, const float* __restrict__ bias,
                     int M, int ntiles RCX_MLP_STAMP_ARG)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    using L = Res128Lds<KS1, HT, CT>;
    constexpr int NW = L::NW, NT = 64 * NW, NCH = L::NCH, NF = L::NF, PER = NF * 64 / NT;   // PER: 1-KB DMA pieces of the pack per wave
    static_assert(NF * 64 % NT == 0, "whole pieces per wave");
    constexpr int ZH = L::ZH, RB = 32 * KS1, RBH = RB / ZH, KH = KS1 / ZH, ZP = L::ZP;
    static_assert(KS1 % ZH == 0 && RBH == 64, "column parts of 32 channels: a request = 16 token rows of 64 bytes");
    constexpr int OC = L::OC, NP = 32 * CT / OC, OP = L::OP;                     // an output request = 32 token rows of 2 OC bytes = 1 KB
    const u32x4q* const Lf = reinterpret_cast<const u32x4q*>(lds_raw);
    float* const Lb1 = reinterpret_cast<float*>(lds_raw + L::b1);
    const float* const Lb2 = Lb1 + 32 * HT;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned char* const Lt = lds_raw + L::images + (size_t)wv * L::IMG;
    {
        // piece i of wave w = bytes [1024 (8 i + w), + 1024) of the pack, lane-linear in LDS as packed
        const u32x4q* src = wfrag + threadIdx.x;
        u32x4q* dst = reinterpret_cast<u32x4q*>(lds_raw) + wv * 64;
#pragma unroll
        for (int i = 0; i < PER; ++i)
            __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(src + i * NT), (__attribute__((address_space(3))) void*)(dst + i * NT), 16, 0, 0);
        for (int i = threadIdx.x; i < 32 * (HT + CT); i += NT) Lb1[i] = bias[i];
    }
    const unsigned nbytes = (unsigned)M * (unsigned)RB;
    const __amdgpu_buffer_rsrc_t zsrc = token_rows(z, nbytes), xsrc = token_rows(xres, nbytes), ysrc = token_rows(y, nbytes);
    // z request i of column part q = i / KH: token 16 (i % KH) + lane / 4, byte 16 (lane % 4) of its 64 bytes -- a lane base plus constants
    const unsigned zo0 = (unsigned)(lane >> 2) * RB + 16u * (lane & 3), za0 = (unsigned)(lane >> 2) * ZP + 16u * (lane & 3);
    // output request p (a piece of OC channels): token lane / 2, bytes 2 OC p + 16 (lane % 2) of its row
    const unsigned ot = lane / 2, ob = 16u * (lane % 2);
    const int stride = NW * (int)gridDim.x;
    int tile = wv * (int)gridDim.x + (int)blockIdx.x;
    u32x4q zq[KS1];
    auto load_z = [&](int t) {
        const unsigned base = (unsigned)t * 32u * RB;                            // (tokens past M: past the buffer -- reads 0, stores dropped)
#pragma unroll
        for (int i = 0; i < KS1; ++i)
            zq[i] = __builtin_bit_cast(u32x4q, __builtin_amdgcn_raw_buffer_load_b128(zsrc, (int)(base + zo0 + 16u * RB * (i % KH) + RBH * (i / KH)), 0, 0));
    };
    if (tile < ntiles) load_z(tile);
    __builtin_amdgcn_s_waitcnt(0x70);                                            // vmcnt(0) lgkmcnt(0): this wave's pieces of the pack have landed
    __syncthreads();                                                             // the only barrier: a wave without a tile leaves right after it
    RCX_MLP_STAMP_BEGIN
    for (; tile < ntiles; tile += stride) {
        const unsigned base = (unsigned)tile * 32u * RB;
        bf16x8 zb[KS1];
        RCX_MLP_STAGE_Z(za0 + 16 * ZP * i)
        if (tile + stride < ntiles) load_z(tile + stride);                       // the next tile's channels: in flight during this tile
        f32x16 d2[CT];
        RCX_MLP_ZERO(d2, CT)
        RCX_MLP_STAMP(5)
#pragma unroll 1
        for (int ht = 0; ht < HT; ++ht) {
            hidden_tile_ring<KS1, CT, 4>(Lf + (size_t)ht * NCH * 64, Lb1 + 32 * ht, lane, h, zb, d2 RCX_MLP_STAMP_PASS);
            RCX_MLP_STAMP_STEP
        }
        u32x4q xq[NP];                                                           // the residual: requested after the products
#pragma unroll
        for (int p = 0; p < NP; ++p) xq[p] = __builtin_bit_cast(u32x4q, __builtin_amdgcn_raw_buffer_load_b128(xsrc, (int)(base + ot * RB + 2u * OC * p + ob), 0, 0));
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            // D2 + b2 (token on the lane) of the piece's channels -- output tile p / 2, register groups 2 (p % 2) and + 1 -> the float32 image
#pragma unroll
            for (int g = 2 * (p & 1); g < 2 * (p & 1) + 2; ++g) RCX_MLP_IMAGE_QUAD(d2[p >> 1], Lb2 + 32 * (p >> 1) + 8 * g + 4 * h, Lt + r * OP + 4 * (8 * (g & 1) + 4 * h))
            wave_sync();
            const unsigned char* src = Lt + ot * OP + 2 * ob;                    // -> rows: + x, rounded once
            const f32x4q lo = *reinterpret_cast<const f32x4q*>(src), hi = *reinterpret_cast<const f32x4q*>(src + 16);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4q, rows_plus_x(lo, hi, xq[p])), ysrc, (int)(base + ot * RB + 2u * OC * p + ob), 0, 0);
            wave_sync();
        }
    }
    RCX_MLP_STAMP(5)
    RCX_MLP_STAMP_END(wv * (int)gridDim.x + (int)blockIdx.x)
}


// ---------------------------------------------------------------------------------------------------------------------------------------------
// C = 512, H = 1024 (the 7 x 7 stage of M3 / A3): the forms above do not stretch to it.  A wave that owned 32 tokens and all 512 outputs would need 256 accumulator
// registers next to 128 for its z fragments, and at 49 tokens an image a workgroup must pull all 2 MB of weights whatever its size: next to the matrix cores the
// weight delivery is the limit, not HBM.  So the work is split by WEIGHT FRAGMENT, not by token: a workgroup of 8 waves (two per SIMD) owns 64 tokens = two
// 32-token tiles, and every fragment of the pack is read by exactly one of its waves, straight from global memory (the L2) into registers -- a whole-wave
// contiguous kilobyte, requested RD fragments ahead of its use -- and feeds TWO products, one per token tile.  LDS carries only B operands:
//   z, staged once as the first product's B fragments (tile tt, k-step ks: 1 KB lane-linear; 64 KB);
//   the hidden layer, SH = 8 hidden tiles (256 units) per step, in a double-buffered exchange of 2 x 32 KB.
// Step s of HT / SH = 4:
//   phase A  wave w forms D1 of hidden tile SH s + w for both token tiles (2 KS1 = 64 products, A = W1 fragments (ht, ks)), adds b1, takes 2 gelu(.) and writes
//            the bf16 result -- as in hidden_tile_ring already the second product's B operands, (tt, q) 1 KB each -- lane-linearly into exchange buffer s & 1;
//   one barrier (raw s_barrier behind an LDS-only wait: __syncthreads() would drain the fragment requests in flight);
//   phase B  wave w owns output tiles 2 w, 2 w + 1 and adds the step's 8 hidden tiles to d2[2][2] (64 registers): 64 products, A = W2 fragments (ht, 2 w + c2, q).
// Buffer s & 1 is rewritten in phase A of step s + 2, which every wave enters only through the barrier of step s + 1, i.e. after every wave's phase B of step s.
// The arithmetic per element is hidden_tile_ring's (float32 sums in the same k order, the hidden layer rounded once, the output once).
// Epilogue: + b2 -> a float32 image of 32 tokens x 64 channels per wave (aliased onto the z fragments and exchange buffer 0, both dead after the last barrier)
// -> rows: + x, 16-byte stores, 128 contiguous bytes per token.  Tokens past M: buffer descriptors (reads 0, stores dropped).
//
//
// The same form at other widths: NW = CT / 2 waves a workgroup, SH = NW hidden tiles a step.  The step count HT / SH may be odd: step s uses exchange buffer
// (s + HT / SH) & 1, so that the LAST step always uses buffer 1 and buffer 0 is dead behind the last barrier, whatever the parity.
//   C = 512, H = 768 (stage 3 of RecNeXt-T / S / B):                  <32, 24, 16, RD>: three steps of 8 hidden tiles
//   C = 384, H = 768 (stage 2 of S / B; the 7 x 7 stage of M1 / A1):  <24, 24, 12, RD, 6>: six waves (SIMDs 0 and 1 hold two, 2 and 3 one), four steps of 6
// One workgroup a CU in every case (LDS: 134 / 133 / 100.5 KB of 160), i.e. at most two waves a SIMD, 256 registers each: __launch_bounds__'s 2.
template <int KS1, int HT, int CT, int RD, int NW = 8>
__global__ void __launch_bounds__(64 * NW, 2)
k_channel_mlp_wide(const bf16_t* __restrict__ z, const bf16_t* __restrict__ xres, bf16_t* __restrict__ y, const u32x4q* __restrict__ wfrag, const float* __restrict__ bias, int M)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    constexpr int NT = 64 * NW, SH = NW, NST = HT / SH, NCH = KS1 + 2 * CT, NF = KS1 + 4 * SH;              // NF: fragments a wave consumes per step
    static_assert(CT == 2 * NW && NW <= 8 && HT % SH == 0 && NF % RD == 0 && KS1 % RD == 0 && KS1 % 8 == 0, "a hidden tile (phase A) and two output tiles (phase B) per wave");
    constexpr int XP = NST & 1;                                                  // exchange buffer of step s: (s + XP) & 1 -- the last step's is buffer 1
    constexpr int ZR = KS1 / 4, ZU = 8 * ZR / NW;                                // z: ZR requests per group of 8 tokens, 8 groups, ZU requests a wave
    static_assert(8 * ZR % NW == 0, "the z requests divide among the waves");
    using L = WideLds<KS1, HT, CT, NW>;
    constexpr int RB = 32 * KS1, OP = L::OP, XBYTES = L::XBYTES;                 // bytes per token row; the output image's row pitch; an exchange buffer
    u32x4q* const Lz = reinterpret_cast<u32x4q*>(lds_raw);                      // [tt][ks][lane]
    u32x4q* const Lx = reinterpret_cast<u32x4q*>(lds_raw + L::xchg);            // [2][hidden tile of the step][tt][q][lane]
    float* const Lb1 = reinterpret_cast<float*>(lds_raw + L::b1);
    const float* const Lb2 = Lb1 + 32 * HT;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // The wave's fragment stream: step s, i < KS1: W1 (SH s + w, ks = i); then for hidden tile hl = (i - KS1) / 4 of the step the four W2 fragments in use order
    // j = (i - KS1) % 4: output tile c2 = j & 1, k half q = j >> 1 (alternating accumulators).
    auto frag = [&](int s, int i) -> u32x4q {
        const int ht = SH * s + (i < KS1 ? wv : (i - KS1) >> 2);
        const int f = i < KS1 ? i : KS1 + 4 * wv + 2 * ((i - KS1) & 1) + (((i - KS1) >> 1) & 1);
        return wfrag[((size_t)ht * NCH + f) * 64 + lane];
    };
    u32x4q ring[RD];
#pragma unroll
    for (int i = 0; i < RD; ++i) ring[i] = frag(0, i);
    const unsigned nbytes = (unsigned)M * (unsigned)RB;
    const __amdgpu_buffer_rsrc_t zsrc = token_rows(z, nbytes), xsrc = token_rows(xres, nbytes), ysrc = token_rows(y, nbytes);
    const unsigned base = blockIdx.x * 64u * RB;
    {
        // z -> B fragments: token group tg = tokens 8 tg .. 8 tg + 7; its request j = the 16-byte pieces 8 j + lane / 8 of the rows of tokens lane % 8 (128 contiguous
        // bytes per row and request; in LDS the 8 tokens of one piece are 128 contiguous bytes of fragment (tt, ks = piece / 2), lane half piece % 2: conflict-free).
        // The 8 ZR requests go to the waves ZU at a time: 8 waves take a token group each.
        u32x4q zq[ZU];
#pragma unroll
        for (int i = 0; i < ZU; ++i) {
            const int tg = ZU == ZR ? wv : (ZU * wv + i) / ZR, j = ZU == ZR ? i : (ZU * wv + i) % ZR;
            zq[i] = __builtin_bit_cast(u32x4q, __builtin_amdgcn_raw_buffer_load_b128(zsrc, (int)(base + (8u * tg + (lane & 7)) * RB + 16u * (lane >> 3) + 128u * j), 0, 0));
        }
        for (int i = threadIdx.x; i < 32 * (HT + CT); i += NT) Lb1[i] = bias[i];
#pragma unroll
        for (int i = 0; i < ZU; ++i) {
            const int tg = ZU == ZR ? wv : (ZU * wv + i) / ZR, j = ZU == ZR ? i : (ZU * wv + i) % ZR;
            Lz[((tg >> 2) * KS1 + (lane >> 4) + 4 * j) * 64 + ((lane >> 3) & 1) * 32 + 8 * (tg & 3) + (lane & 7)] = zq[i];
        }
    }
    __syncthreads();
    if (!(__builtin_popcount(wv) & 1)) __builtin_amdgcn_s_setprio(1);            // one wave of each SIMD's pair takes the matrix pipe first (k_channel_mlp_pair)
    constexpr int LGKM0 = 0xC07F;                                                // s_waitcnt lgkmcnt(0) alone: vmcnt 63, expcnt 7
    f32x16 d2[2][2];
    RCX_MLP_ZERO(d2[0], 2)
    RCX_MLP_ZERO(d2[1], 2)
    // output request j of token tile tt: token 8 j + lane / 8, bytes 128 w + 16 (lane % 8) of its row
    const unsigned ot = lane >> 3, ob = 16u * (lane & 7);
    u32x4q xq[2][4];
    auto step = [&](int s, auto last_c) {
        constexpr bool LAST = decltype(last_c)::value;
        const int sn = LAST ? 0 : s + 1;
        // ---- phase A
        f32x16 d1[2];
        RCX_MLP_ZERO(d1, 2)
        constexpr int BD = 2;                                                   // k-steps the z fragments are read ahead of their products
        u32x4q zb[BD][2];
#pragma unroll
        for (int k = 0; k < BD; ++k)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) zb[k][tt] = Lz[(tt * KS1 + k) * 64 + lane];
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            const bf16x8 a = __builtin_bit_cast(bf16x8, ring[ks % RD]);
            ring[ks % RD] = frag(s, ks + RD);
            const bf16x8 b0 = __builtin_bit_cast(bf16x8, zb[ks % BD][0]), b1 = __builtin_bit_cast(bf16x8, zb[ks % BD][1]);
            if (ks + BD < KS1) {
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) zb[ks % BD][tt] = Lz[(tt * KS1 + ks + BD) * 64 + lane];
            }
            d1[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b0, d1[0], 0, 0, 0);
            d1[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b1, d1[1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);                                  // the request stays RD fragments ahead: left alone, the scheduler sinks each one to its use
        }
        const float* const b1t = Lb1 + 32 * (SH * s + wv);
        u32x4q* const Lw = Lx + (size_t)((s + XP) & 1) * (XBYTES / 16) + wv * 4 * 64 + lane;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            RCX_MLP_HIDDEN_GELU(d1[tt], *reinterpret_cast<const f32x4q*>(b1t + 8 * g + 4 * h))
            Lw[(2 * tt) * 64] = __builtin_bit_cast(u32x4q, hb[0]);
            Lw[(2 * tt + 1) * 64] = __builtin_bit_cast(u32x4q, hb[1]);
        }
        __builtin_amdgcn_s_waitcnt(LGKM0);
        __builtin_amdgcn_s_barrier();
        // ---- phase B
        if constexpr (LAST) {                                                   // the residual: in flight during the last products (the fragment ring has nothing left to fetch)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    xq[tt][j] = __builtin_bit_cast(u32x4q, __builtin_amdgcn_raw_buffer_load_b128(xsrc, (int)(base + (32u * tt + 8u * j + ot) * RB + 128u * wv + ob), 0, 0));
        }
        const u32x4q* const Lr = Lx + (size_t)((s + XP) & 1) * (XBYTES / 16) + lane;
        u32x4q hq[2][2][2];                                                      // [hl parity][tt][q]
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int q = 0; q < 2; ++q) hq[0][tt][q] = Lr[(2 * tt + q) * 64];
#pragma unroll
        for (int hl = 0; hl < SH; ++hl) {
            if (hl + 1 < SH) {
#pragma unroll
                for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                    for (int q = 0; q < 2; ++q) hq[(hl + 1) & 1][tt][q] = Lr[((hl + 1) * 4 + 2 * tt + q) * 64];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = KS1 + 4 * hl + j, c2 = j & 1, q = j >> 1;
                const bf16x8 a = __builtin_bit_cast(bf16x8, ring[i % RD]);
                if (i + RD < NF) ring[i % RD] = frag(s, i + RD);
                else if (!LAST) ring[i % RD] = frag(sn, i + RD - NF);
                d2[c2][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, hq[hl & 1][0][q]), d2[c2][0], 0, 0, 0);
                d2[c2][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, hq[hl & 1][1][q]), d2[c2][1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
#pragma unroll 1
    for (int s = 0; s < NST - 1; ++s) step(s, std::false_type{});
    step(NST - 1, std::true_type{});
    // ---- epilogue (every wave has passed the last barrier: the z fragments and exchange buffer 0 are dead)
    unsigned char* const Lt = lds_raw + (size_t)wv * L::IMG;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
            for (int g = 0; g < 4; ++g) RCX_MLP_IMAGE_QUAD(d2[c2][tt], Lb2 + 32 * (2 * wv + c2) + 8 * g + 4 * h, Lt + r * OP + 4 * (32 * c2 + 8 * g + 4 * h))
        wave_sync();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned char* src = Lt + (8 * j + ot) * OP + 2 * ob;
            const f32x4q lo = *reinterpret_cast<const f32x4q*>(src), hi = *reinterpret_cast<const f32x4q*>(src + 16);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4q, rows_plus_x(lo, hi, xq[tt][j])), ysrc, (int)(base + (32u * tt + 8u * j + ot) * RB + 128u * wv + ob), 0, 0);
        }
        wave_sync();
    }
}

}  // namespace mlp

// The tile counts of C channels, the one statement of the rule on this side (ops._mlp_tiles is Python's; tests/test_mlp768_cpu.py holds the two together):
// k-steps of the first product; output tiles -- rounded up to even above 128 channels: the streamed kernels write their output in halves of two tiles, W2 / b2
// padded with zero rows
constexpr int mlp_ks1(int C) { return (C + 15) / 16; }
constexpr int mlp_ct(int C) { return C > 128 ? (C + 63) / 64 * 2 : (C + 31) / 32; }

// C % 8 == 0, H % 32 == 0 (the host pads the hidden layer with zero units)
static bool mlp_shape(int C, int H, int* ks1, int* ht, int* ct)
{
    if (C <= 0 || H <= 0 || C % 8 || H % 32) return false;
    *ks1 = mlp_ks1(C); *ht = H / 32; *ct = mlp_ct(C);
    return true;
}

size_t channel_mlp_pack_bytes(int C, int H)
{
    int ks1, ht, ct;
    if (!mlp_shape(C, H, &ks1, &ht, &ct)) return 0;
    return (size_t)(ht * ks1 + ct * 2 * ht) * 1024;
}

// ---- one launcher per kernel form, instantiated per shape <CH channels, HT hidden tiles> by the table below; all of one signature (ncu: the device's compute units)
#define RCX_MLP_LAUNCH_ARGS const void* z, const void* x, void* y, const void* wfrag, const float* bias, int M, int C, int ncu, hipStream_t s
typedef hipError_t (*mlp_launcher)(RCX_MLP_LAUNCH_ARGS);

// C <= 96: the pack resident in LDS, one workgroup per CU
template <int CH, int HT>
static hipError_t launch_mlp(RCX_MLP_LAUNCH_ARGS)
{
    constexpr int KS1 = mlp_ks1(CH), CT = mlp_ct(CH);
    // one workgroup per CU shares the LDS weights: 12 waves (three per SIMD, 168 registers) where the accumulators are two output tiles, else 8 (256 registers)
    constexpr int NW = CT <= 2 ? 12 : 8, WPS = NW / 4;
    constexpr bool STAGED = CT <= 2;
    using L = mlp::SmallLds<KS1, HT, CT, NW, STAGED>;
    static_assert(L::bytes <= 160 * 1024, "weights + the waves' images must fit the LDS");
    if (C != CH) return hipErrorInvalidConfiguration;
    auto kfn = mlp::k_channel_mlp<KS1, HT, CT, NW, WPS, CH == 16 * KS1, CH == 32 * CT, STAGED>;
    RCX_SET_LDS_ONCE(kfn, L::bytes);
    const int ntiles = (M + 31) / 32;
    int grid = ncu;
    if (grid * NW > ntiles) grid = (ntiles + NW - 1) / NW;
    hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(64 * NW), L::bytes, s, (const bf16_t*)z, (const bf16_t*)x, (bf16_t*)y, (const mlp::u32x4q*)wfrag, bias, M, C, ntiles RCX_MLP_STAMP_VAL);
    return hipGetLastError();
}

// the streamed form: 4 waves, 128 tokens a workgroup
template <int CH, int HT, int ZH = 1, bool ZPF = true>
static hipError_t launch_mlp_stream(RCX_MLP_LAUNCH_ARGS)
{
    constexpr int KS1 = mlp_ks1(CH), CT = mlp_ct(CH), NW = 4;
    using L = mlp::StreamLds<KS1, HT, CT, NW, ZH>;
    static_assert(L::bytes <= 160 * 1024, "the ring and the waves' images must fit the LDS");
    static_assert(CH == 16 * KS1, "no padding lanes");
    if (C != CH) return hipErrorInvalidConfiguration;
    auto kfn = mlp::k_channel_mlp_stream<KS1, HT, CT, NW, NW / 4, ZH, ZPF>;
    RCX_SET_LDS_ONCE(kfn, L::bytes);
    const int nblocks = (M + 32 * NW - 1) / (32 * NW);
    const int grid = nblocks < ncu ? nblocks : ncu;
    hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(64 * NW), L::bytes, s, (const bf16_t*)z, (const bf16_t*)x, (bf16_t*)y, (const mlp::u32x4q*)wfrag, bias, M, C, nblocks);
    return hipGetLastError();
}

// the streamed form with 8 waves (two per SIMD), 256 tokens a workgroup
template <int CH, int HT>
static hipError_t launch_mlp_pair(RCX_MLP_LAUNCH_ARGS)
{
    constexpr int KS1 = mlp_ks1(CH), CT = mlp_ct(CH);
    using L = mlp::PairLds<KS1, HT, CT>;
    static_assert(L::bytes <= 160 * 1024, "the ring and the waves' images must fit the LDS");
    static_assert(CH == 16 * KS1, "no padding lanes");
    if (C != CH) return hipErrorInvalidConfiguration;
    auto kfn = mlp::k_channel_mlp_pair<KS1, HT, CT, RCX_MLP_PINNED>;
    RCX_SET_LDS_ONCE(kfn, L::bytes);
    const int nblocks = (M + 32 * L::NW - 1) / (32 * L::NW);
    const int grid = nblocks < ncu ? nblocks : ncu;
    hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(64 * L::NW), L::bytes, s, (const bf16_t*)z, (const bf16_t*)x, (bf16_t*)y, (const mlp::u32x4q*)wfrag, bias, M, C, nblocks RCX_MLP_STAMP_VAL);
    return hipGetLastError();
}

// the pack resident in LDS, 8 free-running waves (two per SIMD) a workgroup, one persistent workgroup per CU
template <int CH, int HT>
static hipError_t launch_mlp_res128(RCX_MLP_LAUNCH_ARGS)
{
    constexpr int KS1 = mlp_ks1(CH), CT = mlp_ct(CH);
    using L = mlp::Res128Lds<KS1, HT, CT>;
    static_assert(L::bytes <= 160 * 1024, "the pack, the biases and the waves' images must fit the LDS");
    static_assert(CH == 16 * KS1, "no padding lanes");
    if (C != CH) return hipErrorInvalidConfiguration;
    auto kfn = mlp::k_channel_mlp_res128<KS1, HT, CT>;
    RCX_SET_LDS_ONCE(kfn, L::bytes);
    const int ntiles = (M + 31) / 32;
    int grid = (ntiles + L::NW - 1) / L::NW;
    if (grid > ncu) grid = ncu;
    hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(64 * L::NW), L::bytes, s, (const bf16_t*)z, (const bf16_t*)x, (bf16_t*)y, (const mlp::u32x4q*)wfrag, bias, M, ntiles RCX_MLP_STAMP_VAL);
    return hipGetLastError();
}

// CT / 2 waves, 64 tokens a workgroup, the weights straight from global memory (ncu: unused, a workgroup per 64 tokens)
template <int CH, int HT>
static hipError_t launch_mlp_wide(RCX_MLP_LAUNCH_ARGS)
{
    constexpr int KS1 = mlp_ks1(CH), CT = mlp_ct(CH), NW = CT / 2;
    using L = mlp::WideLds<KS1, HT, CT, NW>;
    static_assert(L::bytes <= 160 * 1024, "the z fragments, the exchange buffers and the biases must fit the LDS");
    static_assert(CH == 16 * KS1, "no padding lanes");
    if (C != CH) return hipErrorInvalidConfiguration;
    auto kfn = mlp::k_channel_mlp_wide<KS1, HT, CT, 8, NW>;
    RCX_SET_LDS_ONCE(kfn, L::bytes);
    hipLaunchKernelGGL(kfn, dim3((unsigned)((M + 63) / 64)), dim3(64 * NW), L::bytes, s, (const bf16_t*)z, (const bf16_t*)x, (bf16_t*)y, (const mlp::u32x4q*)wfrag, bias, M);
    return hipGetLastError();
}

// ---- THE shapes that have a kernel: C channels, H / 32 hidden tiles, the token count a shape is offered from, its launcher.  channel_mlp_applicable and
// channel_mlp read nothing else (a launcher refuses a C that is not its own, so a row whose two statements of C disagree fails at its first launch, loudly).
struct MlpRow { int C, HT, min_tokens; mlp_launcher launch; };
static constexpr MlpRow MLP_ROWS[] = {
    {256, 16, 1, launch_mlp_pair<256, 16>},                     // M3 / A3 stage 2
    {128, 8, 1, launch_mlp_res128<128, 8>},                     // M3 / A3 stage 1
    // The 7 x 7 stage: a workgroup streams all 2 MB of weights for its 64 tokens, so a few workgroups on a mostly idle chip lose to the library's N-split GEMMs.
    // Measured crossover against the four library launches (tools/bench_mlp.py, profiles/r11_channel_mlp512.txt): none in the sweep -- M = 1 568 / 3 136 / 6 272 /
    // 12 544: 29.3 / 29.8 / 31.3 / 36.5 us fused against 53.1 / 52.7 / 53.7 / 62.6 us, so it lies below 1 024, the token count tests/test_mlp_gpu.py pins as
    // unsupported; hence 2 048, the smallest sweep point above it with margin.
    {512, 32, 2048, launch_mlp_wide<512, 32>},                  // M3 / A3 stage 3
    // C = 512, H = 768 and C = 384, H = 768 likewise, each from the smallest point of its sweep (tools/bench_mlp.py, three runs in one job,
    // profiles/r13_channel_mlp768.txt): no crossover in either -- 4 x 4 planes, M = 512 / 1 024 / 2 048 / 4 096 / 8 192: 23.2-23.6 / 23.9-24.9 / 23.8-26.4 /
    // 25.3-25.6 / 28.5-33.0 us fused against 51.0-53.4 / 51.9-67.8 / 51.0-53.3 / 51.0-52.5 / 49.7-50.6 us for the four library launches; 7 x 7 planes, M = 784 /
    // 1 568 / 3 136 / 6 272 / 12 544: 23.6-23.8 / 23.3-23.4 / 23.8-24.1 / 24.8-27.9 / 27.3-27.9 us against 52.8-54.8 / 50.8-52.5 / 50.9-52.7 / 50.9-53.1 /
    // 51.8-54.2.  Below the sweeps nothing was measured, so nothing is offered there.
    {512, 24, 512, launch_mlp_wide<512, 24>},                   // T / S / B stage 3
    {384, 24, 784, launch_mlp_wide<384, 24>},                   // S / B stage 2, M1 / A1 stage 3
    {192, 12, 1, launch_mlp_stream<192, 12>},                   // M1 stage 2
    {160, 10, 1, launch_mlp_stream<160, 10>},                   // M5 / A5 stage 1
    {320, 20, 1, launch_mlp_stream<320, 20, 2, false>},         // M5 / A5 stage 2: whole z rows would not leave room for the ring, nor the next block's z registers
    {64, 4, 1, launch_mlp<64, 4>},                              // M3 / A3 stage 0 ...
    {56, 4, 1, launch_mlp<56, 4>},                              // ... M2
    {48, 3, 1, launch_mlp<48, 3>},                              // M1 stage 0 ...
    {40, 3, 1, launch_mlp<40, 3>},                              // ... M0
    {96, 6, 1, launch_mlp<96, 6>},
    {80, 5, 1, launch_mlp<80, 5>},
};

// the row of (C, H) if M tokens of it have a kernel: bf16, M C 2 < 2^31 (the kernels' 32-bit byte offsets)
static const MlpRow* mlp_row(int M, int C, int H, int dtype)
{
    if (dtype != 1 || M <= 0 || H <= 0 || H % 32) return nullptr;
    if ((unsigned long long)M * C * 2 >= (1ull << 31)) return nullptr;
    for (const MlpRow& row : MLP_ROWS)
        if (row.C == C && row.HT == H / 32) return M >= row.min_tokens ? &row : nullptr;
    return nullptr;
}

bool channel_mlp_applicable(int M, int C, int H, int dtype) { return mlp_row(M, C, H, dtype) != nullptr; }

hipError_t channel_mlp(const void* z, const void* x, void* y, const void* wfrag, const float* bias, int M, int C, int H, int dtype, hipStream_t s)
{
    const MlpRow* const row = mlp_row(M, C, H, dtype);
    if (!row) return hipErrorInvalidConfiguration;
    static std::atomic<int> cus[RCX_MAX_DEVICES];                     // compute units of each device, asked once
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < RCX_MAX_DEVICES) {
        ncu = cus[dev].load(std::memory_order_relaxed);
        if (ncu <= 0) {
            int v = 0;
            ncu = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0 ? v : 256;
            cus[dev].store(ncu, std::memory_order_relaxed);
        }
    }
    return row->launch(z, x, y, wfrag, bias, M, C, ncu, s);
}

}  // namespace rcx

#ifdef RCX_MLP_STAMPS
// the diagnostic build: this translation unit alone as a shared object (tools/mlp_timeline.py); stamps = [wave slot][8] cycle sums, wave slots as the kernels number them
extern "C" int rcx_mlp_diag_fwd(const void* z, const void* x, void* y, const void* wfrag, const float* bias, int M, int C, int H, void* stamps, void* stream)
{
    rcx::g_stamps = (unsigned long long*)stamps;
    return (int)rcx::channel_mlp(z, x, y, wfrag, bias, M, C, H, 1, (hipStream_t)stream);
}
#endif

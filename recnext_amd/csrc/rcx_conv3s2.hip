// The third conv of the T / S / B stem (lsnet/model/recattn.py:208-223, `RecNextStem`; ConvNorm BN-folded): y = act(conv3x3_s2_p1(x) + b), Cin -> Cout = 32 -> 64 (T)
// and 64 -> 128 (S / B), bf16 inference, act = exact GELU (T, S: depth[0] == 0) or identity (B).  x is what rcx_stem.hip's front launch (conv1 + GELU + conv2 + GELU)
// left in the workspace: the 56 x 56 intermediate is written once and read once.
//   An implicit GEMM on the matrix cores, D (32 out channels x 32 pixels) = sum over (tap, 16-channel group) of W fragment x input fragment, as the second product
//   of k_stem -- but here a wave keeps ITS 32 output channels' 9 Cin / 16 weight fragments in registers for the whole launch (72 / 144 VGPRs), so a product costs one
//   ds_read_b128 (the input fragment) instead of two, and no weights take LDS.  A persistent workgroup of 4 waves walks 8 x 8 tiles of output pixels:
//   x. the tile's 17 x 17 input pixels (zeros outside the plane: the padding) go to LDS in 16-byte pieces, even columns first, then odd ones: a product's 32 lanes
//      read pixels (2 py + dy, 2 px + dx), i.e. consecutive pixels of one parity, and with PIX = 2 Cin + 16 bytes a pixel and a row pitch = 64 (mod 128) bytes each of
//      ds_read_b128's four 16-lane groups lands on 16 different 16-byte slots of the 256-byte bank row (MI355X_MICROARCH.md, LDS table);
//   B. wave w takes output tile mt = w % MT and the pixel halves w / MT, + 4 / MT .. of the tile (Cout = 128: one mt, both halves; Cout = 64: one of each); a half whose
//      four rows lie below the plane is skipped (28 rows = 3.5 tiles);
//   y. + b (-> GELU) -> bf16 -> the wave's own 32 pixel x 32 channel image in LDS -> y, 16 bytes a lane with a pixel's 64 bytes contiguous across four lanes (k_stem's).
// Numerics: float32 accumulation in a fixed order (one accumulator, k-steps in tap-major order, then the bias), exact GELU (rcx_gelu.h).
#include "rcx_common.h"
#include "rcx_launch.h"
#include "rcx_gelu.h"

namespace rcx {
namespace conv3s2 {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4q __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4q __attribute__((ext_vector_type(4)));
typedef unsigned u32x2q __attribute__((ext_vector_type(2)));
constexpr int YIMG = 32 * 64;              // bytes of a wave's output image in LDS
constexpr int R = 17;                      // input pixels a side of an 8 x 8 output tile

constexpr int pix_bytes(int cin) { return 2 * cin + 16; }
constexpr int row_pitch(int cin) { return (R * pix_bytes(cin) + 63) / 128 * 128 + 64; }          // >= 17 pixels, = 64 (mod 128)
constexpr size_t lds_bytes(int cin, int mt) { return (size_t)R * row_pitch(cin) + sizeof(float) * 32 * mt + (size_t)4 * YIMG; }

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// CIN input channels (32 | 64), MT = Cout / 32 output tiles (2 | 4), ACT = GELU after the bias
template <int CIN, int MT, bool ACT>
__global__ void __launch_bounds__(256)
k_conv3s2(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, const u32x4q* __restrict__ wfrag, const float* __restrict__ bias, int N, int H, int W, int HO, int WO,
          int tiles_x, int tiles_y)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    constexpr int KG = CIN / 16, KS = 9 * KG, PIX = pix_bytes(CIN), RP = row_pitch(CIN), PP = CIN / 8, NP = R * R * PP, XN = (NP + 255) / 256, CO = 32 * MT;
    static_assert(MT == 2 || MT == 4, "a workgroup's four waves cover MT output tiles x two pixel halves");
    unsigned char* const Lt = lds_raw;                                                // input tile [17 rows][9 even columns, 8 odd ones][PIX]
    float* const Lb = reinterpret_cast<float*>(lds_raw + (size_t)R * RP);             // [32 MT]
    unsigned char* const Ly = reinterpret_cast<unsigned char*>(Lb + 32 * MT) + (size_t)(threadIdx.x >> 6) * YIMG;
    for (int i = threadIdx.x; i < 32 * MT; i += 256) Lb[i] = bias[i];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int mt = wave % MT, nt0 = wave / MT;
    u32x4q wr[KS];                                                                    // this wave's weights: fragment (mt, ks), ks = tap KG + cg (ops.pack_stem3)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wr[ks] = wfrag[(size_t)(mt * KS + ks) * 64 + lane];
    const int ntiles = N * tiles_x * tiles_y;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int n = tile / (tiles_x * tiles_y), tr = tile - n * tiles_x * tiles_y, ty = tr / tiles_x, tx = tr - ty * tiles_x;
        // ---- x. piece e of the tile = (pixel e / PP = (i, j), 16-byte piece e % PP): input pixel (16 ty - 1 + i, 16 tx - 1 + j)
        const bf16_t* const xn = x + (size_t)n * H * W * CIN;
        // (in two rounds: the pieces in flight share the registers with the wave's weights)
        constexpr int XH = (XN + 1) / 2;
#pragma unroll
        for (int u0 = 0; u0 < XN; u0 += XH) {
            u32x4q xq[XH];
#pragma unroll
            for (int v = 0; v < XH; ++v) {
                const int e = threadIdx.x + 256 * (u0 + v), p = e / PP, pc = e - p * PP, i = p / R, j = p - i * R, yy = 16 * ty - 1 + i, xx = 16 * tx - 1 + j;
                const bool ok = u0 + v < XN && e < NP && yy >= 0 && yy < H && xx >= 0 && xx < W;
                xq[v] = ok ? *reinterpret_cast<const u32x4q*>(xn + ((size_t)yy * W + xx) * CIN + 8 * pc) : u32x4q{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int v = 0; v < XH; ++v) {
                const int e = threadIdx.x + 256 * (u0 + v), p = e / PP, pc = e - p * PP, i = p / R, j = p - i * R;
                if (u0 + v < XN && e < NP) *reinterpret_cast<u32x4q*>(Lt + i * RP + ((j & 1) * 9 + (j >> 1)) * PIX + 16 * pc) = xq[v];
            }
        }
        __syncthreads();
        // ---- B. pixel q of the 8 x 8 tile = (q / 8, q % 8); tap (dy, dx) of it is tile pixel (2 py + dy, 2 px + dx): column slot px, 9 + px, px + 1 for dx = 0, 1, 2
        for (int nt = nt0; nt < 2; nt += 4 / MT) {
            if (8 * ty + 4 * nt >= HO) continue;                                      // (wave-uniform)
            const int q = 32 * nt + r, py = q >> 3, px = q & 7;
            const unsigned char* const hp = Lt + (2 * py) * RP + px * PIX + 16 * h;
            f32x16 d;
#pragma unroll
            for (int i = 0; i < 16; ++i) d[i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int t = ks / KG, cg = ks - t * KG, dy = t / 3, dx = t - 3 * dy, slot = dx == 1 ? 9 : (dx == 2 ? 1 : 0);
                const bf16x8 b = *reinterpret_cast<const bf16x8*>(hp + dy * RP + slot * PIX + 32 * cg);
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wr[ks]), b, d, 0, 0, 0);
            }
            // ---- y. register 4 g + i of the product = channel 32 mt + 8 g + 4 h + i of pixel r; the image's 8-byte pieces XOR-ed with (r >> 1) & 7 as in k_stem
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4q bb = *reinterpret_cast<const f32x4q*>(Lb + 32 * mt + 8 * g + 4 * h);
                gelu_f32x2 a = {d[4 * g + 0] + bb.x, d[4 * g + 1] + bb.y}, b = {d[4 * g + 2] + bb.z, d[4 * g + 3] + bb.w};
                if constexpr (ACT) { a = gelu2(a); b = gelu2(b); }
                bf16x4 o;
                o[0] = (__bf16)a.x; o[1] = (__bf16)a.y; o[2] = (__bf16)b.x; o[3] = (__bf16)b.y;
                *reinterpret_cast<u32x2q*>(Ly + 64 * r + 8 * ((2 * g + h) ^ ((r >> 1) & 7))) = __builtin_bit_cast(u32x2q, o);
            }
            wave_sync();
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int ql = 16 * it + (lane >> 2), ck = lane & 3, sw = (ql >> 1) & 7, q2 = 32 * nt + ql, oy = 8 * ty + (q2 >> 3), ox = 8 * tx + (q2 & 7), c0 = 32 * mt + 8 * ck;
                const u32x2q lo = *reinterpret_cast<const u32x2q*>(Ly + 64 * ql + 8 * ((2 * ck) ^ sw)), hi = *reinterpret_cast<const u32x2q*>(Ly + 64 * ql + 8 * ((2 * ck + 1) ^ sw));
                if (oy < HO && ox < WO) *reinterpret_cast<u32x4q*>(y + ((size_t)(n * HO + oy) * WO + ox) * CO + c0) = u32x4q{lo.x, lo.y, hi.x, hi.y};
            }
            wave_sync();                                   // (the wave's next half writes the image again)
        }
        __syncthreads();                                   // every wave has left the tile before the next one's pieces land
    }
}

template <int CIN, int MT, bool ACT>
static hipError_t launch(const void* x, void* y, const void* wfrag, const float* bias, int N, int H, int W, int ncu, hipStream_t s)
{
    const int HO = (H + 1) / 2, WO = (W + 1) / 2, tx = (WO + 7) / 8, ty = (HO + 7) / 8;
    constexpr size_t lds = lds_bytes(CIN, MT);
    const long long ntiles = (long long)N * tx * ty;
    if (ntiles > 0x7fffffffLL || (long long)N * HO * WO > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    constexpr long long per_cu = CIN > 32 ? 2 : 3;                                    // what the registers allow (the weights are 144 / 72 of them)
    const long long grid = ntiles < ncu * per_cu ? ntiles : ncu * per_cu;             // persistent: the weights go to registers once per wave
    auto kfn = k_conv3s2<CIN, MT, ACT>;
    RCX_SET_LDS_ONCE(kfn, lds);
    hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(256), lds, s, (const bf16_t*)x, (bf16_t*)y, (const u32x4q*)wfrag, bias, N, H, W, HO, WO, tx, ty);
    return hipGetLastError();
}

}  // namespace conv3s2

// x: N x H x W x Cin (the front launch's output), y: N x ceil(H/2) x ceil(W/2) x Cout, both 16-byte aligned; (Cin, Cout) = (32, 64) | (64, 128)
hipError_t conv3s2_fwd(const void* x, void* y, const void* wfrag, const float* bias, int N, int H, int W, int CIN, int act, hipStream_t s)
{
    if (N <= 0 || H <= 0 || W <= 0) return hipErrorInvalidConfiguration;
    const int ncu = stem_device_cus();
    if (CIN == 32) return act ? conv3s2::launch<32, 2, true>(x, y, wfrag, bias, N, H, W, ncu, s) : conv3s2::launch<32, 2, false>(x, y, wfrag, bias, N, H, W, ncu, s);
    if (CIN == 64) return act ? conv3s2::launch<64, 4, true>(x, y, wfrag, bias, N, H, W, ncu, s) : conv3s2::launch<64, 4, false>(x, y, wfrag, bias, N, H, W, ncu, s);
    return hipErrorInvalidConfiguration;
}

}  // namespace rcx

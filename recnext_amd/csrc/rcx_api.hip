// C ABI of librecnext_amd.so (include/recnext_amd.h): argument checking, schedule selection,
// error reporting.  No allocation, no synchronisation, no retained pointers.
#include "../../include/recnext_amd.h"
#include "rcx_opts.h"
#include "rcx_launch.h"

#include <cstdarg>
#include <initializer_list>
#include <cstdio>
#include <cstdlib>

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char* what, const char* prefix = "")
{
    snprintf(g_err, sizeof(g_err), "%s%s: %s", prefix, what, hipGetErrorString(e));
    return (int)e;
}

inline bool known_dtype(int d) { return d == RCX_DTYPE_F32 || d == RCX_DTYPE_BF16 || d == RCX_DTYPE_F16; }
inline int down_size(int h, int k) { const int p = k / 2; return (h + 2 * p - k) / 2 + 1; }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Ladder {
    int h[RCX_MAX_LEVEL + 1], w[RCX_MAX_LEVEL + 1];
    size_t f_off[RCX_MAX_LEVEL + 1];   // workspace offsets of F_1..F_level (float)
    size_t c_off[2];                   // two ping-pong conv-output buffers (float), each sized for level 1
    size_t total;
};

Ladder make_ladder(int N, int C, int H, int W, int level, int k)
{
    Ladder L{};
    L.h[0] = H; L.w[0] = W;
    size_t off = 0;
    for (int l = 1; l <= level; ++l) {
        L.h[l] = down_size(L.h[l - 1], k);
        L.w[l] = down_size(L.w[l - 1], k);
        L.f_off[l] = off;
        off += align256(sizeof(float) * (size_t)N * C * L.h[l] * L.w[l]);
    }
    const size_t c1 = level >= 1 ? align256(sizeof(float) * (size_t)N * C * L.h[1] * L.w[1]) : 0;
    const size_t c2 = level >= 2 ? align256(sizeof(float) * (size_t)N * C * L.h[2] * L.w[2]) : 0;
    L.c_off[0] = off; off += c1;       // holds C_1, C_3, ...
    L.c_off[1] = off; off += c2;       // holds C_2, C_4, ...
    L.total = off;
    return L;
}

int check_common(const void* x, const void* y, int N, int C, int H, int W, int k, int dtype)
{
    if (!x || !y) return fail(RCX_ERR_BAD_ARG, "null activation pointer");
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(RCX_ERR_BAD_ARG, "non-positive extent N=%d C=%d H=%d W=%d", N, C, H, W);
    if (k <= 0 || (k & 1) == 0) return fail(RCX_ERR_BAD_ARG, "kernel_size must be odd and positive, got %d", k);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    return 0;
}

// RCX_FORCE_GENERIC=1 (rcx::opt::hand_kernels_off) pins the one-launch-per-ladder-step generic schedule: tests cover both with it.
bool use_plane(int N, int C, int H, int W, int level, int k, int dtype)
{
    return !rcx::opt::hand_kernels_off() && rcx::plane_applicable(N, C, H, W, level, k, dtype);
}

// Split schedule for a plane whose level-1 plane does not fit the register file (128x128 / level 4): three launches,
//   F_1 = down(x) (step kernel, float32) ; C_1 = RecConv2d_{level-1}(F_1) with the first level+1 packs (register-resident) ;
//   y = conv_L(x + resize(C_1)) (step kernel).  F_1 and C_1 live in the caller's workspace.
bool use_split(int N, int C, int H, int W, int level, int k, int dtype)
{
    if (rcx::opt::hand_kernels_off() || level < 1 || k != 5 || H != W || (H & 1)) return false;
    if (H < 64) return false;                            // small planes: the fused LDS-pyramid kernel (or the nested schedule) decides
    if (rcx::lanes_applicable(N, C, H, W, level, k, dtype)) return false;
    return rcx::down5_lanes_applicable(N, C, H, W, k, 2, dtype, RCX_DTYPE_F32) &&
           rcx::lanes_applicable(N, C, H / 2, W / 2, level - 1, k, RCX_DTYPE_F32) &&
           rcx::upadd_lanes_applicable(N, C, H, W, H / 2, W / 2, k, dtype, RCX_DTYPE_F32, dtype);
}

size_t split_bytes(int N, int C, int H, int W) { return 2 * align256(sizeof(float) * (size_t)N * C * (H / 2) * (W / 2)); }

// the register-resident schedule takes precedence where it applies
bool use_lanes(int N, int C, int H, int W, int level, int k, int dtype)
{
    return !rcx::opt::hand_kernels_off() && rcx::lanes_applicable(N, C, H, W, level, k, dtype);
}

// one ladder rung / one up-recursion step: the register-resident kernel where it applies, else the generic one
// RCX_UPADD_CPT=all: the tiled single-step kernels (rcx_upcpt.hip) also where the lanes kernels keep a ragged channel count (tests)
bool upcpt_everywhere() { return rcx::opt::str(rcx::opt::UPADD_CPT)[0] == 'a'; }

// Which single-step kernel a plane gets.  Never a function of N: a batch and its shards must give the same rows bit for bit.
enum StepKernel { STEP_GENERIC, STEP_LANES, STEP_CPT, STEP_CPL14, STEP_CONV5_LANES };

// stride-2 conv5 (stride 1: the plain conv5): the register-resident lanes kernel where it has a plan (the 7 * 2^k / 16 * 2^k squares: it
// already runs at the copy ceiling on 56 x 56 / 28 x 28, 256 x 64 x 56 x 56 24.7 us against 26.1), the tiled channel-per-lane kernel
// (rcx_upcpt.hip) on every other even plane whose width is a multiple of 14 (112 x 112: 15.1 us against 50.8; 200 x 336: 84.8 against 218)
// and on the 16 * 2^k squares in bfloat16 (16-wide tiles: 32 x 64 x 128 x 128 22.4 us against the lanes kernel's 39.9, 32 x 256 x 32 x 32
// 12.1 against 16.2, 64 x 64 16.2 / 16.6).
StepKernel pick_dwconv(int N, int C, int H, int W, int k, int stride, int in_dt, int out_dt)
{
    if (rcx::opt::hand_kernels_off()) return STEP_GENERIC;
    if (rcx::down5_cpl7_applicable(N, C, H, W, k, stride, in_dt, out_dt)) return STEP_CPL14;          // the 7 x 7 plane, whole (round 4)
    const bool lanes_ok = rcx::down5_lanes_applicable(N, C, H, W, k, stride, in_dt, out_dt);
    if (lanes_ok && !upcpt_everywhere() && !(W % 14 != 0 && C % 64 == 0)) return STEP_LANES;
    if (rcx::down5_cpt_applicable(N, C, H, W, k, stride, in_dt, out_dt)) return STEP_CPT;
    if (lanes_ok) return STEP_LANES;
    if (stride == 1 && rcx::conv5_lanes_applicable(N, C, H, W, k, in_dt, out_dt)) return STEP_CONV5_LANES;
    return STEP_GENERIC;
}

// conv5(x + resize(coarse)): the whole-plane kernel on 14 x 14; the tiled channel-per-lane kernel (rcx_upcpt.hip) for whole 64-channel
// waves (256 x 64 x 56 x 56: 61 - 63 us against the lanes kernel's 74 - 76) and wherever the lanes kernel has no plan (float16, planes that
// are not 7 * 2^k / 16 * 2^k squares: 32 x 64 x 200 x 336 168 - 176 us against the generic kernel's 860 - 1 413); ragged channel counts on a
// lanes plane stay with the lanes kernel (256 x 96 x 28 x 28: 24 - 26 us against 28 - 52), and so do 16-wide tiles on a plane lower than
// 64 rows, whose third tile row is mostly empty (32 x 256 x 32 x 32: 20 us against 14; 64 x 64: 31 against 35; 128 x 128: 47 - 52 against 85 - 91).
StepKernel pick_upadd(int N, int C, int H, int W, int Hc, int Wc, int k, int x_dt, int c_dt, int out_dt, bool has_coarse)
{
    if (rcx::opt::hand_kernels_off()) return STEP_GENERIC;
    if (!has_coarse) return rcx::conv5_lanes_applicable(N, C, H, W, k, x_dt, out_dt) ? STEP_CONV5_LANES : STEP_GENERIC;
    if (rcx::upadd_cpl14_applicable(N, C, H, W, Hc, Wc, k, x_dt, c_dt, out_dt)) return STEP_CPL14;
    const bool lanes_ok = rcx::upadd_lanes_applicable(N, C, H, W, Hc, Wc, k, x_dt, c_dt, out_dt);
    const bool whole = C % 64 == 0 && !(W % 14 != 0 && H < 64);
    if ((whole || !lanes_ok || upcpt_everywhere()) && rcx::upadd_cpt_applicable(N, C, H, W, Hc, Wc, k, x_dt, c_dt, out_dt)) return STEP_CPT;
    return lanes_ok ? STEP_LANES : STEP_GENERIC;
}

// Nested schedule for a plane no fused kernel takes (COCO stages, 112 x 112, ...): the split schedule made recursive,
//   F_1 = conv5 stride 2 (x) (float32, workspace) ; C_1 = RecConv2d_{level-1}(F_1) by WHATEVER schedule that block has -- a fused kernel
//   (lanes / LDS pyramid), or this schedule again -- ; y = conv5(x + resize(C_1)),
// both outer steps on single-step kernels (rcx_upcpt.hip / the lanes step kernels).  200 x 336 / level 4: five launches (two down, the
// LDS-pyramid kernel on 50 x 84 / level 2, two up) instead of the generic ladder's nine.  It only ever replaces the generic ladder.
enum FwdSchedule { FWD_LANES, FWD_SPLIT, FWD_PLANE, FWD_NESTED, FWD_GENERIC };
FwdSchedule fwd_schedule(int N, int C, int H, int W, int level, int k, int dtype);

// (reached only where no fused schedule applies: fwd_schedule tries them first)
bool use_nested(int N, int C, int H, int W, int level, int k, int dtype)
{
    if (rcx::opt::hand_kernels_off() || rcx::opt::off(rcx::opt::NESTED) || level < 1 || k != 5 || (H & 1) || (W & 1)) return false;
    const StepKernel d = pick_dwconv(N, C, H, W, k, 2, dtype, RCX_DTYPE_F32);
    const StepKernel u = pick_upadd(N, C, H, W, H / 2, W / 2, k, dtype, RCX_DTYPE_F32, dtype, true);
    if (d == STEP_GENERIC || u == STEP_GENERIC) return false;
    return fwd_schedule(N, C, H / 2, W / 2, level - 1, k, RCX_DTYPE_F32) != FWD_GENERIC;
}

// The forward schedule of a RecConv2d block, in order of precedence.  The plan string, the workspace size and the launch all switch on it.
FwdSchedule fwd_schedule(int N, int C, int H, int W, int level, int k, int dtype)
{
    if (use_lanes(N, C, H, W, level, k, dtype)) return FWD_LANES;
    if (use_split(N, C, H, W, level, k, dtype)) return FWD_SPLIT;
    if (use_plane(N, C, H, W, level, k, dtype)) return FWD_PLANE;
    if (use_nested(N, C, H, W, level, k, dtype)) return FWD_NESTED;
    return FWD_GENERIC;
}

size_t nested_own_bytes(int N, int C, int H, int W) { return 2 * align256(sizeof(float) * (size_t)N * C * (H / 2) * (W / 2)); }

hipError_t step_dwconv(const void* x, void* y, const float* w, const float* b, int N, int C, int H, int W, int k, int stride,
                       int in_dt, int out_dt, hipStream_t s)
{
    switch (pick_dwconv(N, C, H, W, k, stride, in_dt, out_dt)) {
    case STEP_CPL14: return rcx::down5_cpl7(x, y, w, b, N, C, H, in_dt, s);
    case STEP_LANES: return rcx::down5_lanes(x, y, w, b, N, C, H, W, in_dt, out_dt, s);
    case STEP_CPT: return rcx::down5_cpt(x, y, w, b, N, C, H, W, in_dt, out_dt, s);
    case STEP_CONV5_LANES: return rcx::conv5_lanes(x, y, w, b, N, C, H, W, in_dt, s);
    default: return rcx::generic_dwconv(x, y, w, b, N, C, H, W, k, stride, in_dt, out_dt, s);
    }
}

hipError_t step_upadd(const void* x, const void* coarse, void* y, const float* w, const float* b, int N, int C, int H, int W,
                      int Hc, int Wc, int k, int mode, int x_dt, int c_dt, int out_dt, hipStream_t s)
{
    switch (pick_upadd(N, C, H, W, Hc, Wc, k, x_dt, c_dt, out_dt, coarse != nullptr)) {
    case STEP_CPL14: return rcx::upadd_cpl14(x, coarse, y, w, b, N, C, H, mode, x_dt, c_dt, s);
    case STEP_CPT: return rcx::upadd_cpt(x, coarse, y, w, b, N, C, H, W, mode, x_dt, c_dt, s);
    case STEP_LANES: return rcx::upadd_lanes(x, coarse, y, w, b, N, C, H, W, mode, x_dt, c_dt, s);
    case STEP_CONV5_LANES: return rcx::conv5_lanes(x, y, w, b, N, C, H, W, x_dt, s);
    default: return rcx::generic_upadd_dwconv(x, coarse, y, w, b, N, C, H, W, Hc, Wc, k, mode, x_dt, c_dt, out_dt, s);
    }
}

// The per-step schedule, one launch per ladder step on the best single-step kernel each plane has: the down ladder F_l = down(F_{l-1}), F_0 = x
// (model/recnext.py:27-29), the up recursion C_l = conv_j(F_l + resize(C_{l+1})) coarsest first (:31-33), the final conv (:34).  F_l and C_l
// (l >= 1) are float32 planes of h[l] x w[l] at base + f_off[l] / base + c_off[l]; `prefix` starts the error messages.
int recconv2d_steps(const void* x, void* y, const float* wpack, const float* bpack, char* base, const size_t* f_off, const size_t* c_off,
                    const int* h, const int* w, int N, int C, int level, int k, int mode, int dtype, hipStream_t s, const char* prefix)
{
    const size_t wsz = (size_t)k * k * C;
    auto W_ = [&](int i) { return wpack + (size_t)i * wsz; };                       // 0 = down, 1+j = convs[j]
    auto B_ = [&](int i) { return bpack ? bpack + (size_t)i * C : nullptr; };
    auto F_ = [&](int l) { return (float*)(base + f_off[l]); };
    auto C_ = [&](int l) { return (float*)(base + c_off[l]); };
    hipError_t e;
    for (int l = 1; l <= level; ++l) {
        e = step_dwconv(l == 1 ? x : (const void*)F_(l - 1), F_(l), W_(0), B_(0), N, C, h[l - 1], w[l - 1], k, 2,
                        l == 1 ? dtype : RCX_DTYPE_F32, RCX_DTYPE_F32, s);
        if (e != hipSuccess) return hip_fail(e, "down ladder", prefix);
    }
    for (int l = level, j = 0; l >= 1; --l, ++j) {
        e = step_upadd(F_(l), l == level ? nullptr : C_(l + 1), C_(l), W_(1 + j), B_(1 + j), N, C, h[l], w[l],
                       l == level ? 0 : h[l + 1], l == level ? 0 : w[l + 1], k, mode, RCX_DTYPE_F32, RCX_DTYPE_F32, RCX_DTYPE_F32, s);
        if (e != hipSuccess) return hip_fail(e, "up recursion", prefix);
    }
    e = step_upadd(x, level >= 1 ? C_(1) : nullptr, y, W_(1 + level), B_(1 + level), N, C, h[0], w[0],
                   level >= 1 ? h[1] : 0, level >= 1 ? w[1] : 0, k, mode, dtype, RCX_DTYPE_F32, dtype, s);
    return e == hipSuccess ? 0 : hip_fail(e, "final conv", prefix);
}

}  // namespace

extern "C" {

int rcx_abi_version(void) { return RCX_ABI_VERSION; }

void rcx_reload_options(void) { rcx::opt::reload(); }

int rcx_selftest_d16(const void* src, void* flag, void* stream)
{
    if (!src || !flag) return fail(RCX_ERR_BAD_ARG, "rcx_selftest_d16: null pointer");
    hipError_t e = rcx::selftest_d16(src, flag, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_selftest_d16");
}

const char* rcx_last_error(void) { return g_err; }

const char* rcx_recconv2d_fwd_plan(int N, int C, int H, int W, int level, int k, int mode, int dtype)
{
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || level < 0 || level > RCX_MAX_LEVEL || k <= 0 || (k & 1) == 0) return "invalid";
    static thread_local char desc[256];
    const int md = mode == RCX_MODE_NEAREST ? 1 : 0;
    const FwdSchedule sch = fwd_schedule(N, C, H, W, level, k, dtype);
    if (sch == FWD_SPLIT || sch == FWD_NESTED) {
        char inner[192];
        if (sch == FWD_SPLIT) rcx::lanes_describe(N, C, H / 2, W / 2, level - 1, k, md, RCX_DTYPE_F32, inner, (int)sizeof(inner));
        else snprintf(inner, sizeof(inner), "%s", rcx_recconv2d_fwd_plan(N, C, H / 2, W / 2, level - 1, k, mode, RCX_DTYPE_F32));   // (overwrites desc)
        const bool dcpt = pick_dwconv(N, C, H, W, k, 2, dtype, RCX_DTYPE_F32) == STEP_CPT;
        const bool ucpt = pick_upadd(N, C, H, W, H / 2, W / 2, k, dtype, RCX_DTYPE_F32, dtype, true) == STEP_CPT;
        snprintf(desc, sizeof(desc), "%s(%s + %s + %s)", sch == FWD_SPLIT ? "split" : "nested", dcpt ? "k_down5_cpt" : "k_down5_lanes", inner,
                 ucpt ? "k_upadd_cpt" : "k_upadd_lanes");
        return desc;
    }
    if (sch == FWD_LANES) rcx::lanes_describe(N, C, H, W, level, k, md, dtype, desc, (int)sizeof(desc));
    else if (sch == FWD_PLANE) rcx::plane_describe(N, C, H, W, level, k, dtype, desc, (int)sizeof(desc));
    else return "generic";
    return desc;
}

int rcx_pack_dw_weight(const void* w_ckk, float* dst_kkc, int C, int k, int dtype, void* stream)
{
    if (!w_ckk || !dst_kkc || C <= 0 || k <= 0) return fail(RCX_ERR_BAD_ARG, "rcx_pack_dw_weight: bad argument");
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    hipError_t e = rcx::pack_dw_weight(w_ckk, dst_kkc, C, k, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_pack_dw_weight");
}

int rcx_pack_recconv_params(const void* const* w, const void* const* b, float* wpack, float* wpack_flipped, float* bpack,
                            int count, int C, int k, int dtype, void* stream)
{
    if (!w || !wpack || count <= 0 || count > RCX_MAX_LEVEL + 2 || C <= 0 || k <= 0) return fail(RCX_ERR_BAD_ARG, "rcx_pack_recconv_params: bad argument");
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    if (bpack && !b) return fail(RCX_ERR_BAD_ARG, "rcx_pack_recconv_params: bias destination without bias sources");
    rcx::PackPtrs P{};
    for (int j = 0; j < count; ++j) {
        if (!w[j]) return fail(RCX_ERR_BAD_ARG, "rcx_pack_recconv_params: null weight %d", j);
        P.w[j] = w[j];
        P.b[j] = b ? b[j] : nullptr;
    }
    hipError_t e = rcx::pack_params(P, wpack, wpack_flipped, bpack, count, C, k, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_pack_recconv_params");
}

int rcx_unpack_recconv_grads(const float* gwpack, void* const* gw, int count, int C, int k, void* stream)
{
    if (!gwpack || !gw || count <= 0 || count > RCX_MAX_LEVEL + 2 || C <= 0 || k <= 0) return fail(RCX_ERR_BAD_ARG, "rcx_unpack_recconv_grads: bad argument");
    rcx::PackPtrs P{};
    for (int j = 0; j < count; ++j) {
        if (!gw[j]) return fail(RCX_ERR_BAD_ARG, "rcx_unpack_recconv_grads: null destination %d", j);
        P.w[j] = gw[j];
    }
    hipError_t e = rcx::unpack_grads(gwpack, P, count, C, k, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_unpack_recconv_grads");
}

int rcx_pack_bias(const void* b, float* dst, int C, int dtype, void* stream)
{
    if (!b || !dst || C <= 0) return fail(RCX_ERR_BAD_ARG, "rcx_pack_bias: bad argument");
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    hipError_t e = rcx::pack_bias(b, dst, C, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_pack_bias");
}

size_t rcx_recconv2d_fwd_workspace_bytes(int N, int C, int H, int W, int level, int k, int dtype)
{
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || level < 0 || level > RCX_MAX_LEVEL || k <= 0 || (k & 1) == 0) return 0;
    switch (fwd_schedule(N, C, H, W, level, k, dtype)) {
    case FWD_LANES: return 0;                                       // registers only
    case FWD_SPLIT: return split_bytes(N, C, H, W);
    case FWD_PLANE: return 0;                                       // the fused schedule keeps every intermediate in LDS
    case FWD_NESTED:                                                // F_1, C_1, then whatever the inner block needs
        return nested_own_bytes(N, C, H, W) + rcx_recconv2d_fwd_workspace_bytes(N, C, H / 2, W / 2, level - 1, k, RCX_DTYPE_F32);
    default: return make_ladder(N, C, H, W, level, k).total;
    }
}

// ---- rcx_time_next_launch: see rcx_launch.h
extern "C++" {
namespace rcx {
static thread_local LaunchEvents g_launch_events;
LaunchEvents take_launch_events()
{
    const LaunchEvents e = g_launch_events;
    g_launch_events = LaunchEvents{};
    return e;
}
}  // namespace rcx
}

int rcx_time_next_launch(void* start_event, void* stop_event)
{
    rcx::g_launch_events.start = (hipEvent_t)start_event;
    rcx::g_launch_events.stop = (hipEvent_t)stop_event;
    return 0;
}

int rcx_launch_events_pending(void) { return (rcx::g_launch_events.start || rcx::g_launch_events.stop) ? 1 : 0; }

static int recconv2d_fwd_impl(const void* x, void* y, const float* wpack, const float* bpack, void* workspace, size_t workspace_bytes,
                              int N, int C, int H, int W, int level, int k, int mode, int dtype, void* stream);

int rcx_recconv2d_fwd(const void* x, void* y, const float* wpack, const float* bpack,
                      void* workspace, size_t workspace_bytes,
                      int N, int C, int H, int W, int level, int k, int mode, int dtype, void* stream)
{
    const int rc = recconv2d_fwd_impl(x, y, wpack, bpack, workspace, workspace_bytes, N, C, H, W, level, k, mode, dtype, stream);
    rcx::g_launch_events = rcx::LaunchEvents{};        // a pair the schedule did not consume (several launches, an unsupported kernel) does not wait for a later call
    return rc;
}

static int recconv2d_fwd_impl(const void* x, void* y, const float* wpack, const float* bpack,
                      void* workspace, size_t workspace_bytes,
                      int N, int C, int H, int W, int level, int k, int mode, int dtype, void* stream)
{
    if (int rc = check_common(x, y, N, C, H, W, k, dtype)) return rc;
    if (!wpack) return fail(RCX_ERR_BAD_ARG, "null weight pack");
    if (x == y) return fail(RCX_ERR_BAD_ARG, "y must not alias x");
    if (level < 0 || level > RCX_MAX_LEVEL) return fail(RCX_ERR_BAD_ARG, "level %d outside [0,%d]", level, RCX_MAX_LEVEL);
    if (mode != RCX_MODE_BILINEAR && mode != RCX_MODE_NEAREST) return fail(RCX_ERR_BAD_ARG, "unknown mode %d", mode);
    const FwdSchedule sch = fwd_schedule(N, C, H, W, level, k, dtype);
    if (sch == FWD_LANES) {
        hipError_t le = rcx::lanes_recconv(x, y, wpack, bpack, N, C, H, W, level, k, mode, dtype, (hipStream_t)stream);
        return le == hipSuccess ? 0 : hip_fail(le, "lanes schedule");
    }
    if (sch == FWD_SPLIT) {
        const size_t need = split_bytes(N, C, H, W);
        if (!workspace || workspace_bytes < need)
            return fail(RCX_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
        hipStream_t s = (hipStream_t)stream;
        float* f1 = (float*)workspace;
        float* c1 = (float*)((char*)workspace + need / 2);
        const size_t wsz = (size_t)k * k * C;
        hipError_t e = step_dwconv(x, f1, wpack, bpack, N, C, H, W, k, 2, dtype, RCX_DTYPE_F32, s);
        if (e != hipSuccess) return hip_fail(e, "split schedule: down");
        e = rcx::lanes_recconv(f1, c1, wpack, bpack, N, C, H / 2, W / 2, level - 1, k, mode, RCX_DTYPE_F32, s);
        if (e != hipSuccess) return hip_fail(e, "split schedule: inner block");
        e = step_upadd(x, c1, y, wpack + (size_t)(1 + level) * wsz, bpack ? bpack + (size_t)(1 + level) * C : nullptr,
                       N, C, H, W, H / 2, W / 2, k, mode, dtype, RCX_DTYPE_F32, dtype, s);
        return e == hipSuccess ? 0 : hip_fail(e, "split schedule: final conv");
    }
    if (sch == FWD_PLANE) {
        hipError_t pe = rcx::plane_recconv(x, y, wpack, bpack, N, C, H, W, level, k, mode, dtype, (hipStream_t)stream);
        return pe == hipSuccess ? 0 : hip_fail(pe, "plane schedule");
    }
    if (sch == FWD_NESTED) {
        const size_t own = nested_own_bytes(N, C, H, W);
        const size_t need = own + rcx_recconv2d_fwd_workspace_bytes(N, C, H / 2, W / 2, level - 1, k, RCX_DTYPE_F32);
        if (!workspace || workspace_bytes < need)
            return fail(RCX_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
        hipStream_t s = (hipStream_t)stream;
        float* f1 = (float*)workspace;
        float* c1 = (float*)((char*)workspace + own / 2);
        const size_t wsz = (size_t)k * k * C;
        hipError_t e = step_dwconv(x, f1, wpack, bpack, N, C, H, W, k, 2, dtype, RCX_DTYPE_F32, s);
        if (e != hipSuccess) return hip_fail(e, "nested schedule: down");
        // the inner block owns the first level + 1 packs (down, convs[0 .. level - 1]) exactly as the whole block owns level + 2
        if (int rc = rcx_recconv2d_fwd(f1, c1, wpack, bpack, (char*)workspace + own, need - own, N, C, H / 2, W / 2, level - 1, k, mode, RCX_DTYPE_F32, stream))
            return rc;
        e = step_upadd(x, c1, y, wpack + (size_t)(1 + level) * wsz, bpack ? bpack + (size_t)(1 + level) * C : nullptr,
                       N, C, H, W, H / 2, W / 2, k, mode, dtype, RCX_DTYPE_F32, dtype, s);
        return e == hipSuccess ? 0 : hip_fail(e, "nested schedule: final conv");
    }
    const Ladder L = make_ladder(N, C, H, W, level, k);
    if (L.total > 0 && (!workspace || workspace_bytes < L.total))
        return fail(RCX_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", L.total, workspace_bytes);
    size_t c_off[RCX_MAX_LEVEL + 1];
    for (int l = 1; l <= level; ++l) c_off[l] = L.c_off[(l + 1) & 1];               // C_1 -> buf 0, C_2 -> buf 1, ...
    return recconv2d_steps(x, y, wpack, bpack, (char*)workspace, L.f_off, c_off, L.h, L.w, N, C, level, k, mode, dtype, (hipStream_t)stream, "");
}

// ---- training: forward that keeps the fp32 pyramid, and the backward pass (rcx_bwd.hip) ----
namespace {

struct TrainLadder {
    int h[RCX_MAX_LEVEL + 1], w[RCX_MAX_LEVEL + 1];
    size_t f_off[RCX_MAX_LEVEL + 1], c_off[RCX_MAX_LEVEL + 1];   // F_l, C_l (l >= 1), all distinct
    size_t saved_total;
    size_t g_off[RCX_MAX_LEVEL + 1];                               // backward scratch: gT_0..gT_L
    size_t gc_off, part_off, part_bytes, bwd_total;
};

TrainLadder make_train_ladder(int N, int C, int H, int W, int level, int k)
{
    TrainLadder L{};
    L.h[0] = H; L.w[0] = W;
    size_t off = 0;
    for (int l = 1; l <= level; ++l) {
        L.h[l] = down_size(L.h[l - 1], k); L.w[l] = down_size(L.w[l - 1], k);
        const size_t b = align256(sizeof(float) * (size_t)N * C * L.h[l] * L.w[l]);
        L.f_off[l] = off; off += b;
        L.c_off[l] = off; off += b;
    }
    L.saved_total = off;
    off = 0;
    for (int l = 0; l <= level; ++l) { L.g_off[l] = off; off += align256(sizeof(float) * (size_t)N * C * L.h[l] * L.w[l]); }
    L.gc_off = off; off += level >= 1 ? align256(sizeof(float) * (size_t)N * C * L.h[1] * L.w[1]) : 0;
    L.part_bytes = align256(rcx::wgrad_partial_bytes(C, k));
    // the tiled weight-gradient kernels (rcx_cptbwd_kernels.h) leave one row of (k*k + 1) * C sums per (image, 14-row band): N * H / 14 rows
    if (rcx::bwd_cpt_applicable(N, C, H, W, k)) {
        const size_t tiled = align256(sizeof(float) * (size_t)N * ((H + 13) / 14) * (size_t)(k * k + 1) * C);
        if (tiled > L.part_bytes) L.part_bytes = tiled;
    }
    L.part_off = off; off += L.part_bytes * (size_t)(2 * level + 1);     // one partial buffer per weight-gradient call: reduced together
    L.bwd_total = off;
    return L;
}

// The training forward's schedule: the blocks of RecNeXt at 224x224 run their inference kernel, which then also leaves the pyramid behind (one
// launch instead of 2 * level + 1); everything else, and everything under RCX_TRAIN_FUSED=0, the per-step schedule
enum TrainFwdSchedule { TRAIN_TILED, TRAIN_CPL14, TRAIN_CPL7, TRAIN_STEPS };

TrainFwdSchedule train_fwd_schedule(int N, int C, int H, int W, int level, int k, int mode, int dtype)
{
    if (rcx::opt::off(rcx::opt::TRAIN_FUSED) || rcx::opt::hand_kernels_off()) return TRAIN_STEPS;
    if (rcx::cpt_train_applicable(N, C, H, W, level, k, mode == RCX_MODE_NEAREST ? 1 : 0, dtype)) return TRAIN_TILED;
    if (rcx::cpl14_applicable(N, C, H, W, level, k, dtype)) return TRAIN_CPL14;
    return rcx::cpl7b_applicable(N, C, H, W, level, k, dtype) ? TRAIN_CPL7 : TRAIN_STEPS;
}

// The backward schedule of a RecConv2d block (the workspace size depends on the shape alone).  The 14x14 tail: a block deeper than level 2 whose
// level m = level - 2 plane is 14x14 ends in exactly the 14x14 / level 2 block, whose whole backward is one launch.
//   BWD_ONE    the 14x14 / level 2 and 7x7 / level 1 blocks: the whole backward in one launch (rcx_cplbwd.hip; RCX_BWD_FUSED=0: off)
//   BWD_TILED  the 56x56 / level 4 and 28x28 / level 3 blocks: the m fine levels on the tiled adjoint kernels (rcx_cptbwd.hip), then the tail
//   BWD_STEPS  one launch per ladder step, down to the tail where there is one
enum BwdKind { BWD_ONE, BWD_TILED, BWD_STEPS };
struct BwdSchedule { BwdKind kind; int m; bool split; };      // m: the tail's level (0: none); split: the 14x14 launch runs two waves per plane

// The same kinds and cut-overs serve rcx_recconv2d_bwd (want_wgrads) and the input-only rcx_recconv2d_bwd_input; the one launch is the whole-block
// backward (rcx_cplbwd.hip) for the first and the input adjoint (rcx_cpladj.hip) for the second.  That kernel keeps no partial rows, so no batch
// limit; it runs one wave per plane (never split).
BwdSchedule bwd_schedule(const TrainLadder& L, int N, int C, int level, int k, int dtype, bool want_wgrads)
{
    auto one = [&](int H, int W, int lv, int dt) {
        return want_wgrads ? rcx::cplbwd_applicable(N, C, H, W, lv, k, dt) : rcx::cpladj_applicable(N, C, H, W, lv, k, dt);
    };
    const bool split = want_wgrads && rcx::cplbwd_split(N, C);
    if (level >= 1 && one(L.h[0], L.w[0], level, dtype)) return {BWD_ONE, 0, L.h[0] == 14 && split};
    const int m = level >= 3 && L.h[level - 2] == 14 && L.w[level - 2] == 14 && one(14, 14, 2, RCX_DTYPE_F32) ? level - 2 : 0;
    bool tiled = m > 0;       // ... and every plane above the tail 56x56 or 28x28
    for (int l = 0; l < m; ++l)
        tiled = tiled && rcx::bwd_cpt_applicable(N, C, L.h[l], L.w[l], k) && L.h[l + 1] * 2 == L.h[l] && L.w[l + 1] * 2 == L.w[l];
    return {tiled ? BWD_TILED : BWD_STEPS, m, m > 0 && split};
}

// One rcx_recconv2d_bwd or rcx_recconv2d_bwd_input call.  With wgrads: the weight-gradient jobs its partial buffers join (job 0 = the shared down
// conv, job 1 + j = convs[j]).  Without: x and saved are null, J and the partial slots stay unused.  prefix starts the error messages.
struct BwdRun {
    const TrainLadder& L;
    bool wgrads;
    const char* prefix;
    const void *x, *gy;
    void* gx;
    const float *wpack, *wflip;
    const char* saved;
    char* ws;
    int gy_dt, N, C, level, k, mode, dtype;
    hipStream_t s;
    rcx::WgradJobs J;
    int slot;
    const float* Wd(int i) const { return wpack + (size_t)i * k * k * C; }       // 0 = down, 1 + j = convs[j]
    const float* Wf(int i) const { return wflip + (size_t)i * k * k * C; }
    const float* F(int l) const { return (const float*)(saved + L.f_off[l]); }
    const float* Cs(int l) const { return (const float*)(saved + L.c_off[l]); }
    float* G(int l) const { return (float*)(ws + L.g_off[l]); }
    float* next_part() { return (float*)(ws + L.part_off + (size_t)slot++ * L.part_bytes); }
    void add(int job, const float* p, int rows) { J.part[job][J.nslots[job]] = p; J.rows[job][J.nslots[job]] = rows; ++J.nslots[job]; }
};

#define RCX_TRY(call, what, prefix) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail(e_, what, prefix); } while (0)

// the one-launch backward of the whole block (m = 0: x, g = gy) or of its tail (x = F_m, g = dL/dC_m, gx = G_m).  With weight gradients a partial
// row per image for jobs 0 .. level + 1; without, the input adjoint alone, which needs neither x nor the pyramid
hipError_t one_launch(BwdRun& B, const void* g, int g_dt, void* gx, int m, int H, int level, int dtype)
{
    const int md = B.mode == RCX_MODE_NEAREST ? 1 : 0;
    if (!B.wgrads) return rcx::cpladj_recconv(g, g_dt, B.wpack, B.wflip, gx, dtype, B.N, B.C, H, md, B.s);
    float* parts[RCX_MAX_LEVEL + 2];
    for (int j = 0; j < level + 2; ++j) { parts[j] = B.next_part(); B.add(j, parts[j], B.N); }
    return rcx::cplbwd_recconv(m ? B.F(m) : B.x, g, B.wpack, B.wflip, B.saved, B.L.f_off + m, B.L.c_off + m, gx, parts, B.N, B.C, H, level,
                               md, dtype, B.s, g_dt);
}

// BWD_TILED.  Top-down: gW_j from (a_l, C_{l+1}, g_l) and gC_{l+1} = R^T K^ g_l; the tail returns G_m; bottom-up: gW_d from (a_l, G_{l+1}) and
// G_l = K^ g_l + D^T G_{l+1} (G_0 = gx).  g_0 = gy in its own type, g_l = gC_l float32 (parked in the full-resolution slot G(0) the per-step
// schedule keeps gT_0 in: no gT plane exists here).  Without weight gradients the gW launches and their partial rows are skipped, nothing else.
int bwd_tiled(BwdRun& B, int m)
{
    const TrainLadder& L = B.L;
    const int N = B.N, C = B.C, md = B.mode == RCX_MODE_NEAREST ? 1 : 0;
    float* gcl[RCX_MAX_LEVEL + 1] = {};
    size_t off = 0;
    for (int l = 1; l <= m; ++l) { gcl[l] = (float*)(B.ws + L.g_off[0] + off); off += align256(sizeof(float) * (size_t)N * C * L.h[l] * L.w[l]); }
    auto g_of = [&](int l) { return l == 0 ? B.gy : (const void*)gcl[l]; };
    auto gdt_of = [&](int l) { return l == 0 ? B.gy_dt : RCX_DTYPE_F32; };
    auto a_of = [&](int l) { return l == 0 ? B.x : (const void*)B.F(l); };
    auto adt_of = [&](int l) { return l == 0 ? B.dtype : RCX_DTYPE_F32; };
    int rows = 0;
    // (Round 6 measured the four weight-gradient kernels on a second stream, forked and joined by events inside the call -- nothing but the final
    // reduction waits for them, and the chain's middle runs on a fraction of the chip: the event hand-offs cost more than the overlap returns,
    // 342 vs 301 us at 128 x 64 x 56 x 56, 301 vs 220 us at 256 x 128 x 28 x 28, equal at 256 x 64 x 56 x 56; profiles/r06_backward_side_stream.txt.)
    for (int l = 0; l < m; ++l) {
        const int j = B.level - l;                              // convs[j] is level l's conv
        if (B.wgrads) {
            float* p = B.next_part();
            RCX_TRY(rcx::bwd_wgrad_k_cpt(a_of(l), adt_of(l), B.Cs(l + 1), g_of(l), gdt_of(l), p, N, C, L.h[l], md, B.s, &rows), "conv weight grad", B.prefix);
            B.add(1 + j, p, rows);
        }
        RCX_TRY(rcx::bwd_gc_cpt(g_of(l), gdt_of(l), gcl[l + 1], B.Wf(1 + j), N, C, L.h[l], md, B.s), "gradient handed down", B.prefix);
    }
    RCX_TRY(one_launch(B, gcl[m], RCX_DTYPE_F32, B.G(m), m, 14, 2, RCX_DTYPE_F32), "fused nested block", B.prefix);
    for (int l = m - 1; l >= 0; --l) {
        if (B.wgrads) {
            float* p = B.next_part();
            RCX_TRY(rcx::bwd_wgrad_d_cpt(a_of(l), adt_of(l), B.G(l + 1), p, N, C, L.h[l], B.s, &rows), "down weight grad", B.prefix);
            B.add(0, p, rows);
        }
        RCX_TRY(rcx::bwd_gx_cpt(g_of(l), gdt_of(l), B.G(l + 1), l == 0 ? B.gx : (void*)B.G(l), l == 0 ? B.dtype : RCX_DTYPE_F32, B.Wf(1 + B.level - l),
                                B.Wd(0), N, C, L.h[l], B.s), "gradient handed up", B.prefix);
    }
    return 0;
}

// BWD_STEPS: the per-step forward read backwards, float32 throughout, down to the tail (m > 0); without weight gradients, minus the gW launches
int bwd_steps(BwdRun& B, int m)
{
    const TrainLadder& L = B.L;
    const int N = B.N, C = B.C, H = L.h[0], W = L.w[0], level = B.level, k = B.k, mode = B.mode, dtype = B.dtype;
    float* gC = (float*)(B.ws + L.gc_off);
    const float* gyf = (const float*)B.gy;
    int rows = 0;
    // final conv (model/recnext.py:34): gT_0 = K_L^T gy (gx itself with no ladder) ; gW_L = <x + R(C_1), gy>
    RCX_TRY(step_dwconv(gyf, level == 0 ? B.gx : (void*)B.G(0), B.Wf(1 + level), nullptr, N, C, H, W, k, 1, RCX_DTYPE_F32,
                        level == 0 ? dtype : RCX_DTYPE_F32, B.s), "final conv input grad", B.prefix);
    if (B.wgrads) {
        float* p = B.next_part();
        RCX_TRY(rcx::bwd_wgrad(B.x, dtype, level >= 1 ? B.Cs(1) : nullptr, gyf, p, B.J.gw[1 + level], B.J.gb[1 + level], N, C, H, W,
                               level >= 1 ? L.h[1] : 0, level >= 1 ? L.w[1] : 0, H, W, k, 1, mode, 0, B.s, &rows), "final conv weight grad", B.prefix);
        B.add(1 + level, p, rows);
    }
    // up recursion (:31-33), finest level first in the backward direction
    for (int l = 1; l <= level; ++l) {
        const int j = level - l;
        RCX_TRY(rcx::bwd_resize(B.G(l - 1), gC, N, C, L.h[l - 1], L.w[l - 1], L.h[l], L.w[l], mode, B.s), "resize adjoint", B.prefix);
        if (l == m) { RCX_TRY(one_launch(B, gC, RCX_DTYPE_F32, B.G(m), m, 14, 2, RCX_DTYPE_F32), "fused nested block", B.prefix); break; }
        RCX_TRY(step_dwconv(gC, B.G(l), B.Wf(1 + j), nullptr, N, C, L.h[l], L.w[l], k, 1, RCX_DTYPE_F32, RCX_DTYPE_F32, B.s), "conv input grad", B.prefix);
        if (!B.wgrads) continue;
        float* p = B.next_part();
        RCX_TRY(rcx::bwd_wgrad(B.F(l), RCX_DTYPE_F32, l < level ? B.Cs(l + 1) : nullptr, gC, p, B.J.gw[1 + j], B.J.gb[1 + j], N, C, L.h[l], L.w[l],
                               l < level ? L.h[l + 1] : 0, l < level ? L.w[l + 1] : 0, L.h[l], L.w[l], k, 1, mode, 0, B.s, &rows), "conv weight grad", B.prefix);
        B.add(1 + j, p, rows);
    }
    // down ladder (:27-29), coarsest first: the shared weight accumulates over all levels
    for (int l = m ? m : level; l >= 1; --l) {
        if (B.wgrads) {
            float* p = B.next_part();
            RCX_TRY(rcx::bwd_wgrad(l == 1 ? B.x : (const void*)B.F(l - 1), l == 1 ? dtype : RCX_DTYPE_F32, nullptr, B.G(l), p, B.J.gw[0], B.J.gb[0],
                                   N, C, L.h[l - 1], L.w[l - 1], 0, 0, L.h[l], L.w[l], k, 2, mode, 0, B.s, &rows), "down weight grad", B.prefix);
            B.add(0, p, rows);
        }
        RCX_TRY(rcx::bwd_down_input(B.G(l - 1), B.G(l), l == 1 ? B.gx : (void*)B.G(l - 1), l == 1 ? dtype : RCX_DTYPE_F32, B.Wd(0),
                                    N, C, L.h[l - 1], L.w[l - 1], L.h[l], L.w[l], k, B.s), "down input grad", B.prefix);
    }
    return 0;
}

// the seven shape queries below answer 0 / float32 / "invalid" outside these extents (the launch entries diagnose each one: check_common, check_bwd_args)
bool bwd_extents_ok(int N, int C, int H, int W, int level, int k)
{
    return N > 0 && C > 0 && H > 0 && W > 0 && level >= 0 && level <= RCX_MAX_LEVEL && k > 0 && (k & 1);
}

// the argument checks rcx_recconv2d_bwd and rcx_recconv2d_bwd_input share, after check_common and their own pointer checks
int check_bwd_args(int gy_dtype, int C, int level, int mode)
{
    if (!known_dtype(gy_dtype)) return fail(RCX_ERR_BAD_ARG, "unknown gy dtype %d", gy_dtype);
    if (level < 0 || level > RCX_MAX_LEVEL) return fail(RCX_ERR_BAD_ARG, "level %d outside [0,%d]", level, RCX_MAX_LEVEL);
    if (mode != RCX_MODE_BILINEAR && mode != RCX_MODE_NEAREST) return fail(RCX_ERR_BAD_ARG, "unknown mode %d", mode);
    if (C % 4) return fail(RCX_ERR_UNSUPPORTED, "the backward kernels need C %% 4 == 0, got C=%d", C);
    return 0;
}

// The workspace of an input-only backward: none for the one-launch blocks, else the float32 gradient planes of the training backward's
// ladder (gT_0 .. gT_L and the resized-gradient plane) without its partial-sum buffers
size_t bwd_input_workspace(const TrainLadder& L, BwdKind kind) { return kind == BWD_ONE ? 0 : L.part_off; }

// rcx_recconv2d_bwd_plan / rcx_recconv2d_bwd_input_plan, into the entry's own buffer: stem is the one-launch kernel's name without its plane size
const char* bwd_plan(char (&desc)[64], int N, int C, int H, int W, int level, int k, int dtype, bool want_wgrads, const char* stem)
{
    if (!bwd_extents_ok(N, C, H, W, level, k) || !known_dtype(dtype)) return "invalid";
    if (rcx::opt::hand_kernels_off()) return "generic";
    const BwdSchedule b = bwd_schedule(make_train_ladder(N, C, H, W, level, k), N, C, level, k, dtype, want_wgrads);
    if (b.kind == BWD_STEPS && !b.m) return "steps";
    const char* cpl = b.kind == BWD_ONE && H != 14 ? "cpl7" : "cpl14", *split = b.split ? ",split" : "";
    if (b.kind == BWD_ONE) snprintf(desc, sizeof(desc), "one(%s%s%s)", stem, cpl, split);
    else if (b.kind == BWD_TILED) snprintf(desc, sizeof(desc), "tiled(levels=%d)+one(%s%s%s)", b.m, stem, cpl, split);
    else snprintf(desc, sizeof(desc), "steps+one(%s%s%s)", stem, cpl, split);
    return desc;
}

}  // namespace

size_t rcx_recconv2d_train_saved_bytes(int N, int C, int H, int W, int level, int k)
{
    if (!bwd_extents_ok(N, C, H, W, level, k)) return 0;
    return make_train_ladder(N, C, H, W, level, k).saved_total;
}

size_t rcx_recconv2d_bwd_workspace_bytes(int N, int C, int H, int W, int level, int k)
{
    if (!bwd_extents_ok(N, C, H, W, level, k)) return 0;
    return make_train_ladder(N, C, H, W, level, k).bwd_total;
}

int rcx_recconv2d_fwd_train(const void* x, void* y, const float* wpack, const float* bpack, void* saved, size_t saved_bytes,
                            int N, int C, int H, int W, int level, int k, int mode, int dtype, void* stream)
{
    if (int rc = check_common(x, y, N, C, H, W, k, dtype)) return rc;
    if (!wpack) return fail(RCX_ERR_BAD_ARG, "null weight pack");
    if (level < 0 || level > RCX_MAX_LEVEL) return fail(RCX_ERR_BAD_ARG, "level %d outside [0,%d]", level, RCX_MAX_LEVEL);
    if (mode != RCX_MODE_BILINEAR && mode != RCX_MODE_NEAREST) return fail(RCX_ERR_BAD_ARG, "unknown mode %d", mode);
    const TrainLadder L = make_train_ladder(N, C, H, W, level, k);
    if (L.saved_total > 0 && (!saved || saved_bytes < L.saved_total))
        return fail(RCX_ERR_WORKSPACE, "saved-activation buffer too small: need %zu bytes, got %zu", L.saved_total, saved_bytes);
    hipStream_t s = (hipStream_t)stream;
    const int md = mode == RCX_MODE_NEAREST ? 1 : 0;
    const TrainFwdSchedule sch = train_fwd_schedule(N, C, H, W, level, k, mode, dtype);
    if (sch == TRAIN_STEPS) return recconv2d_steps(x, y, wpack, bpack, (char*)saved, L.f_off, L.c_off, L.h, L.w, N, C, level, k, mode, dtype, s, "train fwd: ");
    const hipError_t e = sch == TRAIN_TILED ? rcx::cpt_recconv(x, y, wpack, bpack, N, C, H, level, md, dtype, s, (float*)saved, L.f_off, L.c_off)
                       : sch == TRAIN_CPL14 ? rcx::cpl14_recconv(x, y, wpack, bpack, N, C, md, dtype, s, (float*)saved, L.f_off, L.c_off)
                                            : rcx::cpl7b_recconv(x, y, wpack, bpack, N, C, md, dtype, s, (float*)saved, L.f_off, L.c_off);
    static const char* const what[] = {"train fwd: fused tiled block", "train fwd: fused 14x14 block", "train fwd: fused 7x7 block"};
    return e == hipSuccess ? 0 : hip_fail(e, what[sch]);
}

int rcx_recconv2d_bwd_gy_dtype(int N, int C, int H, int W, int level, int k, int dtype)
{
    if (!bwd_extents_ok(N, C, H, W, level, k) || !known_dtype(dtype)) return RCX_DTYPE_F32;
    // bfloat16 (float16 rows on both sides overflow the tiled weight-gradient kernel's registers), where the one-launch or tiled backward reads it
    if (dtype != RCX_DTYPE_BF16 || C % 4) return RCX_DTYPE_F32;
    return bwd_schedule(make_train_ladder(N, C, H, W, level, k), N, C, level, k, dtype, true).kind != BWD_STEPS ? dtype : RCX_DTYPE_F32;
}

const char* rcx_recconv2d_bwd_plan(int N, int C, int H, int W, int level, int k, int dtype)
{
    static thread_local char desc[64];
    return bwd_plan(desc, N, C, H, W, level, k, dtype, true, "k_recconv_bwd_");
}

int rcx_recconv2d_bwd(const void* x, const void* gy, int gy_dtype, const float* wpack, const float* wpack_flipped, const void* saved,
                      void* gx, float* gwpack, float* gbpack, void* const* gw_out, void* const* gb_out, int grad_dtype,
                      void* workspace, size_t workspace_bytes,
                      int N, int C, int H, int W, int level, int k, int mode, int dtype, void* stream)
{
    if (int rc = check_common(x, gx, N, C, H, W, k, dtype)) return rc;
    if (!gy || !wpack || !wpack_flipped || (!gwpack && !gw_out)) return fail(RCX_ERR_BAD_ARG, "null gradient / weight pointer");
    if (gw_out && !known_dtype(grad_dtype)) return fail(RCX_ERR_BAD_ARG, "unknown gradient dtype %d", grad_dtype);
    if (int rc = check_bwd_args(gy_dtype, C, level, mode)) return rc;
    const TrainLadder L = make_train_ladder(N, C, H, W, level, k);
    if (level >= 1 && !saved) return fail(RCX_ERR_BAD_ARG, "null saved-activation buffer");
    if (!workspace || workspace_bytes < L.bwd_total)
        return fail(RCX_ERR_WORKSPACE, "backward workspace too small: need %zu bytes, got %zu", L.bwd_total, workspace_bytes);
    const BwdSchedule sch = bwd_schedule(L, N, C, level, k, dtype, true);
    if (gy_dtype != RCX_DTYPE_F32 && !(sch.kind != BWD_STEPS && gy_dtype == dtype && dtype == RCX_DTYPE_BF16))
        return fail(RCX_ERR_UNSUPPORTED, "gy of dtype %d: this problem takes float32 (rcx_recconv2d_bwd_gy_dtype)", gy_dtype);
    if (gw_out)
        for (int i = 0; i < level + 2; ++i)
            if (!gw_out[i]) return fail(RCX_ERR_BAD_ARG, "null gw_out[%d]", i);
    hipStream_t s = (hipStream_t)stream;
    BwdRun B{L, true, "bwd: "};
    B.x = x; B.gy = gy; B.wpack = wpack; B.wflip = wpack_flipped; B.saved = (const char*)saved; B.ws = (char*)workspace; B.gx = gx;
    B.gy_dt = gy_dtype; B.N = N; B.C = C; B.level = level; B.k = k; B.mode = mode; B.dtype = dtype; B.s = s;
    // where the final reduction leaves conv i's gradients: the packed float32 rows, or the parameters' own tensors
    rcx::WgradJobs& J = B.J;
    J.njobs = level + 2; J.kk = k * k; J.C = C; J.param_layout = gw_out ? 1 : 0; J.param_dt = grad_dtype;
    for (int i = 0; i < level + 2; ++i) {
        J.gw[i] = gw_out ? (float*)gw_out[i] : gwpack + (size_t)i * k * k * C;
        J.gb[i] = gw_out ? (gb_out ? (float*)gb_out[i] : nullptr) : (gbpack ? gbpack + (size_t)i * C : nullptr);
    }
    if (sch.kind == BWD_ONE) RCX_TRY(one_launch(B, gy, gy_dtype, gx, 0, H, level, dtype), "fused block", B.prefix);
    else if (int rc = sch.kind == BWD_TILED ? bwd_tiled(B, sch.m) : bwd_steps(B, sch.m)) return rc;
    // every weight gradient of the block in one reduction launch (job 0 sums the down conv's levels, coarsest first).  With no ladder the shared
    // down weight is unused: conv 0 is reduced alone, and the down gradient zeroed.
    float* const gw0 = J.gw[0], * const gb0 = J.gb[0];
    if (level == 0) { J.njobs = 1; J.gw[0] = J.gw[1]; J.gb[0] = J.gb[1]; J.nslots[0] = J.nslots[1]; J.part[0][0] = J.part[1][0]; J.rows[0][0] = J.rows[1][0]; }
    RCX_TRY(rcx::bwd_wgrad_reduce_jobs(J, s), "weight-gradient reduction", B.prefix);
    if (level >= 1) return 0;
    const size_t esz = gw_out && grad_dtype != RCX_DTYPE_F32 ? 2 : 4;
    hipError_t e = hipMemsetAsync(gw0, 0, esz * k * k * C, s);
    if (e == hipSuccess && gb0) e = hipMemsetAsync(gb0, 0, esz * C, s);
    return e == hipSuccess ? 0 : hip_fail(e, "bwd: zero down grad");
}

// ---- the input-only backward: gx = A^T gy, from gy and the taps alone (the block is linear in x) ----
size_t rcx_recconv2d_bwd_input_workspace_bytes(int N, int C, int H, int W, int level, int k)
{
    if (!bwd_extents_ok(N, C, H, W, level, k)) return 0;
    const TrainLadder L = make_train_ladder(N, C, H, W, level, k);
    // the one-launch kernels take every dtype the fused forward does, so the float32 schedule decides for all three
    return bwd_input_workspace(L, bwd_schedule(L, N, C, level, k, RCX_DTYPE_F32, false).kind);
}

int rcx_recconv2d_bwd_input_gy_dtype(int N, int C, int H, int W, int level, int k, int dtype)
{
    if (!bwd_extents_ok(N, C, H, W, level, k) || !known_dtype(dtype) || dtype == RCX_DTYPE_F32 || C % 4) return RCX_DTYPE_F32;
    // the block's own 16-bit type where the one-launch or tiled kernels read gy (bfloat16 and float16 alike: no weight-gradient kernel runs)
    return bwd_schedule(make_train_ladder(N, C, H, W, level, k), N, C, level, k, dtype, false).kind != BWD_STEPS ? dtype : RCX_DTYPE_F32;
}

const char* rcx_recconv2d_bwd_input_plan(int N, int C, int H, int W, int level, int k, int dtype)
{
    static thread_local char desc[64];
    return bwd_plan(desc, N, C, H, W, level, k, dtype, false, "k_recconv_adj_");
}

int rcx_recconv2d_bwd_input(const void* gy, int gy_dtype, const float* wpack, const float* wpack_flipped, void* gx,
                            void* workspace, size_t workspace_bytes,
                            int N, int C, int H, int W, int level, int k, int mode, int dtype, void* stream)
{
    if (int rc = check_common(gy, gx, N, C, H, W, k, dtype)) return rc;
    if (!wpack || !wpack_flipped) return fail(RCX_ERR_BAD_ARG, "null weight pack");
    if (gy == gx) return fail(RCX_ERR_BAD_ARG, "gx must not alias gy");
    if (int rc = check_bwd_args(gy_dtype, C, level, mode)) return rc;
    const TrainLadder L = make_train_ladder(N, C, H, W, level, k);
    const BwdSchedule sch = bwd_schedule(L, N, C, level, k, dtype, false);
    const size_t need = bwd_input_workspace(L, sch.kind);
    if (need && (!workspace || workspace_bytes < need))
        return fail(RCX_ERR_WORKSPACE, "input-backward workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    if (gy_dtype != RCX_DTYPE_F32 && !(sch.kind != BWD_STEPS && gy_dtype == dtype))
        return fail(RCX_ERR_UNSUPPORTED, "gy of dtype %d: this problem takes float32 (rcx_recconv2d_bwd_input_gy_dtype)", gy_dtype);
    BwdRun B{L, false, "bwd input: "};
    B.gy = gy; B.gx = gx; B.wpack = wpack; B.wflip = wpack_flipped; B.ws = (char*)workspace;
    B.gy_dt = gy_dtype; B.N = N; B.C = C; B.level = level; B.k = k; B.mode = mode; B.dtype = dtype; B.s = (hipStream_t)stream;
    if (sch.kind == BWD_ONE) RCX_TRY(one_launch(B, gy, gy_dtype, gx, 0, H, level, dtype), "fused block", B.prefix);
    else return sch.kind == BWD_TILED ? bwd_tiled(B, sch.m) : bwd_steps(B, sch.m);
    return 0;
}

#undef RCX_TRY

int rcx_dwconv2d_fwd(const void* x, void* y, const float* w_kkc, const float* bias,
                     int N, int C, int H, int W, int k, int stride, int in_dtype, int out_dtype, void* stream)
{
    if (int rc = check_common(x, y, N, C, H, W, k, in_dtype)) return rc;
    if (!known_dtype(out_dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", out_dtype);
    if (!w_kkc) return fail(RCX_ERR_BAD_ARG, "null weight");
    if (stride != 1 && stride != 2) return fail(RCX_ERR_UNSUPPORTED, "stride %d not supported (1 or 2)", stride);
    hipError_t e = step_dwconv(x, y, w_kkc, bias, N, C, H, W, k, stride, in_dtype, out_dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_dwconv2d_fwd");
}

int rcx_dwconv2d_mult2_fwd(const void* x, void* y, const float* w_kkc, const float* bias,
                           int N, int Cin, int H, int W, int k, int stride, int dtype, void* stream)
{
    if (int rc = check_common(x, y, N, Cin, H, W, k, dtype)) return rc;
    if (!w_kkc) return fail(RCX_ERR_BAD_ARG, "null weight");
    if (stride != 1 && stride != 2) return fail(RCX_ERR_UNSUPPORTED, "stride %d not supported (1 or 2)", stride);
    // Downsample's conv: the register-resident lanes kernel on the planes it was built for (28 x 28 .. 64 x 64: 256 x 64 x 56 x 56 56.7 us
    // = 0.34 of 8 TB/s against the tiled kernel's 64.3), the tiled channel-per-lane kernel (rcx_upcpt.hip, round 3) on the large lanes planes
    // (32 x 64 x 128 x 128: 55 us against 164; 64 x 64 x 112 x 112: 61 against 246), on 14 x 14 (20.6 against 25.9) and on everything the
    // lanes kernel has no plan for (float16; COCO stages 200 x 336: 17 us against the generic kernel's 62).  Never a function of N.
    hipError_t e;
    const bool lanes_ok = !rcx::opt::hand_kernels_off() && rcx::down_lanes_applicable(N, Cin, H, W, k, stride, dtype);
    const bool tiled_ok = !rcx::opt::hand_kernels_off() && rcx::down7m2_cpt_applicable(N, Cin, H, W, k, stride, dtype);
    if (tiled_ok && (!lanes_ok || H > 64 || W > 64 || (H <= 14 && W <= 14) || upcpt_everywhere()))
        e = rcx::down7m2_cpt(x, y, w_kkc, bias, N, Cin, H, W, dtype, (hipStream_t)stream);
    else if (lanes_ok)
        e = rcx::down_lanes(x, y, w_kkc, bias, N, Cin, H, W, k, stride, dtype, (hipStream_t)stream);
    else
        e = rcx::generic_dwconv_mult2(x, y, w_kkc, bias, N, Cin, H, W, k, stride, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_dwconv2d_mult2_fwd");
}

const char* rcx_upadd_dwconv_fwd_plan(int N, int C, int H, int W, int Hc, int Wc, int k, int mode, int x_dtype, int coarse_dtype, int out_dtype, int has_coarse)
{
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || k <= 0 || (k & 1) == 0) return "invalid";
    static thread_local char desc[160];
    switch (pick_upadd(N, C, H, W, Hc, Wc, k, x_dtype, coarse_dtype, out_dtype, has_coarse != 0)) {
    case STEP_CPL14: return H == 7 ? "upadd_cpl14(k_upadd_cpl7)" : "upadd_cpl14(k_upadd_cpl14)";
    case STEP_CPT: return rcx::upadd_cpt_describe(N, C, H, W, mode == RCX_MODE_NEAREST ? 1 : 0, x_dtype, desc, (int)sizeof(desc)) > 0 ? desc : "upadd_cpt(k_upadd_cpt)";
    case STEP_LANES: return "upadd_lanes(k_upadd_lanes)";
    case STEP_CONV5_LANES: return "conv5_lanes(k_upadd_lanes)";
    default: return "generic";
    }
}

int rcx_upadd_dwconv_fwd(const void* x, const void* coarse, void* y, const float* w_kkc, const float* bias,
                         int N, int C, int H, int W, int Hc, int Wc, int k, int mode,
                         int x_dtype, int coarse_dtype, int out_dtype, void* stream)
{
    if (int rc = check_common(x, y, N, C, H, W, k, x_dtype)) return rc;
    if (!known_dtype(out_dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", out_dtype);
    if (!w_kkc) return fail(RCX_ERR_BAD_ARG, "null weight");
    if (mode != RCX_MODE_BILINEAR && mode != RCX_MODE_NEAREST) return fail(RCX_ERR_BAD_ARG, "unknown mode %d", mode);
    if (coarse) {
        if (Hc <= 0 || Wc <= 0) return fail(RCX_ERR_BAD_ARG, "non-positive coarse extent %dx%d", Hc, Wc);
        if (!known_dtype(coarse_dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", coarse_dtype);
    }
    hipError_t e = step_upadd(x, coarse, y, w_kkc, bias, N, C, H, W, Hc, Wc, k, mode, x_dtype, coarse_dtype, out_dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_upadd_dwconv_fwd");
}

// ---- backward of the depthwise convs of RecAttn2d and Downsample ----
namespace {

// the argument checks the three entries below share (check_common's counterpart); c_mult: the channel multiple their kernels need
int check_dw_bwd(const char* who, bool have_ptrs, int N, int C, int H, int W, int dtype, int c_mult)
{
    if (!have_ptrs) return fail(RCX_ERR_BAD_ARG, "%s: null pointer", who);
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(RCX_ERR_BAD_ARG, "non-positive extent N=%d C=%d H=%d W=%d", N, C, H, W);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    if (C % c_mult) return fail(RCX_ERR_UNSUPPORTED, "%s: the backward kernels need C %% %d == 0, got C=%d", who, c_mult, C);
    return 0;
}

// gw / gb = the sum of the `rows` partial rows one tiled kernel left in `part`
hipError_t reduce_one(const float* part, int rows, float* gw, float* gb, int k, int C, hipStream_t s)
{
    rcx::WgradJobs J{};
    J.njobs = 1; J.kk = k * k; J.C = C;
    J.nslots[0] = 1; J.part[0][0] = part; J.rows[0][0] = rows; J.gw[0] = gw; J.gb[0] = gb;
    return rcx::bwd_wgrad_reduce_jobs(J, s);
}

// rcx_dwconv2d_bwd: the stride-2 conv5 on the 56 x 56 / 28 x 28 planes (RecAttn2d's `down` conv) takes the tiled adjoint kernels of
// rcx_recconv2d_bwd (round 6) for its input gradient ...
bool dw_bwd_tiled_gx(int N, int C, int H, int W, int k, int stride)
{
    return stride == 2 && !rcx::opt::hand_kernels_off() && rcx::bwd_cpt_applicable(N, C, H, W, k) && down_size(H, k) * 2 == H && down_size(W, k) * 2 == W;
}

// ... and for its weight gradient while the tiled kernel's N * H / 14 partial rows fit the workspace: rcx_dwconv2d_bwd_workspace_bytes takes no N
// and holds 512 rows (wgrad_partial_bytes), so a larger batch reduces on the generic kernel
bool dw_bwd_tiled_gw(int N, int C, int H, int W, int k, int stride) { return dw_bwd_tiled_gx(N, C, H, W, k, stride) && N * (H / 14) <= 512; }

// backward of conv(x + resize(coarse)) (RecAttn2d's last line in a training step): the tiled adjoint kernels on the 56 x 56 / 28 x 28 planes
bool upadd_bwd_tiled(int N, int C, int H, int W, int Hc, int Wc, int k)
{
    return !rcx::opt::hand_kernels_off() && rcx::bwd_cpt_applicable(N, C, H, W, k) && Hc * 2 == H && Wc * 2 == W;
}

}  // namespace

size_t rcx_dwconv2d_bwd_workspace_bytes(int C, int k)
{
    if (C <= 0 || k <= 0 || (k & 1) == 0) return 0;
    return align256(rcx::wgrad_partial_bytes(C, k));
}

int rcx_dwconv2d_bwd(const void* x, const float* gy, const float* w_kkc, const float* w_flipped_kkc,
                     void* gx, float* gw, float* gb, void* workspace, size_t workspace_bytes,
                     int N, int C, int H, int W, int k, int stride, int x_dtype, void* stream)
{
    if (k <= 0 || (k & 1) == 0) return fail(RCX_ERR_BAD_ARG, "kernel_size must be odd and positive, got %d", k);
    if (int rc = check_dw_bwd("rcx_dwconv2d_bwd", x && gy && gw, N, C, H, W, x_dtype, 4)) return rc;
    if (stride != 1 && stride != 2) return fail(RCX_ERR_UNSUPPORTED, "stride %d not supported (1 or 2)", stride);
    if (gx && (!w_kkc || !w_flipped_kkc)) return fail(RCX_ERR_BAD_ARG, "rcx_dwconv2d_bwd: weights are needed for the input gradient");
    const size_t need = rcx_dwconv2d_bwd_workspace_bytes(C, k);
    if (!workspace || workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    const int p = k / 2, Ho = (H + 2 * p - k) / stride + 1, Wo = (W + 2 * p - k) / stride + 1;
    hipError_t e;
    if (gx) {
        if (stride == 1) e = step_dwconv(gy, gx, w_flipped_kkc, nullptr, N, C, H, W, k, 1, RCX_DTYPE_F32, x_dtype, s);
        else if (dw_bwd_tiled_gx(N, C, H, W, k, stride)) e = rcx::bwd_dT_cpt(gy, gx, x_dtype, w_kkc, N, C, H, s);
        else e = rcx::bwd_down_input(nullptr, gy, gx, x_dtype, w_kkc, N, C, H, W, Ho, Wo, k, s);
        if (e != hipSuccess) return hip_fail(e, "rcx_dwconv2d_bwd: input gradient");
    }
    int rows = 0;
    if (!dw_bwd_tiled_gw(N, C, H, W, k, stride))
        e = rcx::bwd_wgrad(x, x_dtype, nullptr, gy, (float*)workspace, gw, gb, N, C, H, W, 0, 0, Ho, Wo, k, stride, 0, 0, s);
    else if ((e = rcx::bwd_wgrad_d_cpt(x, x_dtype, gy, (float*)workspace, N, C, H, s, &rows)) == hipSuccess)
        e = reduce_one((const float*)workspace, rows, gw, gb, k, C, s);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_dwconv2d_bwd: weight gradient");
}

size_t rcx_upadd_dwconv_bwd_workspace_bytes(int N, int C, int H, int W, int Hc, int Wc, int k)
{
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || k <= 0 || (k & 1) == 0) return 0;
    if (upadd_bwd_tiled(N, C, H, W, Hc, Wc, k)) return align256(sizeof(float) * (size_t)N * ((H + 13) / 14) * (size_t)(k * k + 1) * C);      // one partial row per (image, band)
    return align256(rcx::wgrad_partial_bytes(C, k)) + align256(sizeof(float) * (size_t)N * C * H * W);      // + the float32 gT the resize adjoint reads
}

int rcx_upadd_dwconv_bwd_gy_dtype(int N, int C, int H, int W, int Hc, int Wc, int k, int dtype)
{
    if (dtype != RCX_DTYPE_BF16 || N <= 0 || C <= 0 || C % 4 || k <= 0 || (k & 1) == 0) return RCX_DTYPE_F32;
    return upadd_bwd_tiled(N, C, H, W, Hc, Wc, k) ? dtype : RCX_DTYPE_F32;
}

int rcx_upadd_dwconv_bwd(const void* x, const float* coarse, const void* gy, int gy_dtype, const float* w_kkc, const float* w_flipped_kkc,
                         void* gx, float* gcoarse, float* gw, float* gb, void* workspace, size_t workspace_bytes,
                         int N, int C, int H, int W, int Hc, int Wc, int k, int mode, int dtype, void* stream)
{
    if (Hc <= 0 || Wc <= 0) return fail(RCX_ERR_BAD_ARG, "non-positive coarse extent %dx%d", Hc, Wc);
    if (k <= 0 || (k & 1) == 0) return fail(RCX_ERR_BAD_ARG, "kernel_size must be odd and positive, got %d", k);
    if (!known_dtype(gy_dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", gy_dtype);
    if (mode != RCX_MODE_BILINEAR && mode != RCX_MODE_NEAREST) return fail(RCX_ERR_BAD_ARG, "unknown mode %d", mode);
    if (int rc = check_dw_bwd("rcx_upadd_dwconv_bwd", x && coarse && gy && gw && w_flipped_kkc, N, C, H, W, dtype, 4)) return rc;
    const size_t need = rcx_upadd_dwconv_bwd_workspace_bytes(N, C, H, W, Hc, Wc, k);
    if (!workspace || workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    const bool tiled = upadd_bwd_tiled(N, C, H, W, Hc, Wc, k);
    if (gy_dtype != RCX_DTYPE_F32 && !(tiled && gy_dtype == dtype && dtype == RCX_DTYPE_BF16))
        return fail(RCX_ERR_UNSUPPORTED, "gy of dtype %d: this problem takes float32 (rcx_upadd_dwconv_bwd_gy_dtype)", gy_dtype);
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    hipError_t e;
    if (tiled) {
        const int md = mode == RCX_MODE_NEAREST ? 1 : 0;
        if (gcoarse) {
            e = rcx::bwd_gc_cpt(gy, gy_dtype, gcoarse, w_flipped_kkc, N, C, H, md, s);
            if (e != hipSuccess) return hip_fail(e, "rcx_upadd_dwconv_bwd: coarse gradient");
        }
        if (gx) {
            e = rcx::bwd_gx_cpt(gy, gy_dtype, nullptr, gx, dtype, w_flipped_kkc, nullptr, N, C, H, s);
            if (e != hipSuccess) return hip_fail(e, "rcx_upadd_dwconv_bwd: input gradient");
        }
        int rows = 0;
        e = rcx::bwd_wgrad_k_cpt(x, dtype, coarse, gy, gy_dtype, part, N, C, H, md, s, &rows);
        if (e == hipSuccess) e = reduce_one(part, rows, gw, gb, k, C, s);
        return e == hipSuccess ? 0 : hip_fail(e, "rcx_upadd_dwconv_bwd: weight gradient");
    }
    const float* gyf = (const float*)gy;
    float* gT = (float*)((char*)workspace + align256(rcx::wgrad_partial_bytes(C, k)));
    if (gcoarse) {
        e = step_dwconv(gyf, gT, w_flipped_kkc, nullptr, N, C, H, W, k, 1, RCX_DTYPE_F32, RCX_DTYPE_F32, s);
        if (e == hipSuccess) e = rcx::bwd_resize(gT, gcoarse, N, C, H, W, Hc, Wc, mode, s);
        if (e != hipSuccess) return hip_fail(e, "rcx_upadd_dwconv_bwd: coarse gradient");
    }
    if (gx) {
        if (gcoarse && dtype == RCX_DTYPE_F32) e = hipMemcpyAsync(gx, gT, sizeof(float) * (size_t)N * C * H * W, hipMemcpyDeviceToDevice, s);
        else e = step_dwconv(gyf, gx, w_flipped_kkc, nullptr, N, C, H, W, k, 1, RCX_DTYPE_F32, dtype, s);
        if (e != hipSuccess) return hip_fail(e, "rcx_upadd_dwconv_bwd: input gradient");
    }
    e = rcx::bwd_wgrad(x, dtype, coarse, gyf, part, gw, gb, N, C, H, W, Hc, Wc, H, W, k, 1, mode, 0, s);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_upadd_dwconv_bwd: weight gradient");
}

int rcx_dwconv2d_mult2_bwd(const void* x, const float* gy, const float* w_kkc, void* gx, float* gw, float* gb,
                           void* workspace, size_t workspace_bytes, int N, int Cin, int H, int W, int k, int dtype, void* stream)
{
    if (int rc = check_dw_bwd("rcx_dwconv2d_mult2_bwd", x && gy && gw, N, Cin, H, W, dtype, 2)) return rc;
    if (k != 3 && k != 5 && k != 7) return fail(RCX_ERR_UNSUPPORTED, "kernel_size %d not supported by the multiplier-2 backward (3, 5, 7)", k);
    if (gx && !w_kkc) return fail(RCX_ERR_BAD_ARG, "rcx_dwconv2d_mult2_bwd: weights are needed for the input gradient");
    const size_t need = rcx_dwconv2d_bwd_workspace_bytes(2 * Cin, k);
    if (!workspace || workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    hipError_t e = rcx::bwd_mult2(x, dtype, gy, w_kkc, gx, (float*)workspace, gw, gb, N, Cin, H, W, k, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_dwconv2d_mult2_bwd");
}

int rcx_linear_attention_fwd(const void* qpre, const void* kpre, const void* v, const void* pe, void* out,
                             int B, int n, int C, int heads, int dtype, void* stream)
{
    if (!qpre || !kpre || !v || !pe || !out) return fail(RCX_ERR_BAD_ARG, "rcx_linear_attention_fwd: null pointer");
    if (B <= 0 || n <= 0 || C <= 0 || heads <= 0) return fail(RCX_ERR_BAD_ARG, "non-positive extent B=%d n=%d C=%d heads=%d", B, n, C, heads);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    if (C % heads) return fail(RCX_ERR_BAD_ARG, "C=%d is not a multiple of heads=%d", C, heads);
    const int D = C / heads;
    if (D > 64 || (D % 4 != 0 && D > 32)) return fail(RCX_ERR_UNSUPPORTED, "head dimension %d not supported (at most 64; at most 32 unless a multiple of 4)", D);
    hipError_t e = rcx::linattn_core(qpre, kpre, v, pe, out, B, n, C, heads, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_linear_attention_fwd");
}

int rcx_linear_attention_pe_fwd(const void* qpre, const void* kpre, const void* v, const float* w_pe_kkc, const float* b_pe, void* out,
                                int B, int H, int W, int C, int heads, int dtype, void* stream)
{
    if (!qpre || !kpre || !v || !w_pe_kkc || !out) return fail(RCX_ERR_BAD_ARG, "rcx_linear_attention_pe_fwd: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0) return fail(RCX_ERR_BAD_ARG, "non-positive extent B=%d H=%d W=%d C=%d heads=%d", B, H, W, C, heads);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    if (C % heads) return fail(RCX_ERR_BAD_ARG, "C=%d is not a multiple of heads=%d", C, heads);
    const int D = C / heads;
    if (D > 64 || !rcx::linattn_core_fuses_pe(H * W, C, heads, dtype))
        return fail(RCX_ERR_UNSUPPORTED, "head dimension %d, %d tokens: the fused form exists on the vector-pipe kernel of head dimensions that are multiples of "
                                         "four, at most 64 (use rcx_dwconv2d_fwd + rcx_linear_attention_fwd)", D, H * W);
    hipError_t e = rcx::linattn_core(qpre, kpre, v, nullptr, out, B, H * W, C, heads, dtype, (hipStream_t)stream, w_pe_kkc, b_pe, W);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_linear_attention_pe_fwd");
}

int rcx_recattn_qkcore_launches(int B, int H, int W, int C, int heads)
{
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0 || C % heads) return 0;
    return rcx::recattn_qkcore_launches(B, H, W, C, heads);
}

size_t rcx_recattn_qkcore_workspace_bytes(int B, int H, int W, int C, int heads)
{
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0 || C % heads) return 0;
    return rcx::recattn_qkcore_workspace_bytes(B, H, W, C, heads);
}

int rcx_recattn_qkcore_fwd(const float* d, const void* wqk_bf16, const float* bqk, const float* w_pe_kkc, const float* b_pe, float* out,
                           void* workspace, size_t workspace_bytes, int B, int H, int W, int C, int heads, void* stream)
{
    if (!d || !wqk_bf16 || !bqk || !w_pe_kkc || !out) return fail(RCX_ERR_BAD_ARG, "rcx_recattn_qkcore_fwd: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0) return fail(RCX_ERR_BAD_ARG, "non-positive extent B=%d H=%d W=%d C=%d heads=%d", B, H, W, C, heads);
    if (C % heads) return fail(RCX_ERR_BAD_ARG, "C=%d is not a multiple of heads=%d", C, heads);
    if (((size_t)d & 15) || ((size_t)wqk_bf16 & 15) || ((size_t)out & 15) || ((size_t)bqk & 15) || ((size_t)w_pe_kkc & 15) || ((size_t)b_pe & 15))
        return fail(RCX_ERR_BAD_ARG, "rcx_recattn_qkcore_fwd: d, wqk, bqk, w_pe_kkc, b_pe and out must be 16-byte aligned");
    if (!rcx::recattn_qkcore_applicable(B, H, W, C, heads))
        return fail(RCX_ERR_UNSUPPORTED, "rcx_recattn_qkcore_fwd: head dimension %d, %d heads, %d tokens, C=%d: the matrix-core form takes 32-wide heads, 1, 2, 4, 8 or "
                                         "16 of them (16 only on planes of at most 32 tokens), heads of 4 .. 28 channels in fours (an even count), or of 36 .. 64 "
                                         "in fours (2, 4 or 8 heads), where the LDS holds the plane (rcx_recattn_qkcore_launches; use the projection GEMMs + "
                                         "rcx_linear_attention_pe_fwd)", C / heads, heads, H * W, C);
    const size_t need = rcx::recattn_qkcore_workspace_bytes(B, H, W, C, heads);
    if (need && (!workspace || workspace_bytes < need || ((size_t)workspace & 15)))
        return fail(RCX_ERR_WORKSPACE, "rcx_recattn_qkcore_fwd: needs a 16-byte-aligned workspace of %zu bytes, got %zu", need, workspace ? workspace_bytes : (size_t)0);
    hipError_t e = rcx::recattn_qkcore(d, wqk_bf16, bqk, w_pe_kkc, b_pe, out, workspace, B, H, W, C, heads, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_recattn_qkcore_fwd");
}

int rcx_recattn_down_qkcore_supported(int B, int H, int W, int C, int heads, int x_dtype)
{
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0 || C % heads) return 0;
    return rcx::recattn_down_qkcore_applicable(B, H, W, C, heads, x_dtype) ? 1 : 0;
}

int rcx_recattn_down_qkcore_fwd(const void* x, const float* w_down_kkc, const float* b_down, const void* wqk_bf16, const float* bqk,
                                const float* w_pe_kkc, const float* b_pe, float* out, int B, int H, int W, int C, int heads, int x_dtype, void* stream)
{
    if (!x || !w_down_kkc || !wqk_bf16 || !bqk || !w_pe_kkc || !out) return fail(RCX_ERR_BAD_ARG, "rcx_recattn_down_qkcore_fwd: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0) return fail(RCX_ERR_BAD_ARG, "non-positive extent B=%d H=%d W=%d C=%d heads=%d", B, H, W, C, heads);
    if (C % heads) return fail(RCX_ERR_BAD_ARG, "C=%d is not a multiple of heads=%d", C, heads);
    if (!known_dtype(x_dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", x_dtype);
    if (((size_t)wqk_bf16 & 15) || ((size_t)out & 15) || ((size_t)bqk & 15) || ((size_t)w_pe_kkc & 15) || ((size_t)b_pe & 15))
        return fail(RCX_ERR_BAD_ARG, "rcx_recattn_down_qkcore_fwd: wqk, bqk, w_pe_kkc, b_pe and out must be 16-byte aligned");
    if (!rcx::recattn_down_qkcore_applicable(B, H, W, C, heads, x_dtype))
        return fail(RCX_ERR_UNSUPPORTED, "rcx_recattn_down_qkcore_fwd: %d x %d plane, %d heads of %d, dtype %d: the one-launch form takes the 14 x 14 plane (1 .. 8 heads) "
                                         "and the 7 x 7 plane (1 .. 16 heads) of bf16 / f16 activations, heads of 4 .. 32 channels, or 2, 4 or 8 heads of 36 .. 64 in fours "
                                         "whose image fits the LDS (use rcx_dwconv2d_fwd + rcx_recattn_qkcore_fwd)",
                    H, W, heads, C / heads, x_dtype);
    hipError_t e = rcx::recattn_down_qkcore(x, w_down_kkc, b_down, wqk_bf16, bqk, w_pe_kkc, b_pe, out, B, H, C, heads, x_dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_recattn_down_qkcore_fwd");
}

int rcx_recattn2d_fwd_supported(int B, int H, int W, int C, int heads, int mode, int dtype)
{
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0 || C % heads) return 0;
    return rcx::recattn2d_unit_applicable(B, H, W, C, heads, dtype, mode == RCX_MODE_NEAREST ? 1 : 0) ? 1 : 0;
}

int rcx_recattn2d_fwd(const void* x, void* y, const float* w_down_kkc, const float* b_down, const void* wqk_bf16, const float* bqk,
                      const float* w_pe_kkc, const float* b_pe, const float* w_conv_kkc, const float* b_conv,
                      int B, int H, int W, int C, int heads, int mode, int dtype, void* stream)
{
    if (!x || !y || !w_down_kkc || !wqk_bf16 || !bqk || !w_pe_kkc || !w_conv_kkc) return fail(RCX_ERR_BAD_ARG, "rcx_recattn2d_fwd: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0) return fail(RCX_ERR_BAD_ARG, "non-positive extent B=%d H=%d W=%d C=%d heads=%d", B, H, W, C, heads);
    if (C % heads) return fail(RCX_ERR_BAD_ARG, "C=%d is not a multiple of heads=%d", C, heads);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    if (mode != RCX_MODE_BILINEAR && mode != RCX_MODE_NEAREST) return fail(RCX_ERR_BAD_ARG, "unknown mode %d", mode);
    if (((size_t)wqk_bf16 & 15) || ((size_t)bqk & 15) || ((size_t)w_pe_kkc & 15) || ((size_t)b_pe & 15))
        return fail(RCX_ERR_BAD_ARG, "rcx_recattn2d_fwd: wqk, bqk, w_pe_kkc and b_pe must be 16-byte aligned");
    if (!rcx::recattn2d_unit_applicable(B, H, W, C, heads, dtype, mode == RCX_MODE_NEAREST ? 1 : 0))
        return fail(RCX_ERR_UNSUPPORTED, "rcx_recattn2d_fwd: %d x %d plane, %d heads of %d, mode %d, dtype %d: the one-launch unit takes the 14 x 14 (1 .. 8 heads) and 7 x 7 (1 .. 16 heads) planes of bf16 / f16 "
                                         "activations, heads of 32 or 4 .. 28 channels (not above 32), nearest resize (use rcx_recattn_down_qkcore_fwd / rcx_dwconv2d_fwd + rcx_recattn_qkcore_fwd, then "
                                         "rcx_upadd_dwconv_fwd)", H, W, heads, C / heads, mode, dtype);
    hipError_t e = rcx::recattn2d_unit(x, w_down_kkc, b_down, wqk_bf16, bqk, w_pe_kkc, b_pe, w_conv_kkc, b_conv, y, B, H, C, heads, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_recattn2d_fwd");
}

int rcx_stem_supported(int N, int H, int W, int CM, int CO, int dtype) { return rcx::stem_applicable(N, H, W, CM, CO, dtype) ? 1 : 0; }

size_t rcx_stem_pack_bytes(int CM, int CO) { return rcx::stem_pack_bytes(CM, CO); }

int rcx_stem_fwd(const void* x, void* y, const void* w1frag, const float* b1, const void* w2frag, const float* b2, int N, int H, int W, int CM, int CO, int dtype, void* stream)
{
    if (!x || !y || !w1frag || !b1 || !w2frag || !b2) return fail(RCX_ERR_BAD_ARG, "rcx_stem_fwd: null pointer");
    if (N <= 0 || H <= 0 || W <= 0 || CM <= 0 || CO <= 0) return fail(RCX_ERR_BAD_ARG, "non-positive extent N=%d H=%d W=%d CM=%d CO=%d", N, H, W, CM, CO);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    if (((size_t)x & 1) || ((size_t)y & 7) || ((size_t)w1frag & 15) || ((size_t)b1 & 15) || ((size_t)w2frag & 15) || ((size_t)b2 & 15))
        return fail(RCX_ERR_BAD_ARG, "rcx_stem_fwd: w1frag, b1, w2frag and b2 must be 16-byte aligned, y 8-byte aligned");
    if (!rcx::stem_applicable(N, H, W, CM, CO, dtype))
        return fail(RCX_ERR_UNSUPPORTED, "rcx_stem_fwd: no kernel for CM=%d CO=%d dtype %d (bf16; CM in {20, 24, 28, 32, 40}, CO %% 4 == 0, CO <= 96; one image of x below 2^31 bytes)", CM, CO, dtype);
    hipError_t e = rcx::stem_fwd(x, y, w1frag, b1, w2frag, b2, N, H, W, CM, CO, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_stem_fwd");
}

// The T / S / B stem (lsnet/model/recattn.py:208-223): front launch (rcx_stem.hip) into the workspace, tail launch (rcx_conv3s2.hip) out of it.
namespace {
bool stem3_shape(int N, int H, int W, int C, int final_act, int dtype)
{
    if (dtype != RCX_DTYPE_BF16 || N <= 0 || H <= 0 || W <= 0 || (C != 64 && C != 128) || (final_act != 0 && final_act != 1)) return false;
    if ((unsigned long long)H * W * 6 >= (1ull << 31)) return false;
    const long long h2 = ((H + 1) / 2 + 1) / 2, w2 = ((W + 1) / 2 + 1) / 2;
    return (long long)N * h2 * w2 <= 0x7fffffffLL / 64;                              // tile and pixel counts of both launches stay ints
}
bool any_misaligned(std::initializer_list<const void*> ps)
{
    for (const void* p : ps)
        if ((size_t)p & 15) return true;
    return false;
}
bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
}
}  // namespace

int rcx_stem3_supported(int N, int H, int W, int C, int final_act, int dtype) { return stem3_shape(N, H, W, C, final_act, dtype) ? 1 : 0; }

size_t rcx_stem3_pack_bytes(int C, int conv)
{
    if (C != 64 && C != 128) return 0;
    if (conv == 1) return 2048;                                                      // K = 27 padded to 32, C / 4 <= 32 channels padded to 32
    if (conv == 2) return (size_t)(C / 64) * 9 * ((C / 4 + 15) / 16) * 1024;          // C / 2 = 32 | 64 output channels, C / 4 = 16 | 32 input channels
    if (conv == 3) return (size_t)(C / 32) * 9 * (C / 32) * 1024;                     // C output channels, C / 2 input channels
    return 0;
}

size_t rcx_stem3_workspace_bytes(int N, int H, int W, int C)
{
    if (N <= 0 || H <= 0 || W <= 0 || (C != 64 && C != 128)) return 0;
    return (size_t)N * (size_t)(((H + 1) / 2 + 1) / 2) * (size_t)(((W + 1) / 2 + 1) / 2) * (size_t)(C / 2) * 2;
}

int rcx_stem3_fwd(const void* x, void* y, const void* w1frag, const float* b1, const void* w2frag, const float* b2, const void* w3frag, const float* b3,
                  void* workspace, size_t workspace_bytes, int N, int H, int W, int C, int final_act, int dtype, void* stream)
{
    if (!x || !y || !w1frag || !b1 || !w2frag || !b2 || !w3frag || !b3 || !workspace) return fail(RCX_ERR_BAD_ARG, "rcx_stem3_fwd: null pointer");
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(RCX_ERR_BAD_ARG, "non-positive extent N=%d H=%d W=%d C=%d", N, H, W, C);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    if (final_act != 0 && final_act != 1) return fail(RCX_ERR_BAD_ARG, "rcx_stem3_fwd: final_act must be 0 or 1, got %d", final_act);
    if (((size_t)x & 1) || any_misaligned({y, workspace, w1frag, b1, w2frag, b2, w3frag, b3}))
        return fail(RCX_ERR_BAD_ARG, "rcx_stem3_fwd: y, workspace and the six packs must be 16-byte aligned, x 2-byte aligned");
    if (!stem3_shape(N, H, W, C, final_act, dtype))
        return fail(RCX_ERR_UNSUPPORTED, "rcx_stem3_fwd: no kernel for C=%d dtype %d (bf16; C = 64 | 128; one image of x below 2^31 bytes)", C, dtype);
    const size_t need = rcx_stem3_workspace_bytes(N, H, W, C), xbytes = (size_t)N * H * W * 6;
    const size_t ybytes = (size_t)N * (size_t)((((H + 1) / 2 + 1) / 2 + 1) / 2) * (size_t)((((W + 1) / 2 + 1) / 2 + 1) / 2) * (size_t)C * 2;
    if (overlap(y, ybytes, x, xbytes) || overlap(workspace, workspace_bytes, x, xbytes) || overlap(workspace, workspace_bytes, y, ybytes))
        return fail(RCX_ERR_BAD_ARG, "rcx_stem3_fwd: y and the workspace must overlap neither x nor each other");
    if (workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "rcx_stem3_fwd: needs a workspace of %zu bytes, got %zu", need, workspace_bytes);
    hipError_t e = rcx::stem_front_fwd(x, workspace, w1frag, b1, w2frag, b2, N, H, W, C / 4, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "rcx_stem3_fwd (front)");
    e = rcx::conv3s2_fwd(workspace, y, w3frag, b3, N, ((H + 1) / 2 + 1) / 2, ((W + 1) / 2 + 1) / 2, C / 2, final_act, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_stem3_fwd (tail)");
}

int rcx_channel_mlp_supported(int M, int C, int H, int dtype) { return rcx::channel_mlp_applicable(M, C, H, dtype) ? 1 : 0; }

size_t rcx_channel_mlp_pack_bytes(int C, int H) { return rcx::channel_mlp_pack_bytes(C, H); }

int rcx_channel_mlp_fwd(const void* z, const void* x, void* y, const void* wfrag, const float* bias, int M, int C, int H, int dtype, void* stream)
{
    if (!z || !x || !y || !wfrag || !bias) return fail(RCX_ERR_BAD_ARG, "rcx_channel_mlp_fwd: null pointer");
    if (M <= 0 || C <= 0 || H <= 0) return fail(RCX_ERR_BAD_ARG, "non-positive extent M=%d C=%d H=%d", M, C, H);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    if (((size_t)z & 15) || ((size_t)x & 7) || ((size_t)y & 7) || ((size_t)wfrag & 15) || ((size_t)bias & 15))
        return fail(RCX_ERR_BAD_ARG, "rcx_channel_mlp_fwd: z, wfrag and bias must be 16-byte aligned, x and y 8-byte aligned");
    if (y == z || y == x) return fail(RCX_ERR_BAD_ARG, "rcx_channel_mlp_fwd: y must not alias its inputs");
    if (!rcx::channel_mlp_applicable(M, C, H, dtype))
        return fail(RCX_ERR_UNSUPPORTED, "rcx_channel_mlp_fwd: no kernel for M=%d C=%d H=%d dtype %d (bf16; (C, H) = (40 | 48, 96), (56 | 64, 128), (80, 160), (96, 192), (128, 256), (160, 320), "
                                         "(192, 384), (256, 512), (320, 640), and (384, 768), (512, 768), (512, 1024) each from a minimum M upward; M C 2 < 2^31)", M, C, H, dtype);
    hipError_t e = rcx::channel_mlp(z, x, y, wfrag, bias, M, C, H, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_channel_mlp_fwd");
}

int rcx_ls_recattn_supported(int B, int H, int W, int C, int split, int heads, int dtype)
{
    return rcx::ls_recattn_applicable(B, H, W, C, split, heads, dtype) ? 1 : 0;
}

int rcx_ls_la3_supported(int B, int H, int W, int C, int split, int heads, int dtype)
{
    return rcx::ls_la3_applicable(B, H, W, C, split, heads, dtype) ? 1 : 0;
}

int rcx_ls_recattn_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const float* w_down_kkc, const float* b_down,
                       const float* wqT, const float* bq, const float* wkT, const float* bk, const float* w_pe_kkc, const float* b_pe,
                       const float* w_conv_kkc, const float* b_conv, int B, int H, int W, int C, int split, int heads, int dtype, void* stream)
{
    if (!x || !r || !t || !w_rep || !b_rep || !w_down_kkc || !b_down || !wqT || !bq || !wkT || !bk || !w_pe_kkc || !b_pe || !w_conv_kkc || !b_conv)
        return fail(RCX_ERR_BAD_ARG, "rcx_ls_recattn_fwd: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || split <= 0 || heads <= 0)
        return fail(RCX_ERR_BAD_ARG, "non-positive extent B=%d H=%d W=%d C=%d split=%d heads=%d", B, H, W, C, split, heads);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    if (r == x || t == x || r == t) return fail(RCX_ERR_BAD_ARG, "rcx_ls_recattn_fwd: r and t must alias neither x nor each other");
    if (any_misaligned({x, r, t, w_rep, b_rep, w_down_kkc, b_down, wqT, bq, wkT, bk, w_pe_kkc, b_pe, w_conv_kkc, b_conv}))
        return fail(RCX_ERR_BAD_ARG, "rcx_ls_recattn_fwd: every tensor must be 16-byte aligned");
    if (!rcx::ls_recattn_applicable(B, H, W, C, split, heads, dtype))
        return fail(RCX_ERR_UNSUPPORTED, "rcx_ls_recattn_fwd: %d x %d plane, C=%d, split=%d, %d heads: one head, C and split multiples of 4, and an image whose slice "
                                         "mixer fits the LDS", H, W, C, split, heads);
    hipError_t e = rcx::ls_recattn_fwd(x, r, t, w_rep, b_rep, w_down_kkc, b_down, wqT, bq, wkT, bk, w_pe_kkc, b_pe, w_conv_kkc, b_conv,
                                       B, H, W, C, split, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_ls_recattn_fwd");
}

int rcx_ls_la3_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const float* wqT, const float* bq,
                   const float* wkT, const float* bk, const float* w_pe_kkc, const float* b_pe, int B, int H, int W, int C, int split, int heads,
                   int dtype, void* stream)
{
    if (!x || !r || !t || !w_rep || !b_rep || !wqT || !bq || !wkT || !bk || !w_pe_kkc || !b_pe) return fail(RCX_ERR_BAD_ARG, "rcx_ls_la3_fwd: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || split <= 0 || heads <= 0)
        return fail(RCX_ERR_BAD_ARG, "non-positive extent B=%d H=%d W=%d C=%d split=%d heads=%d", B, H, W, C, split, heads);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    if (r == x || t == x || r == t) return fail(RCX_ERR_BAD_ARG, "rcx_ls_la3_fwd: r and t must alias neither x nor each other");
    if (any_misaligned({x, r, t, w_rep, b_rep, wqT, bq, wkT, bk, w_pe_kkc, b_pe}))
        return fail(RCX_ERR_BAD_ARG, "rcx_ls_la3_fwd: every tensor must be 16-byte aligned");
    if (!rcx::ls_la3_applicable(B, H, W, C, split, heads, dtype))
        return fail(RCX_ERR_UNSUPPORTED, "rcx_ls_la3_fwd: %d x %d plane, C=%d, split=%d, %d heads: at most 64 tokens, C and split multiples of 4, split a multiple "
                                         "of 2 heads", H, W, C, split, heads);
    hipError_t e = rcx::ls_la3_fwd(x, r, t, w_rep, b_rep, wqT, bq, wkT, bk, w_pe_kkc, b_pe, B, H, W, C, split, heads, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_ls_la3_fwd");
}

int rcx_ls_recattn_tiled_supported(int B, int H, int W, int C, int split, int heads, int dtype)
{
    return rcx::ls_recattn_tiled_applicable(B, H, W, C, split, heads, dtype) ? 1 : 0;
}

int rcx_ls_la3_tiled_supported(int B, int H, int W, int C, int split, int heads, int dtype)
{
    return rcx::ls_la3_tiled_applicable(B, H, W, C, split, heads, dtype) ? 1 : 0;
}

size_t rcx_ls_recattn_tiled_workspace_bytes(int B, int H, int W, int C, int split, int heads, int dtype)
{
    return rcx::ls_recattn_tiled_workspace_bytes(B, H, W, C, split, heads, dtype);
}

size_t rcx_ls_la3_tiled_workspace_bytes(int B, int H, int W, int C, int split, int heads, int dtype)
{
    return rcx::ls_la3_tiled_workspace_bytes(B, H, W, C, split, heads, dtype);
}

namespace {
// the argument checks the two tiled token-half entries share, in the order of rcx_ls_recattn_fwd / rcx_ls_la3_fwd, then the workspace
int check_ls_tiled(const char* fn, std::initializer_list<const void*> ps, const void* x, const void* r, const void* t, const void* workspace,
                   size_t workspace_bytes, size_t need, bool supported, int B, int H, int W, int C, int split, int heads, int dtype)
{
    for (const void* p : ps)
        if (!p) return fail(RCX_ERR_BAD_ARG, "%s: null pointer", fn);
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || split <= 0 || heads <= 0)
        return fail(RCX_ERR_BAD_ARG, "non-positive extent B=%d H=%d W=%d C=%d split=%d heads=%d", B, H, W, C, split, heads);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    if (r == x || t == x || r == t) return fail(RCX_ERR_BAD_ARG, "%s: r and t must alias neither x nor each other", fn);
    if (workspace && (workspace == x || workspace == r || workspace == t)) return fail(RCX_ERR_BAD_ARG, "%s: the workspace must alias none of x, r and t", fn);
    if (any_misaligned(ps) || ((size_t)workspace & 15)) return fail(RCX_ERR_BAD_ARG, "%s: every tensor and the workspace must be 16-byte aligned", fn);
    if (!supported)
        return fail(RCX_ERR_UNSUPPORTED, "%s: %d x %d plane, C=%d, split=%d, %d heads: C and split multiples of 4; RecAttn2d one head, LinearAttention3 split a "
                                         "multiple of 2 heads with heads of v in fours; a chunk's LDS within 160 KB", fn, H, W, C, split, heads);
    if (!workspace || workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    return 0;
}
}  // namespace

int rcx_ls_recattn_tiled_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const float* w_down_kkc, const float* b_down,
                             const float* wqT, const float* bq, const float* wkT, const float* bk, const float* w_pe_kkc, const float* b_pe,
                             const float* w_conv_kkc, const float* b_conv, void* workspace, size_t workspace_bytes, int B, int H, int W, int C,
                             int split, int heads, int dtype, void* stream)
{
    if (int rc = check_ls_tiled("rcx_ls_recattn_tiled_fwd", {x, r, t, w_rep, b_rep, w_down_kkc, b_down, wqT, bq, wkT, bk, w_pe_kkc, b_pe, w_conv_kkc, b_conv},
                                x, r, t, workspace, workspace_bytes, rcx::ls_recattn_tiled_workspace_bytes(B, H, W, C, split, heads, dtype),
                                rcx::ls_recattn_tiled_applicable(B, H, W, C, split, heads, dtype), B, H, W, C, split, heads, dtype))
        return rc;
    hipError_t e = rcx::ls_recattn_tiled_fwd(x, r, t, w_rep, b_rep, w_down_kkc, b_down, wqT, bq, wkT, bk, w_pe_kkc, b_pe, w_conv_kkc, b_conv, workspace,
                                             B, H, W, C, split, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_ls_recattn_tiled_fwd");
}

int rcx_ls_la3_tiled_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const float* wqT, const float* bq,
                         const float* wkT, const float* bk, const float* w_pe_kkc, const float* b_pe, void* workspace, size_t workspace_bytes,
                         int B, int H, int W, int C, int split, int heads, int dtype, void* stream)
{
    if (int rc = check_ls_tiled("rcx_ls_la3_tiled_fwd", {x, r, t, w_rep, b_rep, wqT, bq, wkT, bk, w_pe_kkc, b_pe}, x, r, t, workspace, workspace_bytes,
                                rcx::ls_la3_tiled_workspace_bytes(B, H, W, C, split, heads, dtype),
                                rcx::ls_la3_tiled_applicable(B, H, W, C, split, heads, dtype), B, H, W, C, split, heads, dtype))
        return rc;
    hipError_t e = rcx::ls_la3_tiled_fwd(x, r, t, w_rep, b_rep, wqT, bq, wkT, bk, w_pe_kkc, b_pe, workspace, B, H, W, C, split, heads, dtype,
                                         (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_ls_la3_tiled_fwd");
}

int rcx_grouped_conv2d_supported(int N, int H, int W, int Cin, int Cout, int groups, int k, int stride, int dtype)
{
    return rcx::ls_down_applicable(N, H, W, Cin, Cout, groups, k, stride, dtype) ? 1 : 0;
}

int rcx_grouped_conv2d_fwd(const void* x, void* y, const float* wpack, const float* bias, int N, int H, int W, int Cin, int Cout, int groups, int k,
                           int stride, int dtype, void* stream)
{
    if (!x || !y || !wpack) return fail(RCX_ERR_BAD_ARG, "rcx_grouped_conv2d_fwd: null pointer");
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || groups <= 0)
        return fail(RCX_ERR_BAD_ARG, "rcx_grouped_conv2d_fwd: non-positive extent N=%d H=%d W=%d Cin=%d Cout=%d groups=%d", N, H, W, Cin, Cout, groups);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "rcx_grouped_conv2d_fwd: unknown dtype %d", dtype);
    if (y == x || (const void*)wpack == x || (const void*)wpack == y || (bias && ((const void*)bias == x || (const void*)bias == y)))
        return fail(RCX_ERR_BAD_ARG, "rcx_grouped_conv2d_fwd: y must alias neither x nor a pack");
    const size_t es = dtype == RCX_DTYPE_F32 ? 4 : 2;
    if ((size_t)x % es || (size_t)y % es || (size_t)wpack % 4 || (size_t)bias % 4)
        return fail(RCX_ERR_BAD_ARG, "rcx_grouped_conv2d_fwd: x and y must be aligned to one element (%zu bytes), the packs to 4 bytes", es);
    if (!rcx::ls_down_applicable(N, H, W, Cin, Cout, groups, k, stride, dtype))
        return fail(RCX_ERR_UNSUPPORTED, "rcx_grouped_conv2d_fwd: Cin=%d, Cout=%d, groups=%d, k=%d, stride=%d: k = 5, stride = 2, groups dividing Cin and Cout, "
                                         "1 .. 4 channels a group in and out, fewer than 2^31 elements in x and in y", Cin, Cout, groups, k, stride);
    hipError_t e = rcx::ls_down_fwd(x, y, wpack, bias, N, H, W, Cin, Cout, groups, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_grouped_conv2d_fwd");
}

int rcx_grouped_conv2d_bwd_supported(int N, int H, int W, int Cin, int Cout, int groups, int k, int stride, int dtype)
{
    return rcx::ls_down_bwd_applicable(N, H, W, Cin, Cout, groups, k, stride, dtype) ? 1 : 0;
}

size_t rcx_grouped_conv2d_bwd_workspace_bytes(int N, int H, int W, int Cin, int Cout, int groups, int k, int stride, int dtype)
{
    return rcx::ls_down_bwd_workspace_bytes(N, H, W, Cin, Cout, groups, k, stride, dtype);
}

int rcx_grouped_conv2d_bwd(const void* x, const void* gy, const float* wpack, void* gx, float* gwpack, float* gb, void* workspace, size_t workspace_bytes,
                           int N, int H, int W, int Cin, int Cout, int groups, int k, int stride, int dtype, void* stream)
{
    if (!x || !gy || !wpack) return fail(RCX_ERR_BAD_ARG, "rcx_grouped_conv2d_bwd: null pointer");
    if (!gx && !gwpack && !gb) return fail(RCX_ERR_BAD_ARG, "rcx_grouped_conv2d_bwd: null pointer for every output (gx, gwpack and gb)");
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || groups <= 0)
        return fail(RCX_ERR_BAD_ARG, "rcx_grouped_conv2d_bwd: non-positive extent N=%d H=%d W=%d Cin=%d Cout=%d groups=%d", N, H, W, Cin, Cout, groups);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "rcx_grouped_conv2d_bwd: unknown dtype %d", dtype);
    {
        const void* in[3] = {x, gy, wpack};
        const void* out[4] = {gx, gwpack, gb, workspace};
        for (int i = 0; i < 4; ++i) {
            if (!out[i]) continue;
            for (int j = 0; j < 3; ++j)
                if (out[i] == in[j]) return fail(RCX_ERR_BAD_ARG, "rcx_grouped_conv2d_bwd: gx, gwpack, gb and the workspace must alias no input");
            for (int j = i + 1; j < 4; ++j)
                if (out[i] == out[j]) return fail(RCX_ERR_BAD_ARG, "rcx_grouped_conv2d_bwd: gx, gwpack, gb and the workspace must not alias each other");
        }
    }
    const size_t es = dtype == RCX_DTYPE_F32 ? 4 : 2;
    if ((size_t)x % es || (size_t)gy % es || (size_t)gx % es || (size_t)wpack % 4 || (size_t)gwpack % 4 || (size_t)gb % 4 || (size_t)workspace % 4)
        return fail(RCX_ERR_BAD_ARG, "rcx_grouped_conv2d_bwd: x, gy and gx must be aligned to one element (%zu bytes), the packs, gb and the workspace to 4 bytes", es);
    if (!rcx::ls_down_bwd_applicable(N, H, W, Cin, Cout, groups, k, stride, dtype))
        return fail(RCX_ERR_UNSUPPORTED, "rcx_grouped_conv2d_bwd: Cin=%d, Cout=%d, groups=%d, k=%d, stride=%d: k = 5, stride = 2, groups dividing Cin and Cout, "
                                         "1 .. 4 channels a group in and out, fewer than 2^31 elements in x and in gy", Cin, Cout, groups, k, stride);
    if (gwpack || gb) {
        const size_t need = rcx_grouped_conv2d_bwd_workspace_bytes(N, H, W, Cin, Cout, groups, k, stride, dtype);
        if (!workspace || workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, workspace ? workspace_bytes : (size_t)0);
    }
    hipError_t e = rcx::ls_down_bwd(x, gy, wpack, gx, gwpack, gb, workspace, N, H, W, Cin, Cout, groups, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_grouped_conv2d_bwd");
}

int rcx_ls_share_supported(int B, int H, int W, int C, int split, int n_src, int dtype)
{
    return rcx::ls_share_applicable(B, H, W, C, split, n_src, split, dtype) ? 1 : 0;
}

int rcx_ls_share_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const void* const* srcs, int n_src,
                     long long src_pixel_stride, int B, int H, int W, int C, int split, int dtype, void* stream)
{
    if (!x || !r || !t || !w_rep || !b_rep || !srcs) return fail(RCX_ERR_BAD_ARG, "rcx_ls_share_fwd: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || split <= 0 || n_src <= 0)
        return fail(RCX_ERR_BAD_ARG, "non-positive extent B=%d H=%d W=%d C=%d split=%d n_src=%d", B, H, W, C, split, n_src);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    if (r == x || t == x || r == t) return fail(RCX_ERR_BAD_ARG, "rcx_ls_share_fwd: r and t must alias neither x nor each other");
    const size_t align = dtype == RCX_DTYPE_F32 ? 16 : 8;           // four elements, as check_wide
    if ((size_t)x % align || (size_t)r % align || (size_t)t % align || any_misaligned({w_rep, b_rep}))
        return fail(RCX_ERR_BAD_ARG, "rcx_ls_share_fwd: x, r and t must be aligned to four elements (%zu bytes), the packs to 16 bytes", align);
    for (int j = 0; j < n_src; ++j) {
        if (!srcs[j]) return fail(RCX_ERR_BAD_ARG, "rcx_ls_share_fwd: null source %d", j);
        if ((size_t)srcs[j] % align) return fail(RCX_ERR_BAD_ARG, "rcx_ls_share_fwd: source %d must be aligned to four elements (%zu bytes)", j, align);
        if (srcs[j] == r || srcs[j] == t) return fail(RCX_ERR_BAD_ARG, "rcx_ls_share_fwd: r and t must not alias source %d", j);
    }
    if (!rcx::ls_share_applicable(B, H, W, C, split, n_src, src_pixel_stride, dtype))
        return fail(RCX_ERR_UNSUPPORTED, "rcx_ls_share_fwd: C=%d, split=%d, %d sources, pixel stride %lld: C, split and the stride multiples of 4, n_src * split "
                                         "== C, 1 .. %d sources, stride >= split, B*H*W*C < 2^31", C, split, n_src, src_pixel_stride, rcx::kLsShareMaxSrc);
    hipError_t e = rcx::ls_share_fwd(x, r, t, w_rep, b_rep, srcs, n_src, src_pixel_stride, B, H, W, C, split, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_ls_share_fwd");
}

int rcx_linear_attention_bwd(const void* qpre, const void* kpre, const void* v, const void* gout, void* gq, void* gk, void* gv,
                             int B, int n, int C, int heads, int dtype, void* stream)
{
    if (!qpre || !kpre || !v || !gout || !gq || !gk || !gv) return fail(RCX_ERR_BAD_ARG, "rcx_linear_attention_bwd: null pointer");
    if (B <= 0 || n <= 0 || C <= 0 || heads <= 0) return fail(RCX_ERR_BAD_ARG, "non-positive extent B=%d n=%d C=%d heads=%d", B, n, C, heads);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "unknown dtype %d", dtype);
    if (C % heads) return fail(RCX_ERR_BAD_ARG, "C=%d is not a multiple of heads=%d", C, heads);
    if (C / heads > 64) return fail(RCX_ERR_UNSUPPORTED, "head dimension %d not supported (at most 64)", C / heads);
    hipError_t e = rcx::linattn_core_bwd(qpre, kpre, v, gout, gq, gk, gv, B, n, C, heads, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_linear_attention_bwd");
}

int rcx_linear_attention_wide_supported(int B, int n, int Cqk, int Cv, int heads, int dtype)
{
    return rcx::linattn_wide_applicable(B, n, Cqk, Cv, heads, dtype) ? 1 : 0;
}

namespace {
// the argument checks shared by the wide core's two entries: every pointer non-NULL and aligned to four elements of `dtype`
int check_wide(const char* fn, std::initializer_list<const void*> ps, int B, int n, int Cqk, int Cv, int heads, int dtype)
{
    for (const void* p : ps)
        if (!p) return fail(RCX_ERR_BAD_ARG, "%s: null pointer", fn);
    if (B <= 0 || n <= 0 || Cqk <= 0 || Cv <= 0 || heads <= 0)
        return fail(RCX_ERR_BAD_ARG, "%s: non-positive extent B=%d n=%d Cqk=%d Cv=%d heads=%d", fn, B, n, Cqk, Cv, heads);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "%s: unknown dtype %d", fn, dtype);
    if (Cqk % heads || Cv % heads) return fail(RCX_ERR_BAD_ARG, "%s: Cqk=%d and Cv=%d must be multiples of heads=%d", fn, Cqk, Cv, heads);
    const size_t align = dtype == RCX_DTYPE_F32 ? 16 : 8;
    for (const void* p : ps)
        if ((size_t)p % align) return fail(RCX_ERR_BAD_ARG, "%s: every tensor must be aligned to four elements (%zu bytes)", fn, (size_t)align);
    if (!rcx::linattn_wide_applicable(B, n, Cqk, Cv, heads, dtype))
        return fail(RCX_ERR_UNSUPPORTED, "%s: heads of %d (q / k) x %d (v) channels: both must be multiples of 4 from 4 to 128", fn, Cqk / heads, Cv / heads);
    return 0;
}
}  // namespace

int rcx_linear_attention_wide_fwd(const void* qpre, const void* kpre, const void* v, const void* pe, void* out,
                                  int B, int n, int Cqk, int Cv, int heads, int dtype, void* stream)
{
    if (int rc = check_wide("rcx_linear_attention_wide_fwd", {qpre, kpre, v, pe, out}, B, n, Cqk, Cv, heads, dtype)) return rc;
    hipError_t e = rcx::linattn_wide_fwd(qpre, kpre, v, pe, out, B, n, Cqk, Cv, heads, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_linear_attention_wide_fwd");
}

int rcx_linear_attention_wide_bwd(const void* qpre, const void* kpre, const void* v, const void* gout, void* gq, void* gk, void* gv,
                                  int B, int n, int Cqk, int Cv, int heads, int dtype, void* stream)
{
    if (int rc = check_wide("rcx_linear_attention_wide_bwd", {qpre, kpre, v, gout, gq, gk, gv}, B, n, Cqk, Cv, heads, dtype)) return rc;
    hipError_t e = rcx::linattn_wide_bwd(qpre, kpre, v, gout, gq, gk, gv, B, n, Cqk, Cv, heads, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "rcx_linear_attention_wide_bwd");
}

// nn.BatchNorm2d on a dense NHWC tensor (rcx_bn.hip): batch statistics, frozen statistics and their backward
namespace {
struct Span { const void* p; size_t n; };

// the checks the three BatchNorm entries share, in the order the header gives: extents, dtype, alignment (x-like tensors to one element, everything else
// to a float), size, then every output against every input and every other output
int check_bn(const char* fn, int N, int H, int W, int C, int dtype, std::initializer_list<const void*> elems, std::initializer_list<const void*> floats,
             std::initializer_list<Span> ins, std::initializer_list<Span> outs)
{
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(RCX_ERR_BAD_ARG, "%s: non-positive extent N=%d H=%d W=%d C=%d", fn, N, H, W, C);
    if (!known_dtype(dtype)) return fail(RCX_ERR_BAD_ARG, "%s: unknown dtype %d", fn, dtype);
    const size_t es = dtype == RCX_DTYPE_F32 ? 4 : 2;
    for (const void* p : elems)
        if ((size_t)p % es) return fail(RCX_ERR_BAD_ARG, "%s: x-like tensors must be aligned to one element (%zu bytes)", fn, es);
    for (const void* p : floats)
        if ((size_t)p % 4) return fail(RCX_ERR_BAD_ARG, "%s: weight, bias, the statistics, the parameter gradients and the workspace must be aligned to 4 bytes", fn);
    if (!rcx::batchnorm_applicable(N, H, W, C, dtype))
        return fail(RCX_ERR_UNSUPPORTED, "%s: N=%d H=%d W=%d C=%d: 2^31 or more elements", fn, N, H, W, C);
    for (auto o = outs.begin(); o != outs.end(); ++o) {
        if (!o->p) continue;
        for (const Span& i : ins)
            if (i.p && overlap(o->p, o->n, i.p, i.n)) return fail(RCX_ERR_BAD_ARG, "%s: an output or the workspace aliases an input", fn);
        for (auto q = o + 1; q != outs.end(); ++q)
            if (q->p && overlap(o->p, o->n, q->p, q->n)) return fail(RCX_ERR_BAD_ARG, "%s: the outputs and the workspace must not alias each other", fn);
    }
    return 0;
}
}  // namespace

// what the kernels take: fewer than 2^31 elements.  Which of these shapes a model routes here is the binding's rule (recnext_amd/batchnorm.py)
int rcx_batchnorm_supported(int N, int H, int W, int C, int dtype)
{
    return rcx::batchnorm_applicable(N, H, W, C, dtype) ? 1 : 0;
}

size_t rcx_batchnorm_workspace_bytes(int N, int H, int W, int C, int dtype)
{
    if (!rcx::batchnorm_applicable(N, H, W, C, dtype)) return 0;
    return rcx::batchnorm_workspace_bytes(N * H * W, C, dtype);
}

int rcx_batchnorm_train_fwd(const void* x, void* y, const float* weight, const float* bias, float* running_mean, float* running_var, float* save_mean,
                            float* save_invstd, void* workspace, size_t workspace_bytes, int N, int H, int W, int C, float momentum, float eps, int dtype,
                            void* stream)
{
    const char* fn = "rcx_batchnorm_train_fwd";
    if (!x || !y || !weight || !bias || !save_mean || !save_invstd) return fail(RCX_ERR_BAD_ARG, "%s: null pointer", fn);
    if (!running_mean != !running_var) return fail(RCX_ERR_BAD_ARG, "%s: running_mean and running_var come together or not at all", fn);
    if (N > 0 && H > 0 && W > 0 && (long long)N * H * W == 1)
        return fail(RCX_ERR_BAD_ARG, "%s: batch statistics need more than one value per channel (N=%d H=%d W=%d)", fn, N, H, W);
    const size_t es = dtype == RCX_DTYPE_F32 ? 4 : 2, xb = (size_t)N * H * W * C * es, cb = (size_t)C * 4;
    if (int rc = check_bn(fn, N, H, W, C, dtype, {x, y}, {weight, bias, running_mean, running_var, save_mean, save_invstd, workspace},
                          {{x, xb}, {weight, cb}, {bias, cb}},
                          {{y, xb}, {running_mean, cb}, {running_var, cb}, {save_mean, cb}, {save_invstd, cb}, {workspace, workspace_bytes}}))
        return rc;
    const size_t need = rcx::batchnorm_workspace_bytes(N * H * W, C, dtype);
    if (!workspace || workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "%s: workspace too small: need %zu bytes, got %zu", fn, need, workspace ? workspace_bytes : (size_t)0);
    hipError_t e = rcx::batchnorm_train_fwd(x, y, weight, bias, running_mean, running_var, save_mean, save_invstd, workspace, N * H * W, C, momentum, eps, dtype,
                                            (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, fn);
}

int rcx_batchnorm_frozen_fwd(const void* x, void* y, const float* weight, const float* bias, const float* mean, const float* var, float* save_invstd, float eps,
                             int N, int H, int W, int C, int dtype, void* stream)
{
    const char* fn = "rcx_batchnorm_frozen_fwd";
    if (!x || !y || !weight || !bias || !mean || !var) return fail(RCX_ERR_BAD_ARG, "%s: null pointer", fn);
    const size_t es = dtype == RCX_DTYPE_F32 ? 4 : 2, xb = (size_t)N * H * W * C * es, cb = (size_t)C * 4;
    if (int rc = check_bn(fn, N, H, W, C, dtype, {x, y}, {weight, bias, mean, var, save_invstd}, {{x, xb}, {weight, cb}, {bias, cb}, {mean, cb}, {var, cb}},
                          {{y, xb}, {save_invstd, cb}}))
        return rc;
    hipError_t e = rcx::batchnorm_frozen_fwd(x, y, weight, bias, mean, var, save_invstd, N * H * W, C, eps, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, fn);
}

int rcx_batchnorm_bwd(const void* x, const void* gy, const float* weight, const float* mean, const float* invstd, void* gx, float* gweight, float* gbias,
                      void* workspace, size_t workspace_bytes, int N, int H, int W, int C, int batch_stats, int dtype, void* stream)
{
    const char* fn = "rcx_batchnorm_bwd";
    if (!x || !gy || !weight || !mean || !invstd) return fail(RCX_ERR_BAD_ARG, "%s: null pointer", fn);
    if (!gx && !gweight && !gbias) return fail(RCX_ERR_BAD_ARG, "%s: null pointer for every output (gx, gweight and gbias)", fn);
    if (!gweight != !gbias) return fail(RCX_ERR_BAD_ARG, "%s: gweight and gbias come together or not at all", fn);
    if (batch_stats != 0 && batch_stats != 1) return fail(RCX_ERR_BAD_ARG, "%s: batch_stats must be 0 or 1, got %d", fn, batch_stats);
    if (batch_stats && N > 0 && H > 0 && W > 0 && (long long)N * H * W == 1)
        return fail(RCX_ERR_BAD_ARG, "%s: batch statistics need more than one value per channel (N=%d H=%d W=%d)", fn, N, H, W);
    const size_t es = dtype == RCX_DTYPE_F32 ? 4 : 2, xb = (size_t)N * H * W * C * es, cb = (size_t)C * 4;
    if (int rc = check_bn(fn, N, H, W, C, dtype, {x, gy, gx}, {weight, mean, invstd, gweight, gbias, workspace},
                          {{x, xb}, {gy, xb}, {weight, cb}, {mean, cb}, {invstd, cb}}, {{gx, xb}, {gweight, cb}, {gbias, cb}, {workspace, workspace_bytes}}))
        return rc;
    if (batch_stats || gweight) {                                                  // the frozen form without parameter gradients launches no reduction
        const size_t need = rcx::batchnorm_workspace_bytes(N * H * W, C, dtype);
        if (!workspace || workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "%s: workspace too small: need %zu bytes, got %zu", fn, need, workspace ? workspace_bytes : (size_t)0);
    }
    hipError_t e = rcx::batchnorm_bwd(x, gy, weight, mean, invstd, gx, gweight, gbias, workspace, N * H * W, C, batch_stats != 0, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, fn);
}

// RepVGGDW of a training step as one operator (rcx_repdw.hip).  What it takes is what the BatchNorm kernels take: fewer than 2^31 elements.
int rcx_repdw_train_supported(int N, int H, int W, int C, int dtype)
{
    return rcx::batchnorm_applicable(N, H, W, C, dtype) ? 1 : 0;
}

size_t rcx_repdw_train_workspace_bytes(int N, int H, int W, int C, int dtype)
{
    if (!rcx::batchnorm_applicable(N, H, W, C, dtype)) return 0;
    return rcx::repdw_train_workspace_bytes(N * H * W, C, dtype);
}

int rcx_repdw_train_fwd(const void* x, float* r, const float* w3, const float* b3, const float* gamma_a, const float* beta_a, const float* w1, const float* b1,
                        const float* gamma_b, const float* beta_b, float* lk_running_mean, float* lk_running_var, float* sk_running_mean, float* sk_running_var,
                        float* save_mean_x, float* save_var_x, float* save_mean_u, float* save_invstd_u, void* workspace, size_t workspace_bytes,
                        int N, int H, int W, int C, float momentum_a, float eps_a, float momentum_b, float eps_b, int dtype, void* stream)
{
    const char* fn = "rcx_repdw_train_fwd";
    if (!x || !r || !w3 || !b3 || !gamma_a || !beta_a || !w1 || !b1 || !gamma_b || !beta_b || !save_mean_x || !save_var_x || !save_mean_u || !save_invstd_u)
        return fail(RCX_ERR_BAD_ARG, "%s: null pointer", fn);
    const int nrun = !!lk_running_mean + !!lk_running_var + !!sk_running_mean + !!sk_running_var;
    if (nrun != 0 && nrun != 4) return fail(RCX_ERR_BAD_ARG, "%s: the four running buffers come together or not at all", fn);
    if (N > 0 && H > 0 && W > 0 && (long long)N * H * W == 1)
        return fail(RCX_ERR_BAD_ARG, "%s: batch statistics need more than one value per channel (N=%d H=%d W=%d)", fn, N, H, W);
    const size_t es = dtype == RCX_DTYPE_F32 ? 4 : 2, xb = (size_t)N * H * W * C * es, rb = (size_t)N * H * W * C * 4, cb = (size_t)C * 4;
    if (int rc = check_bn(fn, N, H, W, C, dtype, {x},
                          {r, w3, b3, gamma_a, beta_a, w1, b1, gamma_b, beta_b, lk_running_mean, lk_running_var, sk_running_mean, sk_running_var, save_mean_x,
                           save_var_x, save_mean_u, save_invstd_u, workspace},
                          {{x, xb}, {w3, 9 * cb}, {b3, cb}, {gamma_a, cb}, {beta_a, cb}, {w1, cb}, {b1, cb}, {gamma_b, cb}, {beta_b, cb}},
                          {{r, rb}, {lk_running_mean, cb}, {lk_running_var, cb}, {sk_running_mean, cb}, {sk_running_var, cb}, {save_mean_x, cb}, {save_var_x, cb},
                           {save_mean_u, cb}, {save_invstd_u, cb}, {workspace, workspace_bytes}}))
        return rc;
    const size_t need = rcx::repdw_train_workspace_bytes(N * H * W, C, dtype);
    if (!workspace || workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "%s: workspace too small: need %zu bytes, got %zu", fn, need, workspace ? workspace_bytes : (size_t)0);
    hipError_t e = rcx::repdw_train_fwd(x, r, w3, b3, gamma_a, beta_a, w1, b1, gamma_b, beta_b, lk_running_mean, lk_running_var, sk_running_mean, sk_running_var,
                                        save_mean_x, save_var_x, save_mean_u, save_invstd_u, workspace, N, H, W, C, momentum_a, eps_a, momentum_b, eps_b, dtype,
                                        (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, fn);
}

int rcx_repdw_train_bwd(const void* x, const float* g, const float* w3, const float* b3, const float* gamma_a, const float* w1, const float* gamma_b,
                        const float* mean_x, const float* var_x, const float* mean_u, const float* invstd_u, void* gx, float* gw3, float* gb3, float* ggamma_a,
                        float* gbeta_a, float* gw1, float* gb1, float* ggamma_b, float* gbeta_b, void* workspace, size_t workspace_bytes,
                        int N, int H, int W, int C, float eps_b, int dtype, void* stream)
{
    const char* fn = "rcx_repdw_train_bwd";
    if (!x || !g || !w3 || !b3 || !gamma_a || !w1 || !gamma_b || !mean_x || !var_x || !mean_u || !invstd_u) return fail(RCX_ERR_BAD_ARG, "%s: null pointer", fn);
    const int npar = !!gw3 + !!gb3 + !!ggamma_a + !!gbeta_a + !!gw1 + !!gb1 + !!ggamma_b + !!gbeta_b;
    if (!gx && !npar) return fail(RCX_ERR_BAD_ARG, "%s: null pointer for every output (gx and the parameter gradients)", fn);
    if (npar != 0 && npar != 8) return fail(RCX_ERR_BAD_ARG, "%s: the eight parameter gradients come together or not at all", fn);
    if (N > 0 && H > 0 && W > 0 && (long long)N * H * W == 1)
        return fail(RCX_ERR_BAD_ARG, "%s: batch statistics need more than one value per channel (N=%d H=%d W=%d)", fn, N, H, W);
    const size_t es = dtype == RCX_DTYPE_F32 ? 4 : 2, xb = (size_t)N * H * W * C * es, rb = (size_t)N * H * W * C * 4, cb = (size_t)C * 4;
    if (int rc = check_bn(fn, N, H, W, C, dtype, {x, gx},
                          {g, w3, b3, gamma_a, w1, gamma_b, mean_x, var_x, mean_u, invstd_u, gw3, gb3, ggamma_a, gbeta_a, gw1, gb1, ggamma_b, gbeta_b, workspace},
                          {{x, xb}, {g, rb}, {w3, 9 * cb}, {b3, cb}, {gamma_a, cb}, {w1, cb}, {gamma_b, cb}, {mean_x, cb}, {var_x, cb}, {mean_u, cb}, {invstd_u, cb}},
                          {{gx, xb}, {gw3, 9 * cb}, {gb3, cb}, {ggamma_a, cb}, {gbeta_a, cb}, {gw1, cb}, {gb1, cb}, {ggamma_b, cb}, {gbeta_b, cb},
                           {workspace, workspace_bytes}}))
        return rc;
    const size_t need = rcx::repdw_train_workspace_bytes(N * H * W, C, dtype);
    if (!workspace || workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "%s: workspace too small: need %zu bytes, got %zu", fn, need, workspace ? workspace_bytes : (size_t)0);
    hipError_t e = rcx::repdw_train_bwd(x, g, w3, b3, gamma_a, w1, gamma_b, mean_x, var_x, mean_u, invstd_u, gx, gw3, gb3, ggamma_a, gbeta_a, gw1, gb1, ggamma_b,
                                        gbeta_b, workspace, N, H, W, C, eps_b, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, fn);
}

// A depthwise ConvNorm of a training step as one operator (rcx_dwbn.hip): k = 3 | 5, stride 1 | 2, the up-add form at stride 1 only, and what the
// BatchNorm kernels take: fewer than 2^31 elements.
int rcx_dwconv_bn_train_supported(int N, int H, int W, int C, int k, int stride, int has_coarse, int dtype)
{
    return rcx::dwconv_bn_train_applicable(N, H, W, C, k, stride, has_coarse, dtype) ? 1 : 0;
}

size_t rcx_dwconv_bn_train_workspace_bytes(int N, int H, int W, int C, int k, int stride, int has_coarse, int dtype)
{
    if (!rcx::dwconv_bn_train_applicable(N, H, W, C, k, stride, has_coarse, dtype)) return 0;
    return rcx::dwconv_bn_train_workspace_bytes(N, H, W, C, k, stride, dtype);
}

namespace {
// the checks the two entries share, ahead of check_bn: the conv's form, the coarse plane, R = 1
int check_dwbn(const char* fn, int N, int H, int W, int k, int stride, const float* a, int Hc, int Wc)
{
    if (k != 3 && k != 5) return fail(RCX_ERR_UNSUPPORTED, "%s: kernel size %d (3 or 5)", fn, k);
    if (stride != 1 && stride != 2) return fail(RCX_ERR_UNSUPPORTED, "%s: stride %d (1 or 2)", fn, stride);
    if (a && stride != 1) return fail(RCX_ERR_UNSUPPORTED, "%s: the up-add form (a given) is stride 1 only", fn);
    if (a && (Hc <= 0 || Wc <= 0)) return fail(RCX_ERR_BAD_ARG, "%s: non-positive coarse extent Hc=%d Wc=%d", fn, Hc, Wc);
    if (a && ((long long)Hc >= (1ll << 31) / Wc || (long long)N * Hc * Wc >= (1ll << 31)))
        return fail(RCX_ERR_UNSUPPORTED, "%s: N=%d Hc=%d Wc=%d: 2^31 or more coarse pixels", fn, N, Hc, Wc);
    if (N > 0 && H > 0 && W > 0 && (long long)N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1) == 1)
        return fail(RCX_ERR_BAD_ARG, "%s: batch statistics need more than one value per channel (N=%d H=%d W=%d stride %d)", fn, N, H, W, stride);
    return 0;
}
}  // namespace

int rcx_dwconv_bn_train_fwd(const void* x, const float* a, int Hc, int Wc, const float* w, const float* b, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, void* y, float* u, float* save_mean, float* save_invstd, void* workspace,
                            size_t workspace_bytes, int N, int H, int W, int C, int k, int stride, float momentum, float eps, int dtype, void* stream)
{
    const char* fn = "rcx_dwconv_bn_train_fwd";
    if (!x || !w || !gamma || !beta || !y || !u || !save_mean || !save_invstd) return fail(RCX_ERR_BAD_ARG, "%s: null pointer", fn);
    if (!running_mean != !running_var) return fail(RCX_ERR_BAD_ARG, "%s: running_mean and running_var come together or not at all", fn);
    if (int rc = check_dwbn(fn, N, H, W, k, stride, a, Hc, Wc)) return rc;
    const size_t es = dtype == RCX_DTYPE_F32 ? 4 : 2, cb = (size_t)C * 4, xb = (size_t)N * H * W * C * es;
    const size_t R = (size_t)N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1), ab = a ? (size_t)N * Hc * Wc * cb : 0;
    if (int rc = check_bn(fn, N, H, W, C, dtype, {x, y}, {a, w, b, gamma, beta, running_mean, running_var, u, save_mean, save_invstd, workspace},
                          {{x, xb}, {a, ab}, {w, (size_t)k * k * cb}, {b, cb}, {gamma, cb}, {beta, cb}},
                          {{y, R * C * es}, {u, R * cb}, {running_mean, cb}, {running_var, cb}, {save_mean, cb}, {save_invstd, cb}, {workspace, workspace_bytes}}))
        return rc;
    const size_t need = rcx::dwconv_bn_train_workspace_bytes(N, H, W, C, k, stride, dtype);
    if (!workspace || workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "%s: workspace too small: need %zu bytes, got %zu", fn, need, workspace ? workspace_bytes : (size_t)0);
    hipError_t e = rcx::dwconv_bn_train_fwd(x, a, Hc, Wc, w, b, gamma, beta, running_mean, running_var, y, u, save_mean, save_invstd, workspace, N, H, W, C, k, stride,
                                            momentum, eps, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, fn);
}

int rcx_dwconv_bn_train_bwd(const void* x, const float* a, int Hc, int Wc, const float* u, const void* g, const float* w, const float* gamma, const float* mean,
                            const float* invstd, void* gx, float* ga, float* gw, float* gb, float* ggamma, float* gbeta, void* workspace, size_t workspace_bytes,
                            int N, int H, int W, int C, int k, int stride, int dtype, void* stream)
{
    const char* fn = "rcx_dwconv_bn_train_bwd";
    if (!x || !u || !g || !w || !gamma || !mean || !invstd) return fail(RCX_ERR_BAD_ARG, "%s: null pointer", fn);
    if (!gx && !ga && !gw && !gb && !ggamma && !gbeta) return fail(RCX_ERR_BAD_ARG, "%s: null pointer for every output (gx, ga, gw, gb, ggamma, gbeta)", fn);
    if (ga && !a) return fail(RCX_ERR_BAD_ARG, "%s: ga without a (the plain form has no coarse plane)", fn);
    if (int rc = check_dwbn(fn, N, H, W, k, stride, a, Hc, Wc)) return rc;
    const size_t es = dtype == RCX_DTYPE_F32 ? 4 : 2, cb = (size_t)C * 4, xb = (size_t)N * H * W * C * es;
    const size_t R = (size_t)N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1), ab = a ? (size_t)N * Hc * Wc * cb : 0;
    if (int rc = check_bn(fn, N, H, W, C, dtype, {x, g, gx}, {a, u, w, gamma, mean, invstd, ga, gw, gb, ggamma, gbeta, workspace},
                          {{x, xb}, {a, ab}, {u, R * cb}, {g, R * C * es}, {w, (size_t)k * k * cb}, {gamma, cb}, {mean, cb}, {invstd, cb}},
                          {{gx, xb}, {ga, ab}, {gw, (size_t)k * k * cb}, {gb, cb}, {ggamma, cb}, {gbeta, cb}, {workspace, workspace_bytes}}))
        return rc;
    const size_t need = rcx::dwconv_bn_train_workspace_bytes(N, H, W, C, k, stride, dtype);
    if (!workspace || workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "%s: workspace too small: need %zu bytes, got %zu", fn, need, workspace ? workspace_bytes : (size_t)0);
    hipError_t e = rcx::dwconv_bn_train_bwd(x, a, Hc, Wc, u, g, w, gamma, mean, invstd, gx, ga, gw, gb, ggamma, gbeta, workspace, N, H, W, C, k, stride, dtype,
                                            (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, fn);
}

// A channel mixer's BatchNorm of a training step with its epilogue (rcx_bnact.hip): the exact GELU behind it, or the residual add with the DropPath scale.
// What it takes is what the BatchNorm kernels take: fewer than 2^31 elements.
int rcx_bn_act_supported(int N, int H, int W, int C, int dtype, int rdtype, int epilogue)
{
    return rcx::bn_act_applicable(N, H, W, C, dtype, rdtype, epilogue) ? 1 : 0;
}

size_t rcx_bn_act_workspace_bytes(int N, int H, int W, int C, int dtype, int rdtype, int epilogue)
{
    if (!rcx::bn_act_applicable(N, H, W, C, dtype, rdtype, epilogue)) return 0;
    return rcx::bn_act_workspace_bytes(N * H * W, C, dtype);
}

namespace {
// the checks the two entries share, ahead of check_bn: the epilogue, the residual's dtype, R = 1
int check_bn_act(const char* fn, int N, int H, int W, int epilogue, int dtype, int rdtype)
{
    if (epilogue != RCX_BN_EPI_GELU && epilogue != RCX_BN_EPI_ADD) return fail(RCX_ERR_BAD_ARG, "%s: unknown epilogue %d", fn, epilogue);
    if (!known_dtype(rdtype)) return fail(RCX_ERR_BAD_ARG, "%s: unknown dtype %d of the residual", fn, rdtype);
    if (known_dtype(dtype) && rdtype != dtype && !(epilogue == RCX_BN_EPI_ADD && rdtype == RCX_DTYPE_F32))
        return fail(RCX_ERR_UNSUPPORTED, "%s: rdtype %d with dtype %d (the residual is of u's type, or float32 with the ADD epilogue)", fn, rdtype, dtype);
    if (N > 0 && H > 0 && W > 0 && (long long)N * H * W == 1)
        return fail(RCX_ERR_BAD_ARG, "%s: batch statistics need more than one value per channel (N=%d H=%d W=%d)", fn, N, H, W);
    return 0;
}
}  // namespace

int rcx_bn_act_train_fwd(const void* u, const void* r, const float* scale, void* out, const float* weight, const float* bias, float* running_mean,
                         float* running_var, float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes, int N, int H, int W, int C,
                         float momentum, float eps, int epilogue, int dtype, int rdtype, void* stream)
{
    const char* fn = "rcx_bn_act_train_fwd";
    const bool add = epilogue == RCX_BN_EPI_ADD;
    if (!add) { r = nullptr; scale = nullptr; }                                    // used by ADD only
    if (!u || !out || !weight || !bias || !save_mean || !save_invstd || (add && !r)) return fail(RCX_ERR_BAD_ARG, "%s: null pointer", fn);
    if (!running_mean != !running_var) return fail(RCX_ERR_BAD_ARG, "%s: running_mean and running_var come together or not at all", fn);
    if (int rc = check_bn_act(fn, N, H, W, epilogue, dtype, rdtype)) return rc;
    const bool res32 = rdtype != dtype;
    const size_t es = dtype == RCX_DTYPE_F32 ? 4 : 2, rs = rdtype == RCX_DTYPE_F32 ? 4 : 2, ne = (size_t)N * H * W * C, cb = (size_t)C * 4;
    if (int rc = check_bn(fn, N, H, W, C, dtype, {u, res32 ? nullptr : r, res32 ? nullptr : out},
                          {res32 ? r : nullptr, res32 ? out : nullptr, scale, weight, bias, running_mean, running_var, save_mean, save_invstd, workspace},
                          {{u, ne * es}, {r, ne * rs}, {scale, (size_t)N * 4}, {weight, cb}, {bias, cb}},
                          {{out, ne * rs}, {running_mean, cb}, {running_var, cb}, {save_mean, cb}, {save_invstd, cb}, {workspace, workspace_bytes}}))
        return rc;
    const size_t need = rcx::bn_act_workspace_bytes(N * H * W, C, dtype);
    if (!workspace || workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "%s: workspace too small: need %zu bytes, got %zu", fn, need, workspace ? workspace_bytes : (size_t)0);
    hipError_t e = rcx::bn_act_train_fwd(u, r, scale, out, weight, bias, running_mean, running_var, save_mean, save_invstd, workspace, N * H * W, C, H * W, momentum,
                                         eps, epilogue, dtype, rdtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, fn);
}

int rcx_bn_act_train_bwd(const void* u, const void* g, const float* scale, const float* weight, const float* bias, const float* mean, const float* invstd,
                         void* gu, float* gweight, float* gbias, void* workspace, size_t workspace_bytes, int N, int H, int W, int C, int epilogue, int dtype,
                         int rdtype, void* stream)
{
    const char* fn = "rcx_bn_act_train_bwd";
    const bool add = epilogue == RCX_BN_EPI_ADD;
    if (add) bias = nullptr;                                                       // the GELU's backward forms y again; ADD's does not
    else scale = nullptr;
    if (!u || !g || !weight || !mean || !invstd || (!add && !bias)) return fail(RCX_ERR_BAD_ARG, "%s: null pointer", fn);
    if (!gu && !gweight && !gbias) return fail(RCX_ERR_BAD_ARG, "%s: null pointer for every output (gu, gweight and gbias)", fn);
    if (!gweight != !gbias) return fail(RCX_ERR_BAD_ARG, "%s: gweight and gbias come together or not at all", fn);
    if (int rc = check_bn_act(fn, N, H, W, epilogue, dtype, rdtype)) return rc;
    const bool res32 = rdtype != dtype;
    const size_t es = dtype == RCX_DTYPE_F32 ? 4 : 2, rs = rdtype == RCX_DTYPE_F32 ? 4 : 2, ne = (size_t)N * H * W * C, cb = (size_t)C * 4;
    if (int rc = check_bn(fn, N, H, W, C, dtype, {u, res32 ? nullptr : g, gu}, {res32 ? g : nullptr, scale, weight, bias, mean, invstd, gweight, gbias, workspace},
                          {{u, ne * es}, {g, ne * rs}, {scale, (size_t)N * 4}, {weight, cb}, {bias, cb}, {mean, cb}, {invstd, cb}},
                          {{gu, ne * es}, {gweight, cb}, {gbias, cb}, {workspace, workspace_bytes}}))
        return rc;
    const size_t need = rcx::bn_act_workspace_bytes(N * H * W, C, dtype);
    if (!workspace || workspace_bytes < need) return fail(RCX_ERR_WORKSPACE, "%s: workspace too small: need %zu bytes, got %zu", fn, need, workspace ? workspace_bytes : (size_t)0);
    hipError_t e = rcx::bn_act_train_bwd(u, g, scale, weight, bias, mean, invstd, gu, gweight, gbias, workspace, N * H * W, C, H * W, epilogue, dtype, rdtype,
                                         (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, fn);
}

}  // extern "C"

namespace {

bool ranges_overlap(const void* a, size_t ab, const void* b, size_t bb)
{
    const size_t a0 = (size_t)a, b0 = (size_t)b;
    return a && b && a0 < b0 + bb && b0 < a0 + ab;
}

// the checks rcx_pool_head_fwd and rcx_global_pool_fwd share (w NULL and K = 1 for the pool alone): 0, or the refusal
int check_head(const char* fn, const void* x, const void* w, const float* bias, const void* y, int N, int H, int W, int C, int K, int xdtype, int wdtype)
{
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0) return fail(RCX_ERR_BAD_ARG, "%s: non-positive extent N=%d H=%d W=%d C=%d K=%d", fn, N, H, W, C, K);
    if (!known_dtype(xdtype) || !known_dtype(wdtype)) return fail(RCX_ERR_BAD_ARG, "%s: unknown dtype %d / %d", fn, xdtype, wdtype);
    const size_t es = xdtype == RCX_DTYPE_F32 ? 4 : 2, ws = wdtype == RCX_DTYPE_F32 ? 4 : 2;
    if ((size_t)x % 16 || (size_t)w % 16 || (size_t)y % es || (size_t)bias % 4)
        return fail(RCX_ERR_BAD_ARG, "%s: x and the weight must be aligned to 16 bytes, y to one element (%zu bytes), bias to 4", fn, es);
    const unsigned long long lim = 1ull << 31, xe = (unsigned long long)N * H * W * C, we = (unsigned long long)K * C, ye = (unsigned long long)N * (w ? K : C);
    if ((unsigned long long)H * W >= lim || xe >= lim || we >= lim || ye >= lim)
        return fail(RCX_ERR_BAD_ARG, "%s: 2^31 or more elements (x %llu, the weight %llu, y %llu)", fn, xe, we, ye);
    if (ranges_overlap(y, ye * es, x, xe * es) || ranges_overlap(y, ye * es, w, we * ws) || ranges_overlap(y, ye * es, bias, (size_t)K * 4))
        return fail(RCX_ERR_BAD_ARG, "%s: y must overlap neither x nor the weight nor the bias", fn);
    return 0;
}

}  // namespace

extern "C" {

int rcx_pool_head_supported(int N, int H, int W, int C, int K, int xdtype, int wdtype)
{
    return rcx::pool_head_applicable(N, H, W, C, K, xdtype, wdtype) ? 1 : 0;
}

int rcx_pool_head_fwd(const void* x, const void* wpack, const float* bias, void* y, int N, int H, int W, int C, int K, int xdtype, int wdtype, void* stream)
{
    const char* fn = "rcx_pool_head_fwd";
    if (!x || !wpack || !y) return fail(RCX_ERR_BAD_ARG, "%s: null pointer", fn);
    if (int rc = check_head(fn, x, wpack, bias, y, N, H, W, C, K, xdtype, wdtype)) return rc;
    if (!rcx::pool_head_applicable(N, H, W, C, K, xdtype, wdtype))
        return fail(RCX_ERR_UNSUPPORTED, "%s: C=%d, xdtype=%d, wdtype=%d: C a multiple of 8 up to 1024, the weight float32 or of x's type", fn, C, xdtype, wdtype);
    hipError_t e = rcx::pool_head_fwd(x, wpack, bias, y, N, H, W, C, K, xdtype, wdtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, fn);
}

int rcx_global_pool_fwd(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream)
{
    const char* fn = "rcx_global_pool_fwd";
    if (!x || !y) return fail(RCX_ERR_BAD_ARG, "%s: null pointer", fn);
    if (int rc = check_head(fn, x, nullptr, nullptr, y, N, H, W, C, 1, dtype, dtype)) return rc;
    if (!rcx::global_pool_applicable(N, H, W, C, dtype)) return fail(RCX_ERR_UNSUPPORTED, "%s: C=%d: C a multiple of 8 up to 1024", fn, C);
    hipError_t e = rcx::global_pool_fwd(x, y, N, H, W, C, dtype, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, fn);
}

}  // extern "C"

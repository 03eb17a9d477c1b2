/*
 * recnext_amd -- C ABI of the MI355X (gfx950) RecConv2d / RecAttn2d token-mixer kernels.
 *
 * The reference (suous/RecNeXt) has no FFI layer: its boundary for this path is the Python class
 *     RecConv2d(in_channels, kernel_size=5, bias=False, level=2, mode='bilinear')   model/recnext.py:9
 *     RecAttn2d(dim, num_heads, kernel_size=5, stage=1, mode="nearest")             model/recattn.py:55
 * whose bodies are chains of ATen calls.  This header is what a binding for that class would
 * call instead (see INTEGRATION.md for the ctypes stub); each entry point cites the reference
 * lines it replaces.
 *
 * Conventions
 *   - Activations: device pointers to NHWC-contiguous memory (the storage of a torch.channels_last
 *     tensor of logical shape N x C x H x W).  dtype: RCX_DTYPE_F32, RCX_DTYPE_BF16 or RCX_DTYPE_F16 (arithmetic is float32 for all three).
 *   - Weights: float32 device memory, *packed* tap-major (k,k,C) by rcx_pack_dw_weight from the
 *     reference's (C,1,k,k) parameter layout; biases float32 (C).  A RecConv2d parameter pack is
 *     (level+2) such blocks back to back: [down, convs[0], ..., convs[level]]  (convs[0] pairs with
 *     the coarsest level, model/recnext.py:32-34).
 *   - The library never allocates, frees, synchronises or retains pointers; all work is enqueued
 *     on the hipStream_t passed as `stream` (NULL = the default stream).  Calls are re-entrant.
 *   - Return value: 0 ok; <0 argument / unsupported-configuration error; >0 a hipError_t.
 *     rcx_last_error() returns a thread-local message for the last non-zero return.
 */
#ifndef RECNEXT_AMD_H
#define RECNEXT_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCX_ABI_VERSION 7

enum { RCX_DTYPE_F32 = 0, RCX_DTYPE_BF16 = 1, RCX_DTYPE_F16 = 2 };   /* F16: the reference's autocast dtype (engine.py:48) */
enum { RCX_MODE_BILINEAR = 0, RCX_MODE_NEAREST = 1 };   /* F.interpolate(mode=...), model/recnext.py:33 */
enum { RCX_MAX_LEVEL = 8 };

enum {
    RCX_ERR_BAD_ARG = -1,       /* null pointer, non-positive extent, even k, level out of range */
    RCX_ERR_UNSUPPORTED = -2,   /* configuration outside what the kernels implement */
    RCX_ERR_WORKSPACE = -3      /* workspace smaller than rcx_recconv2d_fwd_workspace_bytes() */
};

int rcx_abi_version(void);
const char* rcx_last_error(void);
/* The RCX_* environment switches (A/B measurement knobs) are read once, at the first call that consults one; this
 * re-reads them.  For tests and A/B tools that flip a switch inside one process; not to be called while another thread is in the library. */
void rcx_reload_options(void);

/* Start-up self-test of one hardware behaviour the 16-bit load paths rely on and the ISA does not promise: a D16 "hi" load
 * (global_load_short_d16_hi, buffer_load_short_d16_hi, ds_read_u16_d16_hi) ZEROES the other half of its destination register on gfx950, so a
 * bf16 element lands in float32 position with no conversion (rcx_cpt_kernel.h row loads, rcx_cpl14_pieces.h, rcx_lanes.h).  One 64-lane launch:
 * reads the 64 16-bit values at `src`, ORs a failure mask into *flag (caller-zeroed uint32: bit 0 global, 1 buffer, 2 LDS form); asynchronous on
 * `stream` -- the caller reads *flag after synchronising.  The Python binding runs it once per device before its first 16-bit launch and raises
 * if the flag is not 0.  Replaces nothing in the reference. */
int rcx_selftest_d16(const void* src, void* flag, void* stream);

/* Description of the kernel schedule rcx_recconv2d_fwd would use for this problem, e.g. "generic" or
 * "plane(cb=16,band8,nt=512,lds=157760)"; thread-local storage, valid until the next call on this thread. */
const char* rcx_recconv2d_fwd_plan(int N, int C, int H, int W, int level, int k, int mode, int dtype);

/* Repack one depthwise weight (C,1,k,k) [dtype f32|bf16|f16] -> float32 (k,k,C).
 * Replaces nothing in the reference (layout plumbing for nn.Conv2d(groups=C).weight, model/recnext.py:21-22). */
int rcx_pack_dw_weight(const void* w_ckk, float* dst_kkc, int C, int k, int dtype, void* stream);
/* All parameters of one RecConv2d block in one launch: w[j] (C,1,k,k) and b[j] (C) [dtype f32|bf16|f16], j = 0 .. count-1 in pack
 * order [down, convs[0], ..., convs[level]] (HOST arrays of DEVICE pointers; b may be NULL, b[j] may be NULL) -> wpack (count,k,k,C),
 * wpack_flipped (the same with every k x k rotated by 180 degrees: the taps rcx_recconv2d_bwd wants; may be NULL) and bpack (count,C)
 * (may be NULL), all float32.  A training step repacks after every optimizer step (engine.py:38-71): this replaces 2*(level+2)
 * rcx_pack_dw_weight / rcx_pack_bias launches and the flip. */
int rcx_pack_recconv_params(const void* const* w, const void* const* b, float* wpack, float* wpack_flipped, float* bpack,
                            int count, int C, int k, int dtype, void* stream);
/* The inverse layout change for the gradients: gwpack (count,k,k,C) float32 -> gw[j] (C,1,k,k) float32 contiguous, one launch. */
int rcx_unpack_recconv_grads(const float* gwpack, void* const* gw, int count, int C, int k, void* stream);
/* Convert one bias vector (C) [dtype f32|bf16|f16] -> float32 (C). */
int rcx_pack_bias(const void* b, float* dst, int C, int dtype, void* stream);

/* Scratch bytes rcx_recconv2d_fwd needs for this problem (may be 0). */
size_t rcx_recconv2d_fwd_workspace_bytes(int N, int C, int H, int W, int level, int k, int dtype);

/*
 * RecConv2d.forward -- model/recnext.py:24-34 (down ladder :27-29, up recursion :31-33, final conv :34).
 *   x, y    : N x H x W x C activations of `dtype` (y may not alias x)
 *   wpack   : (level+2, k, k, C) float32, [down, convs[0..level]]
 *   bpack   : (level+2, C) float32 or NULL (bias=False)
 *   level>=0, k odd, mode RCX_MODE_*.
 */
int rcx_recconv2d_fwd(const void* x, void* y, const float* wpack, const float* bpack,
                      void* workspace, size_t workspace_bytes,
                      int N, int C, int H, int W, int level, int k, int mode, int dtype, void* stream);

/*
 * Measurement hook (nothing in the reference; bench.py's roofline object): the next rcx_recconv2d_fwd of this thread that runs as ONE fused kernel
 * (plan "cpt(...)" or "cpl(...)": the 56x56 / 28x28 / 14x14 / 7x7 blocks) has the two HIP events recorded by the command processor at the kernel's
 * start and end (hipExtLaunchKernelGGL) -- its duration as rocprofv3 sees it, without the dispatch gaps an event pair recorded around the call
 * brackets, and without delaying the next kernel.  Either may be NULL.  Cleared when that call returns, consumed or not
 * (rcx_launch_events_pending() == 1 after arming, 0 once consumed or cleared).
 */
int rcx_time_next_launch(void* start_event, void* stop_event);
int rcx_launch_events_pending(void);

/*
 * Training (engine.py:48-64): a forward that keeps the fp32 pyramid F_1..F_L, C_1..C_L in `saved`, and the backward pass.
 *   rcx_recconv2d_fwd_train   same contract as rcx_recconv2d_fwd (the blocks of RecNeXt at 224x224 run their inference launch, which then also
 *                             writes the pyramid; other shapes the per-level schedule); `saved` must hold
 *                             rcx_recconv2d_train_saved_bytes() and stay untouched until rcx_recconv2d_bwd has run.
 *   rcx_recconv2d_bwd         gy: N x H x W x C of `gy_dtype` (dL/dy): float32 always works; the block's own 16-bit `dtype` -- dL/dy exactly as
 *                             autograd hands it over under autocast, no float32 copy -- where rcx_recconv2d_bwd_gy_dtype() returns it (the
 *                             tiled 56x56 / level 4 and 28x28 / level 3 backward);  gx: N x H x W x C of `dtype` (dL/dx);
 *                             wpack_flipped: wpack with every k x k tap block rotated by 180 degrees (transpose convs);
 *                             gwpack: (level+2, k, k, C) float32 = dL/d[down, convs[0..level]] in the packed layout, the
 *                             shared down weight accumulated over all levels (model/recnext.py:21,28);
 *                             gbpack: (level+2, C) float32 or NULL.
 *                             gw_out / gb_out (HOST arrays of level+2 DEVICE pointers, or NULL): if gw_out is given the gradients leave in the
 *                             PARAMETERS' own layout and type instead -- gw_out[i] (C,1,k,k) contiguous, gb_out[i] (C) (gb_out may be NULL when
 *                             the block has no bias), elements of `grad_dtype` -- written by the final reduction itself (no unpack launch, no
 *                             dtype copy); gwpack / gbpack are then not written and may be NULL.
 *                             Needs C % 4 == 0.  Deterministic (no atomics).
 *   rcx_recconv2d_bwd_gy_dtype  the element type rcx_recconv2d_bwd wants gy in for this problem: `dtype` where a 16-bit gy is read as it is,
 *                             else RCX_DTYPE_F32.
 *   rcx_recconv2d_bwd_plan    the schedule rcx_recconv2d_bwd would use for this problem (same arguments as rcx_recconv2d_bwd_gy_dtype):
 *                             "one(k_recconv_bwd_cpl7)", "one(k_recconv_bwd_cpl14)" / "one(k_recconv_bwd_cpl14,split)" (two waves per plane),
 *                             "tiled(levels=2)+one(...)" / "tiled(levels=1)+one(...)" (the tiled fine levels, then the 14x14 block), "steps+one(...)"
 *                             (one launch per ladder step down to a 14x14 tail), "steps", "generic" (RCX_FORCE_GENERIC=1) or "invalid";
 *                             thread-local storage, valid until the next call on this thread.
 */
size_t rcx_recconv2d_train_saved_bytes(int N, int C, int H, int W, int level, int k);
size_t rcx_recconv2d_bwd_workspace_bytes(int N, int C, int H, int W, int level, int k);
int rcx_recconv2d_fwd_train(const void* x, void* y, const float* wpack, const float* bpack, void* saved, size_t saved_bytes,
                            int N, int C, int H, int W, int level, int k, int mode, int dtype, void* stream);
int rcx_recconv2d_bwd_gy_dtype(int N, int C, int H, int W, int level, int k, int dtype);
const char* rcx_recconv2d_bwd_plan(int N, int C, int H, int W, int level, int k, int dtype);
int rcx_recconv2d_bwd(const void* x, const void* gy, int gy_dtype, const float* wpack, const float* wpack_flipped, const void* saved,
                      void* gx, float* gwpack, float* gbpack, void* const* gw_out, void* const* gb_out, int grad_dtype,
                      void* workspace, size_t workspace_bytes,
                      int N, int C, int H, int W, int level, int k, int mode, int dtype, void* stream);

/*
 * Input-only backward of the RecConv2d block (model/recnext.py:24-34) for a block whose parameters want no gradient (frozen, or folded for
 * inference): gx = dL/dx alone.  The block is linear in x, so gx depends on gy and the taps only -- no x, no saved pyramid (the forward is
 * the inference rcx_recconv2d_fwd), and no weight gradient is formed.
 *   rcx_recconv2d_bwd_input   gy: N x H x W x C of `gy_dtype`: float32 always works; the block's own 16-bit `dtype` (bfloat16 or float16) where
 *                             rcx_recconv2d_bwd_input_gy_dtype() returns it (the one-launch and tiled schedules);  gx: N x H x W x C of `dtype`,
 *                             must not alias gy;  wpack / wpack_flipped as for rcx_recconv2d_bwd (bpack plays no part: the gradient of a bias
 *                             term with respect to x is zero, so a folded block's pack works as it is);  workspace:
 *                             rcx_recconv2d_bwd_input_workspace_bytes() bytes (0: may be NULL).  Needs C % 4 == 0.  Deterministic (no atomics).
 *   rcx_recconv2d_bwd_input_workspace_bytes   0 for the 14x14 / level 2 and 7x7 / level 1 blocks; never more than
 *                             rcx_recconv2d_bwd_workspace_bytes() for the same problem.
 *   rcx_recconv2d_bwd_input_gy_dtype  the element type rcx_recconv2d_bwd_input wants gy in: `dtype` where a 16-bit gy is read as it is, else
 *                             RCX_DTYPE_F32.
 *   rcx_recconv2d_bwd_input_plan  the schedule rcx_recconv2d_bwd_input would use: "one(k_recconv_adj_cpl7)", "one(k_recconv_adj_cpl14)" (the whole
 *                             adjoint in one launch, any batch), "tiled(levels=2)+one(k_recconv_adj_cpl14)" / "tiled(levels=1)+one(...)" (the tiled
 *                             fine levels of the 56x56 / 28x28 blocks, then the 14x14 adjoint), "steps+one(...)" (one launch per ladder step down to a
 *                             14x14 tail), "steps", "generic" (RCX_FORCE_GENERIC=1) or "invalid"; thread-local storage, valid until the next call
 *                             on this thread.  RCX_BWD_FUSED=0 pins "steps", as for rcx_recconv2d_bwd.
 */
size_t rcx_recconv2d_bwd_input_workspace_bytes(int N, int C, int H, int W, int level, int k);
int rcx_recconv2d_bwd_input_gy_dtype(int N, int C, int H, int W, int level, int k, int dtype);
const char* rcx_recconv2d_bwd_input_plan(int N, int C, int H, int W, int level, int k, int dtype);
int rcx_recconv2d_bwd_input(const void* gy, int gy_dtype, const float* wpack, const float* wpack_flipped, void* gx,
                            void* workspace, size_t workspace_bytes,
                            int N, int C, int H, int W, int level, int k, int mode, int dtype, void* stream);

/*
 * Depthwise conv, zero padding k/2, stride 1 or 2 -- nn.Conv2d(groups=C) as used at
 * model/recnext.py:21-22 and by RecAttn2d's ConvNorm(dw k5 s2) after BN folding (model/recattn.py:61, :89-111).
 *   x: N x H x W x C (in_dtype);  y: N x Ho x Wo x C (out_dtype), Ho = (H + 2*(k/2) - k)/stride + 1.
 */
int rcx_dwconv2d_fwd(const void* x, void* y, const float* w_kkc, const float* bias,
                     int N, int C, int H, int W, int k, int stride,
                     int in_dtype, int out_dtype, void* stream);

/*
 * Depthwise conv with channel multiplier 2: nn.Conv2d(Cin, 2*Cin, k, stride, padding=k/2, groups=Cin), i.e. output
 * channel o reads input channel o/2 -- Downsample.token_mixer, model/recnext.py:165 / model/recattn.py:178
 * (with the eval-mode BatchNorm that follows it, :166/:170, folded into w/bias by the caller).
 *   x: N x H x W x Cin ; y: N x Ho x Wo x 2*Cin ; w: (k,k,2*Cin) float32 packed ; x and y share `dtype`.
 */
int rcx_dwconv2d_mult2_fwd(const void* x, void* y, const float* w_kkc, const float* bias,
                           int N, int Cin, int H, int W, int k, int stride, int dtype, void* stream);

/*
 * y = dwconv_k(x + resize(coarse -> (H,W), mode)) -- the body of one up-recursion step
 * (model/recnext.py:33-34) and the tail of RecAttn2d.forward (model/recattn.py:67).
 *   x: N x H x W x C (x_dtype); coarse: N x Hc x Wc x C (coarse_dtype) or NULL (then y = dwconv_k(x));
 *   y: N x H x W x C (out_dtype).
 */
/* Which kernel rcx_upadd_dwconv_fwd would run ("upadd_cpt(k_upadd_cpt<mode, pitch>,...)", "upadd_cpl14(...)", "upadd_lanes(...)",
 * "conv5_lanes(...)", "generic"); has_coarse = 0 for the plain conv (coarse == NULL).  Thread-local storage, valid until the next call. */
const char* rcx_upadd_dwconv_fwd_plan(int N, int C, int H, int W, int Hc, int Wc, int k, int mode,
                                      int x_dtype, int coarse_dtype, int out_dtype, int has_coarse);
int rcx_upadd_dwconv_fwd(const void* x, const void* coarse, void* y, const float* w_kkc, const float* bias,
                         int N, int C, int H, int W, int Hc, int Wc, int k, int mode,
                         int x_dtype, int coarse_dtype, int out_dtype, void* stream);

/*
 * Backward of rcx_dwconv2d_fwd (a depthwise ConvNorm.conv of RecAttn2d in a training step, engine.py:48-64): what autograd
 * derives for nn.Conv2d(groups=C, padding=k/2, stride 1|2), model/recattn.py:61,64 and model/recnext.py:21-22.
 *   x: N x H x W x C (x_dtype); gy: N x Ho x Wo x C float32; w_kkc / w_flipped_kkc: (k,k,C) float32 packs, the second with
 *   both tap axes reversed; gx: like x, may be NULL; gw: (k,k,C) float32, gb: (C) float32 or NULL -- both overwritten.
 *   workspace: rcx_dwconv2d_bwd_workspace_bytes(C, k) bytes.  Deterministic.  C must be a multiple of 4.
 */
size_t rcx_dwconv2d_bwd_workspace_bytes(int C, int k);
int rcx_dwconv2d_bwd(const void* x, const float* gy, const float* w_kkc, const float* w_flipped_kkc,
                     void* gx, float* gw, float* gb, void* workspace, size_t workspace_bytes,
                     int N, int C, int H, int W, int k, int stride, int x_dtype, void* stream);

/*
 * Backward of rcx_upadd_dwconv_fwd with a coarse plane: what autograd derives for the last line of RecAttn2d.forward,
 * `conv(x + F.interpolate(a, size=x.shape[2:], mode))` (model/recattn.py:67; also model/recnext.py:33-34), in a training step (engine.py:48-64).
 *   x: N x H x W x C (`dtype`); coarse: N x Hc x Wc x C float32 (the forward's `a`); gy: N x H x W x C of `gy_dtype` -- float32 always works, the
 *   16-bit `dtype` itself where rcx_upadd_dwconv_bwd_gy_dtype() returns it (56x56 / 28x28 planes with an exact 2x coarse plane: the tiled adjoint
 *   kernels of rcx_recconv2d_bwd); w_kkc / w_flipped_kkc as for rcx_dwconv2d_bwd.
 *   gx: like x (= K^T gy) or NULL; gcoarse: N x Hc x Wc x C float32 (= R^T K^T gy) or NULL; gw: (k,k,C) float32 (= <x + R(coarse), gy>), gb: (C) float32
 *   or NULL -- all overwritten.  workspace: rcx_upadd_dwconv_bwd_workspace_bytes() bytes.  Deterministic.  C must be a multiple of 4.
 */
size_t rcx_upadd_dwconv_bwd_workspace_bytes(int N, int C, int H, int W, int Hc, int Wc, int k);
int rcx_upadd_dwconv_bwd_gy_dtype(int N, int C, int H, int W, int Hc, int Wc, int k, int dtype);
int rcx_upadd_dwconv_bwd(const void* x, const float* coarse, const void* gy, int gy_dtype, const float* w_kkc, const float* w_flipped_kkc,
                         void* gx, float* gcoarse, float* gw, float* gb, void* workspace, size_t workspace_bytes,
                         int N, int C, int H, int W, int Hc, int Wc, int k, int mode, int dtype, void* stream);

/*
 * Backward of rcx_dwconv2d_mult2_fwd with stride 2 (Downsample.token_mixer, model/recnext.py:165, in a training step).
 *   x: N x H x W x Cin (dtype); gy: N x Ho x Wo x 2*Cin float32; w_kkc: (k,k,2*Cin) float32; gx: like x or NULL;
 *   gw: (k,k,2*Cin) float32, gb: (2*Cin) float32 or NULL; workspace: rcx_dwconv2d_bwd_workspace_bytes(2*Cin, k) bytes.
 *   k in {3,5,7}, Cin even.  Deterministic.
 */
int rcx_dwconv2d_mult2_bwd(const void* x, const float* gy, const float* w_kkc, void* gx, float* gw, float* gb,
                           void* workspace, size_t workspace_bytes, int N, int Cin, int H, int W, int k, int dtype, void* stream);

/*
 * Linear-attention core of RecAttn2d's coarse level: everything after the grouped 1x1 `qk` conv of
 * LinearAttention1.forward (model/recattn.py:21-28) / LinearAttention2.forward (:44-51; the same function):
 *     q = elu(qpre)+1, k = elu(kpre)+1; out = q^T (k v^T) / (n * (q^T mean_n(k) + 1e-6)) + pe
 *   qpre, kpre: B x n x C pre-activations of the q / k halves of the `qk` conv (BatchNorm folded, bias added);
 *   v: B x n x C, the attention input itself (:22); pe: B x n x C, output of the `pe` depthwise 3x3 ConvNorm (:27);
 *   out: B x n x C.  n = h*w tokens, token-major (= NHWC); head h owns channels [h*C/heads, (h+1)*C/heads).
 *   All five tensors share `dtype`; C/heads at most 64 (at most 32 unless it is a multiple of 4).
 */
int rcx_linear_attention_fwd(const void* qpre, const void* kpre, const void* v, const void* pe, void* out,
                             int B, int n, int C, int heads, int dtype, void* stream);
/*
 * The same with `pe` computed where it is used (round 3): pe = depthwise 3x3 conv (pad 1) of v + bias -- LinearAttention's `pe`
 * ConvNorm (model/recattn.py:14, :27 / :50) with its BatchNorm folded -- from the (3, 3, C) float32 pack of rcx_pack_dw_weight and the
 * (C) bias pack (or NULL); v is the H x W plane in NHWC.  One launch and one tensor less than rcx_dwconv2d_fwd + rcx_linear_attention_fwd.
 * RCX_ERR_UNSUPPORTED unless C/heads is a multiple of 4 (every head of the A-series is 32 wide) and the call runs on the vector-pipe kernel
 * (fewer than 512 tokens for 32-wide heads and 16-bit I/O: on the matrix-core kernel the fused form measured slower and is not offered).
 */
int rcx_linear_attention_pe_fwd(const void* qpre, const void* kpre, const void* v, const float* w_pe_kkc, const float* b_pe, void* out,
                                int B, int H, int W, int C, int heads, int dtype, void* stream);

/*
 * RecAttn2d's whole coarse level on the matrix cores, for 16-bit-activation runs (round 4): the grouped 1x1 `qk` conv (model/recattn.py:13 / :36
 * with its BatchNorm folded, :21 / :44), the activation, k v^T, the normaliser, q kv and + pe (:22-27 / :45-50) -- what rcx_linear_attention_pe_fwd
 * does plus the projection that used to be two library GEMMs; q and k never exist in memory.
 *   d      : B x (H W) x C float32, the output of the stride-2 ConvNorm (:61), NHWC; also v and the input of `pe`;
 *   wqk    : (2C) x (C/2) bf16, rows [0, C) = the q half of the conv's weight, rows [C, 2C) = the k half (BatchNorm folded in float32, then rounded);
 *   bqk    : (2C) float32 biases; w_pe_kkc / b_pe: as rcx_linear_attention_pe_fwd (b_pe may be NULL);  out: B x (H W) x C float32;
 *   workspace: rcx_recattn_qkcore_workspace_bytes(...) bytes (0 bytes / may be NULL when one launch does it).  Every pointer 16-byte aligned.
 * 1, 2, 4, 8 or 16 heads of dimension C / heads = 32, or of 4, 8 .. 28 when heads is even (a head is padded to 32 inside the kernels; memory stays
 * compact: RecNeXt-A0 / A1 / A2's 20 / 24 / 28), or 2, 4 or 8 heads of 36, 40 .. 64 (round 8: RecNeXt-A5's 40; a head is two 32-channel tiles in
 * registers, the LDS images keep the true width C -- where that image does not fit, e.g. 8 heads of 64 on 7 x 7, the plane takes two launches).  Planes of at most 64 tokens whose image fits the CU's LDS: ONE launch, a workgroup
 * per image, a wave per head (16 heads: at most 32 tokens; RecNeXt-A's stages 2 and 3 at 224 x 224).  Other planes: TWO launches (the k^T v partial
 * sums of every image go through the workspace, summed in a fixed order: deterministic), at most 8 heads.  rcx_recattn_qkcore_launches() tells which
 * (0: no kernel for the shape -> the call returns RCX_ERR_UNSUPPORTED).  The products run on the matrix cores with bf16 operands and float32
 * accumulation, everything else is float32: meant for 16-bit activations (results within north_star's 1e-2 of the float32 forward); float32 callers
 * keep rcx_linear_attention_pe_fwd.
 */
int rcx_recattn_qkcore_launches(int B, int H, int W, int C, int heads);
size_t rcx_recattn_qkcore_workspace_bytes(int B, int H, int W, int C, int heads);
int rcx_recattn_qkcore_fwd(const float* d, const void* wqk_bf16, const float* bqk, const float* w_pe_kkc, const float* b_pe, float* out,
                           void* workspace, size_t workspace_bytes, int B, int H, int W, int C, int heads, void* stream);

/*
 * The same preceded by RecAttn2d's stride-2 depthwise 5x5 ConvNorm (model/recattn.py:12 / :61, BatchNorm folded) in the same launch: x -> d stays in
 * LDS, d never exists in memory.  x: B x H x W x C bf16 / f16 NHWC; w_down_kkc (5,5,C) / b_down (C, may be NULL) float32 as rcx_dwconv2d_fwd takes
 * them; the rest as rcx_recattn_qkcore_fwd; out: B x ceil(H/2) x ceil(W/2) x C float32.  Planes 14 x 14 (1 .. 8 heads) and 7 x 7 (1 .. 16 heads) only --
 * RecNeXt-A's stages 2 and 3 at 224 x 224 --, head dimensions as rcx_recattn_qkcore_fwd (36 .. 64: 2, 4 or 8 heads, the coarse plane's image within the
 * LDS); rcx_recattn_down_qkcore_supported() says (1 / 0); else RCX_ERR_UNSUPPORTED.
 */
int rcx_recattn_down_qkcore_supported(int B, int H, int W, int C, int heads, int x_dtype);
int rcx_recattn_down_qkcore_fwd(const void* x, const float* w_down_kkc, const float* b_down, const void* wqk_bf16, const float* bqk,
                                const float* w_pe_kkc, const float* b_pe, float* out, int B, int H, int W, int C, int heads, int x_dtype, void* stream);

/*
 * RecAttn2d.forward whole (model/recattn.py:54-67 in eval mode, BatchNorms folded): y = ConvNorm_k5(x + interpolate(LinearAttention(ConvNorm_k5s2(x)),
 * size = x's, mode = nearest)) in ONE launch -- a workgroup per image, x's plane read twice (the stride-2 conv, the final conv), d and the attention
 * output only ever in LDS.  x, y: B x H x W x C bf16 / f16 NHWC; w_down_kkc / b_down, w_conv_kkc / b_conv: (5,5,C) / (C) float32 packs (biases may be
 * NULL); wqk / bqk / w_pe_kkc / b_pe as rcx_recattn_qkcore_fwd.  Planes 14 x 14 and 7 x 7, 1 .. 8 heads of 32 channels (or 4 .. 28; never above 32:
 * the attention output's image would not fit the LDS beside d's), RCX_MODE_NEAREST;
 * rcx_recattn2d_fwd_supported() says (1 / 0); else RCX_ERR_UNSUPPORTED -- the caller then chains the entry points above and rcx_upadd_dwconv_fwd.
 */
int rcx_recattn2d_fwd_supported(int B, int H, int W, int C, int heads, int mode, int dtype);
int rcx_recattn2d_fwd(const void* x, void* y, const float* w_down_kkc, const float* b_down, const void* wqk_bf16, const float* bqk,
                      const float* w_pe_kkc, const float* b_pe, const float* w_conv_kkc, const float* b_conv,
                      int B, int H, int W, int C, int heads, int mode, int dtype, void* stream);

/*
 * The channel mixer of a MetaNeXtBlock / Downsample with the residual add around it, inference, ONE launch (model/recnext.py:125-132 `mlp`,
 * :157-158 `x + drop_path(channel_mixer(norm(token_mixer(x))))`, :169-171; model/recattn.py:171, :184), both 1x1 ConvNorms BN-folded (:75-97):
 *     y[m][:] = x[m][:] + W2 gelu(W1 z[m][:] + b1) + b2        m = 0 .. M-1 tokens (M = N H W of an NHWC tensor), gelu = the exact (erf) form
 *   z, x, y : M x C bf16 (z = the token mixer's output, x = the block's input; z == x for Downsample); y may alias neither;
 *   wfrag   : rcx_channel_mlp_pack_bytes(C, H) bytes -- W1 (H x C) and W2 (C x H) rounded to bf16 and laid out as the matrix-core fragments the kernel
 *             reads (recnext_amd/ops.py::pack_channel_mlp builds it; layout in recnext_amd/csrc/rcx_mlp.hip); 16-byte aligned;
 *   bias    : 32 (H/32 + ceil(C/32)) floats: b1 (H), then b2 padded with zeros to a multiple of 32.
 * H % 32 == 0 (pad the hidden layer with zero units: gelu(0) = 0 meets zero weights), C % 8 == 0, M C 2 < 2^31, the weights must fit the LDS.
 * rcx_channel_mlp_supported() says whether there is a kernel for (C, H): today C = 40 / 48 with H = 96, 56 / 64 with 128, 80 / 160, 96 / 192, 128 / 256 (weights resident in LDS) and
 * C = 128 / 256, 160 / 320, 192 / 384, 256 / 512, 320 / 640 (weights streamed through LDS; W2 / b2 padded to an even number of 32-row output tiles when C > 128),
 * and C = 512 / 1024, 512 / 768 and 384 / 768, each from a minimum token count M of its own upward (weights straight from global memory; below it the library's GEMMs
 * are faster: ask with the real M);
 * else RCX_ERR_UNSUPPORTED and the caller keeps the GEMM library.  The products run on the matrix cores with bf16 operands (the hidden activations are
 * rounded to bf16 once, after the GELU) and float32 accumulation.
 */
int rcx_channel_mlp_supported(int M, int C, int H, int dtype);
size_t rcx_channel_mlp_pack_bytes(int C, int H);
int rcx_channel_mlp_fwd(const void* z, const void* x, void* y, const void* wfrag, const float* bias, int M, int C, int H, int dtype, void* stream);

/*
 * RecNextStem, inference, ONE launch (model/recnext.py:134-146; both 3x3 stride-2 ConvNorms BN-folded, :75-97; nn.GELU between them):
 *     y = conv3x3_s2_p1(gelu(conv3x3_s2_p1(x) + b1)) + b2
 *   x  : N x H x W x 3 bf16 (NHWC);  y : N x ceil(ceil(H/2)/2) x ceil(ceil(W/2)/2) x CO bf16 (NHWC);
 *   w1frag : 2 ceil(CM/32) KB, the first conv's (CM, 3, 3, 3) weight rounded to bf16 as matrix-core fragments (K = 27 taps padded to 32);  b1 : 32 ceil(CM/32) float32;
 *   w2frag : rcx_stem_pack_bytes(CM, CO) bytes, the second conv's (CO, CM, 3, 3) weight likewise (recnext_amd/ops.py::pack_stem builds all four);
 *   b2 : 32 ceil(CO/32) float32 (zero padded).  All four 16-byte aligned.  CM in {20, 24, 28, 32, 40} (the registered models' embed_dim[0] / 2), CO % 4 == 0, CO <= 96.
 * The 112 x 112 x CM intermediate exists only as 17 x 17 tiles in LDS, rounded to bf16 once (as the library path does).  rcx_stem_supported() says whether the
 * shape has a kernel; else RCX_ERR_UNSUPPORTED and the caller keeps the conv library.
 */
int rcx_stem_supported(int N, int H, int W, int CM, int CO, int dtype);
size_t rcx_stem_pack_bytes(int CM, int CO);
int rcx_stem_fwd(const void* x, void* y, const void* w1frag, const float* b1, const void* w2frag, const float* b2, int N, int H, int W, int CM, int CO, int dtype, void* stream);

/*
 * RecNextStem of the LSNet-style RecNeXt-T / S / B and their share-channel forms, inference (lsnet/model/recattn.py:208-223; three 3x3 stride-2 ConvNorms
 * BN-folded, 3 -> C/4 -> C/2 -> C, nn.GELU after the first two and, where final_act = 1 (depth[0] == 0: T and S), after the third):
 *     y = act3(conv3(gelu(conv2(gelu(conv1(x) + b1)) + b2)) + b3)
 *   x : N x H x W x 3 bf16 (NHWC, 2-byte aligned);  y : N x H3 x W3 x C bf16 (NHWC), the planes ceil(/2) three times;  C = 64 (T) | 128 (S / B).
 *   w1frag, b1, w2frag, b2 : as rcx_stem_fwd's with CM = C/4, CO = C/2;  w3frag : the third conv's (C, C/2, 3, 3) weight as matrix-core fragments in the same
 *   order;  b3 : C float32.  rcx_stem3_pack_bytes(C, conv) = bytes of conv 1 | 2 | 3's fragments (recnext_amd/ops.py::pack_stem3 builds all six).
 *   workspace : rcx_stem3_workspace_bytes(N, H, W, C) bytes, the N x H2 x W2 x C/2 bf16 intermediate -- written once by the first launch (conv1 + GELU + conv2 +
 *   GELU; the N x H1 x W1 x C/4 intermediate exists only as tiles in LDS) and read once by the second (conv3).  y, workspace and the packs 16-byte aligned;
 *   y and the workspace overlap neither x nor each other.
 * Float32 sums in a fixed order, each intermediate rounded to bf16 once (as the library path does); an image's output does not depend on N or on its place in
 * the batch.  rcx_stem3_supported() says whether the shape has a kernel; else RCX_ERR_UNSUPPORTED and the caller keeps the conv library.
 */
int rcx_stem3_supported(int N, int H, int W, int C, int final_act, int dtype);
size_t rcx_stem3_pack_bytes(int C, int conv);
size_t rcx_stem3_workspace_bytes(int N, int H, int W, int C);
int rcx_stem3_fwd(const void* x, void* y, const void* w1frag, const float* b1, const void* w2frag, const float* b2, const void* w3frag, const float* b3,
                  void* workspace, size_t workspace_bytes, int N, int H, int W, int C, int final_act, int dtype, void* stream);

/*
 * The token half of a block of the LSNet-style RecNeXt-T / S / B (lsnet/model/recattn.py:226-251, eval mode, every BatchNorm folded):
 *     r = RepVGGDW(x) = dw3x3(x) + dw1x1(x) + x                (:8-34; ONE biased depthwise 3x3 conv: lk + zero-padded sk + identity at the centre tap)
 *     t = cat(mixer(r[..., :split]), r[..., split:])            (:226-237, PartialChannelOperation; no slice copy, no concatenation)
 * The block then returns r + MLP(t) (:249-251), which the caller evaluates.  x, r, t: B x H x W x C NHWC, one dtype (float32, bf16 or f16); r and t
 * must not alias x or each other.  w_rep / b_rep: the folded RepVGGDW as a (3,3,C) / (C) float32 pack.  Every other pack covers the slice only
 * (`split` channels): w_*_kkc / b_* are (k,k,split) / (split) float32 packs (rcx_pack_dw_weight / rcx_pack_bias); wqT / wkT are the q and k rows of the
 * folded 1x1 `qk` conv, transposed to (inputs, outputs) float32, with float32 biases bq / bk.  All pointers non-NULL; x, r, t and every pack 16-byte
 * aligned; C and split multiples of 4.  float32 arithmetic, each output rounded once at its store, deterministic (fixed-order reductions, no atomics);
 * two launches: the passthrough channels on a wide grid, the slice on one workgroup per image with all of the mixer's intermediates in LDS.
 *
 * rcx_ls_recattn_fwd: mixer = RecAttn2d (:115-127) with one head of `split` channels: d = dw5 stride 2 (w_down), q / k = elu(grouped 1x1 qk(d)) + 1
 * (q from d's channels [0, split/2), k from [split/2, split)), o = q (k^T v) n^-1 / (q . mean(k) + 1e-6) + pe(d) (LinearAttention1 / 2, :37-86,
 * which are the same function), then t_s = conv5(r_s + nearest(o)) (w_conv).  wqT / wkT: (split/2, split).  `heads` must be 1; planes whose image
 * (the fine slice, d, k / q and k^T v in float32) fits the LDS: 28 x 28 at split 32, 14 x 14 at 64, 7 x 7 at 96 and their 256-input counterparts
 * except 32 x 32.
 * rcx_ls_la3_fwd: mixer = LinearAttention3 (:89-112) at full resolution: qk = elu(full 1x1 qk(r_s)) + 1, q = its channels [0, split/2), k = [split/2,
 * split), each split into `heads` heads (the module's own num_heads, i.e. the constructor's / 2), v = r_s split into as many heads of split/heads;
 * o = q (k^T v) n^-1 / (q . mean(k) + 1e-6) + pe(r_s).  wqT / wkT: (split, split/2).  Planes of at most 64 tokens.
 * The *_supported queries say whether a shape has a kernel (1 / 0); else the entries return RCX_ERR_UNSUPPORTED.
 */
int rcx_ls_recattn_supported(int B, int H, int W, int C, int split, int heads, int dtype);
int rcx_ls_recattn_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const float* w_down_kkc, const float* b_down,
                       const float* wqT, const float* bq, const float* wkT, const float* bk, const float* w_pe_kkc, const float* b_pe,
                       const float* w_conv_kkc, const float* b_conv, int B, int H, int W, int C, int split, int heads, int dtype, void* stream);
int rcx_ls_la3_supported(int B, int H, int W, int C, int split, int heads, int dtype);
int rcx_ls_la3_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const float* wqT, const float* bq,
                   const float* wkT, const float* bk, const float* w_pe_kkc, const float* b_pe, int B, int H, int W, int C, int split, int heads,
                   int dtype, void* stream);

/*
 * The same token halves for ANY plane size (H x W >= 1 x 1, odd and non-square included): the image is cut into chunks of attention tokens and any
 * number of workgroups work on it.  Same tensors, packs, argument rules and arithmetic as the two entries above (float32, the same elu(.)+1 and
 * normaliser, r and t rounded once at their stores), plus a caller-provided float32 workspace of rcx_ls_*_tiled_workspace_bytes(...) bytes, 16-byte
 * aligned, aliasing none of x, r, t: it holds the slice channels only (the fine slice in float32, RecAttn2d's half-size d and attention result, and
 * one partial k^T v and sum(k) per image and chunk).  The library allocates nothing.  The partials are summed in chunk order, no atomics; the chunk
 * length (64 tokens for split <= 64, else 32) depends on `split` alone, never on B: a batch and its shards give the same rows bit for bit.
 * rcx_ls_recattn_tiled_fwd replaces lsnet/model/recattn.py:8-15 (RepVGGDW), :37-86 (LinearAttention1 / 2), :115-127 (RecAttn2d) and the slice / cat
 *   of :226-237 in four launches (RepVGGDW on every channel; d, k and the partials; q and the attention on the half-size plane (H+1)/2 x (W+1)/2;
 *   conv5(r_s + nearest(.)) back at H x W).  `heads` must be 1.
 * rcx_ls_la3_tiled_fwd replaces :8-15, :89-112 (LinearAttention3) and :226-237 in three launches (RepVGGDW; k and the partials; q, the attention
 *   and pe).  split a multiple of 2 heads and split / heads a multiple of 4.
 * A short or NULL workspace returns RCX_ERR_WORKSPACE, a shape without a kernel RCX_ERR_UNSUPPORTED (rcx_ls_*_tiled_supported: 1 / 0; the workspace
 * query returns 0 for such a shape).  rcx_ls_recattn_fwd / rcx_ls_la3_fwd and their queries keep their meaning: a caller asks those first.
 */
int rcx_ls_recattn_tiled_supported(int B, int H, int W, int C, int split, int heads, int dtype);
size_t rcx_ls_recattn_tiled_workspace_bytes(int B, int H, int W, int C, int split, int heads, int dtype);
int rcx_ls_recattn_tiled_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const float* w_down_kkc, const float* b_down,
                             const float* wqT, const float* bq, const float* wkT, const float* bk, const float* w_pe_kkc, const float* b_pe,
                             const float* w_conv_kkc, const float* b_conv, void* workspace, size_t workspace_bytes, int B, int H, int W, int C,
                             int split, int heads, int dtype, void* stream);
int rcx_ls_la3_tiled_supported(int B, int H, int W, int C, int split, int heads, int dtype);
size_t rcx_ls_la3_tiled_workspace_bytes(int B, int H, int W, int C, int split, int heads, int dtype);
int rcx_ls_la3_tiled_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const float* wqT, const float* bq,
                         const float* wkT, const float* bk, const float* w_pe_kkc, const float* b_pe, void* workspace, size_t workspace_bytes,
                         int B, int H, int W, int C, int split, int heads, int dtype, void* stream);

/*
 * The token half of a SHARE block of the share-channel RecNeXt-T / S / B (lsnet/model/recattn_share_channel.py): replaces :8-15 (RepVGGDW), :281-283
 * (ShareChannelOperation: x + cat(x1s)) and the token side of :302-304 in one launch (eval mode, BatchNorms folded):
 *     r = dw3x3(x; w_rep, b_rep)                                  the folded RepVGGDW pack of the entries above, the same bits as their r
 *     t[pixel, j*split + c] = r[pixel, j*split + c] + srcs[j][pixel * src_pixel_stride + c]        c < split, j < n_src
 * x, r, t: B x H x W x C NHWC of `dtype` (float32, bf16 or f16).  srcs: a HOST array of n_src device pointers, read during the call and not kept
 * (the pointers travel to the kernel by value).  Each is the first channel of a B x H x W tensor of `dtype` whose pixels lie src_pixel_stride
 * elements apart: C for the first `split` channels of an earlier block's t (the slice mixer's output x1, :272-276, read in place), `split` for a
 * dense tensor.  Elements [split, stride) of a source pixel are never read.  r and t alias neither x, nor each other, nor a source.  Every pointer
 * non-NULL and aligned to four elements of `dtype` (the packs to 16 bytes).  float32 arithmetic; t is the unrounded r plus the source, so each output
 * is rounded once at its store; no atomics, no workspace, any H x W >= 1 x 1.  Supported (rcx_ls_share_supported: 1 / 0; the entry also wants
 * src_pixel_stride >= split and a multiple of 4): C and split multiples of 4, n_src * split == C, 1 <= n_src <= 8, B*H*W*C < 2^31, a known dtype;
 * else RCX_ERR_UNSUPPORTED.  RCX_ERR_BAD_ARG for a NULL or misaligned pointer, a non-positive extent, an unknown dtype or aliasing outputs.
 */
int rcx_ls_share_supported(int B, int H, int W, int C, int split, int n_src, int dtype);
int rcx_ls_share_fwd(const void* x, void* r, void* t, const float* w_rep, const float* b_rep, const void* const* srcs, int n_src,
                     long long src_pixel_stride, int B, int H, int W, int C, int split, int dtype, void* stream);

/*
 * Downsample.token_mixer of the LSNet-style RecNeXt-T / S / B and of their share-channel variants (lsnet/model/recattn.py:254-263,
 * lsnet/model/recattn_share_channel.py:223-232): the grouped 5x5 stride-2 ConvNorm with groups = gcd(Cin, Cout), eval mode, the BatchNorm folded
 * into the pack, in one launch without a workspace:
 *     y = conv2d(x, w, bias, kernel 5, stride 2, padding 2, groups)        Ho = ceil(H / 2), Wo = ceil(W / 2)
 * x: N x H x W x Cin and y: N x Ho x Wo x Cout, NHWC of `dtype` (float32, bf16 or f16), aligned to one element (wider alignment is used where
 * x has it).  With ci = Cin / groups and co = Cout / groups, wpack is float32 (k, k, ci, Cout):
 *     wpack[((ky*k + kx)*ci + j)*Cout + o] = weight[o][j][ky][kx]
 * bias: float32 (Cout) or NULL.  float32 arithmetic; each output is one thread's fmaf chain over (ky, kx, j) from the bias, rounded once at its
 * store: bitwise repeatable, and the tiling depends on (H, W, Cin, Cout, groups, dtype) alone, so an image's result does not depend on the batch.
 * Supported (rcx_grouped_conv2d_supported: 1 / 0): k = 5, stride = 2, groups >= 1 dividing Cin and Cout, ci and co each 1 .. 4 (the registered
 * models use 1 -> 2, 2 -> 3 and 3 -> 4), any N, H, W >= 1, fewer than 2^31 elements in x and in y; else RCX_ERR_UNSUPPORTED.  RCX_ERR_BAD_ARG
 * for a NULL x / y / wpack, a non-positive extent, an unknown dtype, a misaligned pointer or a y that aliases x or a pack.  Both are decided
 * before any HIP call.
 */
int rcx_grouped_conv2d_supported(int N, int H, int W, int Cin, int Cout, int groups, int k, int stride, int dtype);
int rcx_grouped_conv2d_fwd(const void* x, void* y, const float* wpack, const float* bias, int N, int H, int W, int Cin, int Cout, int groups,
                           int k, int stride, int dtype, void* stream);

/*
 * Backward of rcx_grouped_conv2d_fwd: the gradients engine.py's training step (loss.backward() under autocast) needs through Downsample.token_mixer of
 * the T / S / B families (lsnet/model/recattn.py:254-263, recattn_share_channel.py:223-232), whose BatchNorm stays the caller's operator:
 *     gx[n,iy,ix,g*ci+j] = sum_{ky,kx,u} wpack[((ky*k+kx)*ci+j)*Cout + g*co+u] * gy[n,(iy+2-ky)/2,(ix+2-kx)/2,g*co+u]   (quotients integral, in the plane)
 *     gwpack[((ky*k+kx)*ci+j)*Cout + o] = sum_{n,oy,ox} gy[n,oy,ox,o] * x[n,2*oy+ky-2,2*ox+kx-2,g*ci+j],    gb[o] = sum_{n,oy,ox} gy[n,oy,ox,o]
 * x and gx: N x H x W x Cin, gy: N x Ho x Wo x Cout, NHWC of `dtype`, aligned to one element; gy is read in its own type (no float32 copy).  wpack:
 * the forward's float32 pack; gwpack: float32 in the same (k, k, ci, Cout) layout; gb: float32 (Cout).  gx may be NULL (no input gradient wanted);
 * gwpack and gb may be NULL (frozen weights), gb alone too; not all three.  What is given is overwritten, never accumulated into.  float32
 * arithmetic, no atomics: a gx element is one thread's fmaf chain in the order (ky, kx, u), rounded once at its store, under a tiling that depends on
 * (H, W, Cin, Cout, groups, dtype) alone (an image's gx does not depend on its batch); gwpack / gb are summed in two stages through the workspace,
 * P partials of (25 ci + 1) Cout floats, P a function of the arguments (N among them), so repeat launches are bit-identical.
 * workspace: rcx_grouped_conv2d_bwd_workspace_bytes(...) bytes, aligned to 4, needed when gwpack or gb is given (0 for an unsupported problem).
 * Supported (rcx_grouped_conv2d_bwd_supported: 1 / 0): what rcx_grouped_conv2d_supported takes; else RCX_ERR_UNSUPPORTED.  RCX_ERR_BAD_ARG for a NULL
 * x / gy / wpack, three NULL outputs, a non-positive extent, an unknown dtype, a misaligned pointer, or an output or the workspace aliasing an input or
 * each other; RCX_ERR_WORKSPACE for a workspace smaller than the query.  All decided before any HIP call.
 */
int rcx_grouped_conv2d_bwd_supported(int N, int H, int W, int Cin, int Cout, int groups, int k, int stride, int dtype);
size_t rcx_grouped_conv2d_bwd_workspace_bytes(int N, int H, int W, int Cin, int Cout, int groups, int k, int stride, int dtype);
int rcx_grouped_conv2d_bwd(const void* x, const void* gy, const float* wpack, void* gx, float* gwpack, float* gb, void* workspace, size_t workspace_bytes,
                           int N, int H, int W, int Cin, int Cout, int groups, int k, int stride, int dtype, void* stream);

/*
 * Backward of rcx_linear_attention_fwd(the gradients engine.py:48-64 needs through RecAttn2d, model/recattn.py:16-28 / :39-51):
 *   given gout = dL/dout (B x n x C), writes gq = dL/dqpre, gk = dL/dkpre, gv = dL/dv (all B x n x C, `dtype`); dL/dpe = gout is the
 *   caller's.  float32 arithmetic, deterministic (fixed summation order).  C/heads at most 64.
 */
int rcx_linear_attention_bwd(const void* qpre, const void* kpre, const void* v, const void* gout, void* gq, void* gk, void* gv,
                             int B, int n, int C, int heads, int dtype, void* stream);

/*
 * The linear-attention core with separate q / k and v widths, forward and backward, for the LSNet-style RecNeXt-T / S / B in training:
 * LinearAttention3 (lsnet/model/recattn.py:97-109: q and k take s/2 channels of the full 1x1 `qk`, v is the whole slice) and the 96-channel heads
 * of LinearAttention1 / 2 (:45-56 / :71-82) that rcx_linear_attention_fwd / _bwd do not take.  With Dk = Cqk/heads and Dv = Cv/heads:
 *     q = elu(qpre)+1, k = elu(kpre)+1; out = q^T (k v^T) / (n * (q^T mean_n(k) + 1e-6)) + pe
 *   qpre, kpre: B x n x Cqk pre-activations (BatchNorm applied, bias added), head h owns channels [h*Dk, (h+1)*Dk);
 *   v, pe, out: B x n x Cv, head h owns channels [h*Dv, (h+1)*Dv).  n tokens, token-major (= NHWC).
 * The backward writes gq, gk (B x n x Cqk) and gv (B x n x Cv) from gout = dL/dout (B x n x Cv); dL/dpe = gout is the caller's.
 * Every tensor has `dtype` (float32, bf16 or f16) and is aligned to four elements; out / gq / gk / gv alias no input.  float32 arithmetic, every
 * sum in a fixed order in one thread (bitwise deterministic, no atomics); one workgroup per (image, head), so an image's results do not depend
 * on the batch.  Dk and Dv: multiples of 4 from 4 to 128, any pairing (every pair fits the LDS: at most 115 KiB for the backward at 128 x 128);
 * n >= 1, heads >= 1.  rcx_linear_attention_wide_supported() says whether a shape has a kernel (1 / 0); else the entries return RCX_ERR_UNSUPPORTED
 * (RCX_ERR_BAD_ARG for a null or misaligned pointer, a non-positive extent, an unknown dtype or channels that heads do not divide).
 */
int rcx_linear_attention_wide_supported(int B, int n, int Cqk, int Cv, int heads, int dtype);
int rcx_linear_attention_wide_fwd(const void* qpre, const void* kpre, const void* v, const void* pe, void* out,
                                  int B, int n, int Cqk, int Cv, int heads, int dtype, void* stream);
int rcx_linear_attention_wide_bwd(const void* qpre, const void* kpre, const void* v, const void* gout, void* gq, void* gk, void* gv,
                                  int B, int n, int Cqk, int Cv, int heads, int dtype, void* stream);

/*
 * nn.BatchNorm2d of the training step on a dense NHWC tensor, forward and backward: the `bn` of every ConvNorm (lsnet/model/recattn.py:130-146) as
 * engine.py:38-71 runs it (model.train(), loss.backward() under autocast), and its eval-mode form with gradients flowing, which the detection and
 * segmentation backbones use (frozen statistics).  x, y, gy, gx: N x H x W x C of `dtype` (float32, bf16 or f16), R = N H W rows of C contiguous channels,
 * aligned to one element; weight, bias, every statistic and every parameter gradient: float32 (C), aligned to 4 bytes.  All arithmetic is float32.
 *   rcx_batchnorm_train_fwd   save_mean[c] = mean_r x[r,c], save_invstd[c] = 1 / sqrt(var_r x[r,c] + eps) (biased variance),
 *                             y = (x - save_mean) * save_invstd * weight + bias, rounded once at the store; with running_mean / running_var (both or
 *                             neither; in-out): running = (1 - momentum) * running + momentum * stat, the variance unbiased (R / (R - 1)), as nn.BatchNorm2d.
 *   rcx_batchnorm_frozen_fwd  y = (x - mean) / sqrt(var + eps) * weight + bias from given statistics, one launch; save_invstd (C) or NULL receives
 *                             1 / sqrt(var + eps) as the kernel formed it, for rcx_batchnorm_bwd.
 *   rcx_batchnorm_bwd         with xhat = (x - mean) * invstd from the forward's saved float32 statistics:
 *                               gweight = sum_r gy * xhat, gbias = sum_r gy                                          (both forms)
 *                               gx = weight * invstd * (gy - sum gy / R - xhat * sum(gy * xhat) / R)                   (batch_stats = 1)
 *                               gx = weight * invstd * gy                                                            (batch_stats = 0: frozen statistics)
 *                             gx may be NULL, or the pair (gweight, gbias): not all three, and not one of the pair alone.  With batch_stats = 0 and no
 *                             pair the reduction is not launched and no workspace is needed.  gy is read in x's dtype.  Outputs are overwritten.
 * The sums are never sum x and sum x^2: a thread sums (x - p) and (x - p)^2 against its first element p, threads are combined pairwise (Chan) through LDS
 * in a fixed tree, one partial a workgroup goes to the workspace and the P partials of a channel are combined in index order by a launch of its own.
 * No atomics and no waiting between workgroups.  16-byte accesses are used where C is a multiple of 8 (16-bit) / 4 (float32) and every pointer is
 * aligned to 16 bytes, an element-wide path otherwise (the two need not agree bit for bit); P and the tiling depend on (R, C, dtype) and that choice
 * alone, so repeat launches are bit-identical.
 * workspace: rcx_batchnorm_workspace_bytes(...) bytes (0 for an unsupported problem), aligned to 4, for rcx_batchnorm_train_fwd and for every
 * rcx_batchnorm_bwd that reduces.  rcx_batchnorm_supported: 1 / 0, a rule on (N H W, C, dtype) alone.
 * RCX_ERR_BAD_ARG: a NULL required pointer, one running pointer (or one of gweight / gbias) without the other, a non-positive extent, R = 1 with batch
 * statistics, an unknown dtype, a misaligned pointer, an output or the workspace overlapping an input or each other; RCX_ERR_UNSUPPORTED: 2^31 or more
 * elements; RCX_ERR_WORKSPACE: a workspace smaller than the query.  All decided before any HIP call.
 */
int rcx_batchnorm_supported(int N, int H, int W, int C, int dtype);
size_t rcx_batchnorm_workspace_bytes(int N, int H, int W, int C, int dtype);
int rcx_batchnorm_train_fwd(const void* x, void* y, const float* weight, const float* bias, float* running_mean, float* running_var, float* save_mean,
                            float* save_invstd, void* workspace, size_t workspace_bytes, int N, int H, int W, int C, float momentum, float eps, int dtype,
                            void* stream);
int rcx_batchnorm_frozen_fwd(const void* x, void* y, const float* weight, const float* bias, const float* mean, const float* var, float* save_invstd, float eps,
                             int N, int H, int W, int C, int dtype, void* stream);
int rcx_batchnorm_bwd(const void* x, const void* gy, const float* weight, const float* mean, const float* invstd, void* gx, float* gweight, float* gbias,
                      void* workspace, size_t workspace_bytes, int N, int H, int W, int C, int batch_stats, int dtype, void* stream);

/*
 * RepVGGDW of the training step as one operator, forward and backward (lsnet/model/recattn.py:8-15: r = lk(x) + sk(x) + x, lk a depthwise 3x3 ConvNorm,
 * sk a depthwise 1x1 ConvNorm, both BatchNorms on batch statistics, so nothing can be folded).  x, gx: N x H x W x C of `dtype` (float32, bf16 or f16),
 * R = N H W rows of C contiguous channels, aligned to one element; r and g = dL/dr: the same extents in float32; every parameter, statistic and parameter
 * gradient float32, aligned to 4 bytes: w3, gw3 (C,1,3,3); all others (C).  Zero padding, biased variances, all arithmetic float32.
 *   u  = sum_d w3[d] x(p + d) + b3           ia = 1 / sqrt(var u + eps_a)          ib = 1 / sqrt(w1^2 var x + eps_b)
 *   rcx_repdw_train_fwd  r = gamma_a (u - mean u) ia + beta_a + gamma_b w1 (x - mean x) ib + beta_b + x; saves mean x, var x, mean u, ia; with the four
 *                        running buffers (all or none; in-out), as nn.BatchNorm2d with the unbiased variance:
 *                          lk mean <- (1 - ma) old + ma mean u              lk var <- (1 - ma) old + ma var u R / (R - 1)
 *                          sk mean <- (1 - mb) old + mb (w1 mean x + b1)    sk var <- (1 - mb) old + mb w1^2 var x R / (R - 1)
 *                        Three launches: statistics of x and u in one pass, finalize, apply.
 *   rcx_repdw_train_bwd  from x and the four saved statistics (u is formed again, never stored), uhat = (u - mean u) ia, S0 = sum g, Su = sum g uhat,
 *                        Sx = sum g (x - mean x):
 *                          gbeta_a = gbeta_b = S0, ggamma_a = Su, ggamma_b = w1 ib Sx, gw1 = gamma_b eps_b ib^3 Sx, gb3 = gb1 = 0 (exactly)
 *                          gu = gamma_a ia (g - S0 / R - uhat Su / R),   gw3[d] = sum_p gu(p) x(p + d)
 *                          gx(q) = sum_d w3[d] gu(q - d) + gamma_b w1 ib (g - S0 / R - (x - mean x) w1^2 ib^2 Sx / R) + g
 *                        gx may be NULL, or the eight parameter gradients together: not both, and none of the eight alone.  Four launches (sums,
 *                        finalize, gx with per-workgroup tap partials, their reduction), three without the parameter gradients.  Outputs are overwritten.
 * Statistics are pivoted (n, mean, M2) partials combined pairwise in a fixed tree and then in index order, as rcx_batchnorm_*: never sum x and sum x^2,
 * no atomics, no waiting between workgroups; 16-byte accesses where C is a multiple of 8 (16-bit) / 4 (float32) and every pointer is aligned to 16
 * bytes, an element-wide path otherwise; the tiling depends on (N H W, C, dtype) and that choice alone, so repeat launches are bit-identical.
 * workspace: rcx_repdw_train_workspace_bytes(...) bytes (0 for an unsupported problem), aligned to 4, for both entries.
 * rcx_repdw_train_supported: 1 / 0, a rule on (N H W, C, dtype) alone.
 * RCX_ERR_BAD_ARG: a NULL required pointer, some but not all of the running buffers (or of the parameter gradients), a non-positive extent, R = 1, an
 * unknown dtype, a misaligned pointer, an output or the workspace overlapping an input or each other; RCX_ERR_UNSUPPORTED: 2^31 or more elements;
 * RCX_ERR_WORKSPACE: a workspace smaller than the query.  All decided before any HIP call.
 */
int rcx_repdw_train_supported(int N, int H, int W, int C, int dtype);
size_t rcx_repdw_train_workspace_bytes(int N, int H, int W, int C, int dtype);
int rcx_repdw_train_fwd(const void* x, float* r, const float* w3, const float* b3, const float* gamma_a, const float* beta_a, const float* w1, const float* b1,
                        const float* gamma_b, const float* beta_b, float* lk_running_mean, float* lk_running_var, float* sk_running_mean, float* sk_running_var,
                        float* save_mean_x, float* save_var_x, float* save_mean_u, float* save_invstd_u, void* workspace, size_t workspace_bytes,
                        int N, int H, int W, int C, float momentum_a, float eps_a, float momentum_b, float eps_b, int dtype, void* stream);
int rcx_repdw_train_bwd(const void* x, const float* g, const float* w3, const float* b3, const float* gamma_a, const float* w1, const float* gamma_b,
                        const float* mean_x, const float* var_x, const float* mean_u, const float* invstd_u, void* gx, float* gw3, float* gb3, float* ggamma_a,
                        float* gbeta_a, float* gw1, float* gb1, float* ggamma_b, float* gbeta_b, void* workspace, size_t workspace_bytes,
                        int N, int H, int W, int C, float eps_b, int dtype, void* stream);

/*
 * A depthwise ConvNorm of the training step as one operator, forward and backward: the slice mixers' down[0] (5x5, stride 2), pe (3x3), conv (5x5 on
 * x + resize(a)) and LinearAttention3's pe (lsnet/model/recattn.py:54-67, :89-112), the BatchNorm on batch statistics, so nothing can be folded.
 * x, gx: N x H x W x C of `dtype` (float32, bf16 or f16), aligned to one element; y, g = dL/dy: N x Ho x Wo x C of `dtype`, Ho = (H - 1) / stride + 1,
 * Wo likewise, R = N Ho Wo rows of C contiguous channels; a, ga: N x Hc x Wc x C float32, or NULL (the plain form; Hc, Wc are then ignored); u: R x C
 * float32; w, gw (C,1,k,k) and every other parameter, statistic and parameter gradient (C): float32, aligned to 4 bytes.  k = 3 | 5, zero padding k / 2,
 * stride = 1 | 2 (the up-add form: stride 1 only), all arithmetic float32.
 *   z = x + a(floor(h Hc / H), floor(w Wc / W))   (nearest, the float index arithmetic of rcx_upadd_dwconv_fwd)        u = sum_d w[d] z(p stride + d - k/2) + b
 *   rcx_dwconv_bn_train_fwd  y = gamma (u - mean u) ia + beta, ia = 1 / sqrt(var u + eps) (biased variance), rounded once from float32; writes u, mean u
 *                            and ia; b may be NULL; with running_mean / running_var (both or neither; in-out), as nn.BatchNorm2d with the unbiased
 *                            variance R / (R - 1).  Three launches: conv + statistics in one pass (u is stored), finalize, apply from u.
 *   rcx_dwconv_bn_train_bwd  from x, a, the stored u and the two saved statistics; g is read in y's dtype as it is.  uhat = (u - mean u) ia,
 *                            S0 = sum g, Su = sum g uhat, gu = gamma ia (g - S0 / R - uhat Su / R):
 *                              gbeta = S0, ggamma = Su, gb = 0 (exactly: a bias in front of a BatchNorm on batch statistics has no gradient; written as zeros)
 *                              gw[d] = sum_p gu(p) z(p stride + d - k/2)
 *                              gx(q) = sum_d w[d] gu(p), p stride + d - k/2 = q     (gu from g and u at those p: u is never formed again)
 *                              ga(r) = sum of gx, before its rounding, over the fine pixels whose nearest source is r, in raster order (a gather)
 *                            Every output may be NULL, not all of them; ga needs a.  Launches: sums, finalize; one for gx and ga (skipped when both are
 *                            NULL); two for gw (per-workgroup tap partials, their reduction; skipped when gw is NULL).  Outputs are overwritten.
 * Statistics are pivoted (n, mean, M2) partials combined pairwise in a fixed tree and then in index order, as rcx_batchnorm_*: never sum u and sum u^2,
 * no atomics, no waiting between workgroups; 16-byte accesses where C is a multiple of 8 (16-bit) / 4 (float32) and every pointer is aligned to 16
 * bytes, an element-wide path otherwise; the tiling depends on (rows, C, dtype) and that choice alone, so repeat launches are bit-identical, and an
 * image's u, y and gx do not depend on the other images but through the statistics.
 * workspace: rcx_dwconv_bn_train_workspace_bytes(...) bytes (0 for an unsupported problem), aligned to 4, for both entries.
 * rcx_dwconv_bn_train_supported: 1 / 0, a rule on (N, H, W, C, k, stride, has_coarse, dtype) alone.
 * RCX_ERR_BAD_ARG: a NULL required pointer, one running pointer without the other, every output NULL, ga without a, a non-positive extent, R = 1, an
 * unknown dtype, a misaligned pointer, an output or the workspace overlapping an input or each other; RCX_ERR_UNSUPPORTED: k not 3 or 5, stride not 1 or
 * 2, the up-add form with stride 2, 2^31 or more elements; RCX_ERR_WORKSPACE: a workspace smaller than the query.  All decided before any HIP call.
 */
int rcx_dwconv_bn_train_supported(int N, int H, int W, int C, int k, int stride, int has_coarse, int dtype);
size_t rcx_dwconv_bn_train_workspace_bytes(int N, int H, int W, int C, int k, int stride, int has_coarse, int dtype);
int rcx_dwconv_bn_train_fwd(const void* x, const float* a, int Hc, int Wc, const float* w, const float* b, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, void* y, float* u, float* save_mean, float* save_invstd, void* workspace,
                            size_t workspace_bytes, int N, int H, int W, int C, int k, int stride, float momentum, float eps, int dtype, void* stream);
int rcx_dwconv_bn_train_bwd(const void* x, const float* a, int Hc, int Wc, const float* u, const void* g, const float* w, const float* gamma, const float* mean,
                            const float* invstd, void* gx, float* ga, float* gw, float* gb, float* ggamma, float* gbeta, void* workspace, size_t workspace_bytes,
                            int N, int H, int W, int C, int k, int stride, int dtype, void* stream);

/*
 * The two BatchNorms of a channel mixer in the training step, each with what follows it as its epilogue: lsnet/model/recattn.py:199-205 (mlp:
 * ConvNorm, GELU, ConvNorm), :240-251 and :254-263 (x + drop_path(channel_mixer(.))), :208-223 (the stem's ConvNorm -> GELU pairs), and
 * model/recnext.py:125-131, :134-146, :149-158, :161-171 for the M / A families, as engine.py:38-71 runs them.  u, gu: N x H x W x C of `dtype` (float32,
 * bf16 or f16), R = N H W rows of C contiguous channels, aligned to one element; weight, bias, every statistic and parameter gradient float32 (C),
 * aligned to 4 bytes; all arithmetic float32; y = (u - save_mean) * save_invstd * weight + bias is never stored.
 *   epilogue = RCX_BN_EPI_GELU   out = z = y Phi(y), Phi(y) = (1 + erf(y / sqrt 2)) / 2, the exact GELU on a float32 erf good to a few ulps (not the
 *                                fit of rcx_channel_mlp_fwd); out and g = dL/dz of `dtype`; rdtype = dtype; r and scale are ignored.
 *   epilogue = RCX_BN_EPI_ADD    out = r + scale[n] * y: the residual add behind the mixer with the DropPath mask; scale float32 (N) or NULL (= 1);
 *                                r, out and g = dL/dout of `rdtype` = dtype or float32 (an autocast step's float32 residual); r may not overlap out.
 *   rcx_bn_act_train_fwd   the statistics exactly as rcx_batchnorm_train_fwd forms and saves them (the same two launches; running_mean / running_var
 *                          both or neither, in-out), then one apply launch; out is rounded once, at its store.
 *   rcx_bn_act_train_bwd   d = g * (Phi(y) + y phi(y)), y formed again from u and the saved statistics (GELU; bias is read), or d = scale[n] * g (ADD;
 *                          bias is ignored; dL/dr is g itself and has no kernel); with xhat = (u - mean) * invstd:
 *                            gweight = sum_r d * xhat, gbias = sum_r d, gu = weight * invstd * (d - sum d / R - xhat * sum(d * xhat) / R)
 *                          gu may be NULL, or the pair (gweight, gbias): not all three, and not one of the pair alone.  Three launches (sums of d,
 *                          finalize, gu), two without gu; d is formed twice and never stored.  Outputs are overwritten.
 * The reductions, both access paths (16 bytes where C is a multiple of 8 (16-bit) / 4 (float32) and every pointer read that wide is aligned to 16
 * bytes, element-wide otherwise), the tiling and the workspace are rcx_batchnorm_*'s: no atomics, no waiting between workgroups, repeat launches
 * bit-identical.  workspace: rcx_bn_act_workspace_bytes(...) bytes (0 for an unsupported problem), aligned to 4, for both entries.
 * rcx_bn_act_supported: 1 / 0, a rule on (N H W, C, dtype, rdtype, epilogue) alone.
 * RCX_ERR_BAD_ARG: a NULL required pointer (r with ADD, bias with the GELU's backward), one running pointer (or one of gweight / gbias) without the
 * other, every output NULL, an unknown epilogue or dtype, a non-positive extent, R = 1, a misaligned pointer, an output or the workspace overlapping an
 * input or each other; RCX_ERR_UNSUPPORTED: rdtype neither dtype nor (ADD) float32, 2^31 or more elements; RCX_ERR_WORKSPACE: a workspace smaller than
 * the query.  All decided before any HIP call.
 */
#define RCX_BN_EPI_GELU 0
#define RCX_BN_EPI_ADD 1
int rcx_bn_act_supported(int N, int H, int W, int C, int dtype, int rdtype, int epilogue);
size_t rcx_bn_act_workspace_bytes(int N, int H, int W, int C, int dtype, int rdtype, int epilogue);
int rcx_bn_act_train_fwd(const void* u, const void* r, const float* scale, void* out, const float* weight, const float* bias, float* running_mean,
                         float* running_var, float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes, int N, int H, int W, int C,
                         float momentum, float eps, int epilogue, int dtype, int rdtype, void* stream);
int rcx_bn_act_train_bwd(const void* u, const void* g, const float* scale, const float* weight, const float* bias, const float* mean, const float* invstd,
                         void* gu, float* gweight, float* gbias, void* workspace, size_t workspace_bytes, int N, int H, int W, int C, int epilogue, int dtype,
                         int rdtype, void* stream);

/*
 * The classifier head behind the last block, global average pool + linear, in one launch without a workspace: model/recnext.py forward_head
 * (x.mean((2, 3)), head_drop, head) with RecNextClassifier (two NormLinear heads averaged; one nn.Linear after fuse()) for the M / A families, and
 * lsnet/model/recattn.py:266-293 (RecNextClassifier) with the forward_head of RecNext (:307-387) for T / S / B and their share-channel variants:
 *     y[n][k] = bias[k] + sum_c w[k][c] * ((1 / (H W)) sum_p x[n][p][c])                n < N, k < K
 * x: N x H x W x C, NHWC of `xdtype` (float32, bf16 or f16), aligned to 16 bytes.  y: N x K of `xdtype`, aligned to one element, rounded once, at its
 * store.  wpack: the K x C weight, row-major as nn.Linear holds it, of `wdtype` = float32 or `xdtype`, aligned to 16 bytes; the kernel widens it
 * exactly.  bias: float32 (K), aligned to 4 bytes, or NULL.  All arithmetic is float32: the pooled sum (8 pixel slices, 4 when C > 512, each a chain
 * in pixel order, added as a fixed tree), the product with the float32 1 / (H W), the dot product (a lane's fmaf chain over its own 8 or 16
 * channels, then a tree over the 64 lanes), the bias.  No 16-bit intermediate, no matrix-core operand, no atomics.  An output is one fixed expression
 * of its image's pixels and its class's row: the same bits at any N, at any position in the batch and on every launch.
 * rcx_global_pool_fwd is the pool alone (num_classes = 0, where the head is nn.Identity): y: N x C of `dtype`, the float32 mean rounded once.
 * Supported (rcx_pool_head_supported: 1 / 0, without a GPU): C a multiple of 8 up to 1024, wdtype float32 or xdtype, any N, H, W, K >= 1 (for
 * rcx_global_pool_fwd the same rule with K = 1); else RCX_ERR_UNSUPPORTED.  RCX_ERR_BAD_ARG for a NULL x / wpack / y, a non-positive extent, an
 * unknown dtype, a misaligned pointer, a y that overlaps x, wpack or bias, or 2^31 or more elements in x, wpack or y.  All decided before any HIP call.
 */
int rcx_pool_head_supported(int N, int H, int W, int C, int K, int xdtype, int wdtype);
int rcx_pool_head_fwd(const void* x, const void* wpack, const float* bias, void* y, int N, int H, int W, int C, int K, int xdtype, int wdtype, void* stream);
int rcx_global_pool_fwd(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RECNEXT_AMD_H */

/*
 * kpx.h -- C ABI of libkpx_hip.so: the MI355X (gfx950) kernels behind the detector_translator
 * per-frame hot path.
 *
 * The reference (YunjiKim/Unsupervised-Keypoint-Learning-...) has no FFI / custom-op boundary: its
 * arithmetic is TensorFlow-1.12 ops called from Python.  Each entry point below therefore names the
 * reference call site(s) (file:line under /root/reference) whose TF op it replaces.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes, no torch / C++ types; every pointer is DEVICE memory owned by the caller
 *     (the library never allocates, frees or keeps global state);
 *   - tensors are float32 NHWC; conv kernels HWIO [kh][kw][Cin][Cout]; "ld*" = pixel stride in floats
 *     (>= channel count) so that producers can write into / consumers read from channel slices of a wider
 *     buffer (this is how tf.concat(axis=-1) is realised without a copy);
 *   - asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return 0 on success, KPX_EINVAL (-1) for a bad argument, or -(hipError_t) if the launch failed;
 *     nothing throws across the ABI; re-entrant, callable from any host thread.  The only process state is a per-device
 *     "large-LDS attribute already set" bit per kernel family (std::atomic, idempotent) and the tuning switches (KPX_* environment
 *     variables), which are parsed ONCE, on first use (csrc/kpx_env.hip; no launch path calls getenv); kpx_reload_env() parses them again.
 */
#ifndef KPX_H
#define KPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KPX_EINVAL (-1)
#define KPX_ABI_VERSION 25

enum { KPX_ACT_NONE = 0, KPX_ACT_RELU = 1, KPX_ACT_LRELU = 2 /* slope 0.01 */, KPX_ACT_TANH = 3 /* forward only */ };

int kpx_abi_version(void);

/* Parse the KPX_* tuning / debugging switches again (they are otherwise read once, on first use).  For harnesses that flip a switch
 * between launches (bench.py: KPX_NO_WINO=1 to time the direct kernel on the roofline layer).  Call it from the launching thread, between
 * launches.  Returns 0.  (No reference counterpart: TF-1.12 reads its TF_* switches the same way, once.) */
int kpx_reload_env(void);

/* `arith` argument of kpx_conv2d_fwd_f32 / _dgrad_f32 / _wgrad_f32: the arithmetic of the layers those entries run on the bf16 matrix
 * pipe (csrc/conv_gemm3.hip: strided / 4x4 / 1x1 layers and their weight gradients).  KPX_ARITH_F32: every fp32 operand is split exactly
 * into three bf16 terms and six partial products are accumulated in fp32 -- fp32-equivalent, the fp32 configuration (the fp32-MFMA
 * kernels the other shapes run on are unaffected by the argument).  KPX_ARITH_BF16: operands truncated to bf16, one product, fp32
 * accumulation -- the bf16 configuration (BASELINE configs[2]).  Per call: two models of different configurations can share a process.
 * No reference counterpart (TF-1.12 computes models/networks/layers.py:6-9 in the graph's one dtype). */
enum { KPX_ARITH_F32 = 0, KPX_ARITH_BF16 = 1 };

/* ---- convolution: replaces tf.pad + tf.layers.conv2d(padding='same') (models/networks/layers.py:6-9)
 *      and tf.nn.conv2d + bias_add + relu (models/networks/vgg.py:51-54).
 *      y[n,oh,ow,:] = act( sum_{r,q,c} x[n, oh*stride + r - pad_t, ow*stride + q - pad_l, c] * w[r,q,c,:] + bias )
 *      pad_t/pad_l are the TOTAL top/left padding (explicit tf.pad + TF's SAME split, decided by the caller);
 *      bottom/right padding is implied by Ho/Wo.  bias may be NULL.  fp32 MFMA implicit GEMM.
 *      `workspace` (optional, may be NULL): split-K scratch for small-M / long-K layers; size from
 *      kpx_conv2d_fwd_workspace_bytes (0 = not needed).  Without it the layer runs unsplit. */
size_t kpx_conv2d_fwd_workspace_bytes(int N, int Ho, int Wo, int Cin, int Cout, int KH, int KW);
int kpx_conv2d_fwd_f32(const float* x, int N, int Hi, int Wi, int Cin, int ldx,
                       const float* w_hwio, int KH, int KW, const float* bias,
                       float* y, int Ho, int Wo, int Cout, int ldy,
                       int stride, int pad_t, int pad_l, int act, int arith,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused Winograd F(2x2,3x3) path of the 3x3 stride-1 SAME convolution with PRE-TRANSFORMED filters (fp32 MFMA; same reference
 *      call sites as kpx_conv2d_fwd_f32 for kernel=3, stride=1).  kpx_conv2d_fwd_f32 / _dgrad_f32 take this path by themselves when a
 *      workspace is given (transforming the filter on every call); a caller that keeps U = G g G^T between calls -- constant filters
 *      (VGG19, vgg.py:57-61), or once per optimiser update for trainable ones -- uses these entry points directly:
 *        kpx_wino_u_bytes: size of U for a [3][3][Cin][Cout] filter (either direction);
 *        kpx_wino_filter_transform_f32: one filter; dgrad != 0 transforms the flipped / transposed filter of the data gradient;
 *        kpx_wino_filter_transform_batch_f32: n filters in ONE launch, `descs` = DEVICE array of KpxWinoDesc;
 *        kpx_conv3x3_wino_f32: out[N,H,W,Nn] = act(conv3x3_same(in[N,H,W,K]) + bias) with U for (K gathered, Nn produced) channels.
 *      Shapes: H, W multiples of 16 (or 8x8 images with N a multiple of 4), see kpx_conv3x3_wino_eligible. */
typedef struct KpxWinoDesc { const float* w; float* u; int cin, cout, dgrad, reserved; } KpxWinoDesc;
size_t kpx_wino_u_bytes(int Cin, int Cout);
int kpx_wino_filter_transform_f32(const float* w_hwio, int Cin, int Cout, int dgrad, float* u, void* stream);
int kpx_wino_filter_transform_batch_f32(const void* descs, int n, void* stream);
int kpx_conv3x3_wino_eligible(int N, int H, int W, int K, int Nn, int ldin, const void* in);
/* Epilogue options of kpx_conv3x3_wino_f32 (all NULL: the plain convolution):
 *   tile_stats alone: the batch-norm statistics of the OUTPUT as well (tf.contrib.layers.batch_norm follows every generator conv,
 *     models/networks/layers.py:13-14): tile_stats[N * (H/16) * (W/16)][2][Nn] = per 16x16-pixel tile and channel, the sum and the sum
 *     of squares of out (fp32, fixed summation order).  kpx_bn_train_fwd_f32 takes them as tile_stats instead of its pass over the
 *     activation.  H, W multiples of 16.
 *   tile_stats + bn_y + bn_beta: data gradient of a 3x3 layer whose INPUT was bn_y = relu(BN(x)): out = dgrad (written as usual) and,
 *     per 16x16-pixel tile and channel, tile_stats[tile][2][Nn] = sum(dz), sum(dz * (bn_y - bn_beta)) with dz = out * [bn_y > 0] -- the
 *     two reductions of that batch norm's backward (bn_y: its output at the same pixels / channels, pixel stride ld_bn_y >= Nn).
 *     kpx_bn_train_bwd_f32 takes them as tile_stats.  No bias, act = KPX_ACT_NONE; H, W multiples of 16.
 * Any other mix returns KPX_EINVAL. */
int kpx_conv3x3_wino_f32(const float* in, int N, int H, int W, int K, int ldin, const float* u, const float* bias,
                         float* out, int Nn, int ldout, int act, float* tile_stats, const float* bn_y, int ld_bn_y,
                         const float* bn_beta, void* stream);
size_t kpx_conv3x3_wino_stats_tiles(int N, int H, int W);

/* ---- bf16 STORAGE (the bf16 configuration proper, BASELINE configs[2] "bf16 storage + fp32 accumulate"): the same layers.conv call sites
 *      (layers.py:4-10; networks/__init__.py:13-24,50-62,80-97; vgg.py:20-40) with bf16 activation tensors in HBM.  `in` is bf16
 *      [N,H,W,K] (pixel stride ldin ELEMENTS, a multiple of 8; 16-byte aligned), `out` bf16 [N,H,W,Nn] (out_f32 = 0; Nn, ldout multiples
 *      of 8) or fp32 (out_f32 = 1; multiples of 4).  Filters stay fp32 masters; kpx_conv3x3_bf16s_prepare_f32 (or the batched form: one
 *      launch per optimiser update over a device table of {const float* w; void* wf; int Cin, Cout, dgrad, NB = 4 * ceil(Nn / 128)}
 *      entries, 32 bytes each) writes the fragment-ordered bf16 copy of one direction (kpx_conv3x3_bf16s_weights_bytes(K, Nn) bytes).
 *      out = mask_gate( act( conv3x3_same(in, wf) + bias ) ): `mask` (optional, bf16 [N,H,W,Nn], pixel stride ldmask) zeroes the output
 *      where mask <= 0 (ReLU backward of the tensor a data gradient belongs to); `stats` (optional) receives per-workgroup channel sums
 *      and sums of squares of the fp32 results before the activation, [kpx_conv3x3_bf16s_stats_tiles(...)][2][Nn] floats, for the batch
 *      norm that follows (layers.py:13-14).  Shapes: W a multiple of 32, or W = 16 / 8 (whole images per tile); K a multiple of 32 or
 *      8 / 16; kpx_conv3x3_bf16s_eligible tells. */
size_t kpx_conv3x3_bf16s_weights_bytes(int K, int Nn);
int kpx_conv3x3_bf16s_eligible(int N, int H, int W, int K, int Nn, int ldin, const void* in);
int kpx_conv3x3_bf16s_stats_tiles(int N, int H, int W, int K, int Nn);
int kpx_conv3x3_bf16s_prepare_f32(const float* w_hwio, int Cin, int Cout, int dgrad, void* wf, void* stream);
int kpx_conv3x3_bf16s_prepare_batch_f32(const void* table, int ndesc, void* stream);
int kpx_conv3x3_bf16s(const void* in, int N, int H, int W, int K, int ldin, const void* wf, const float* bias,
                      void* out, int Nn, int ldout, int out_f32, int act, const void* mask, int ldmask, float* stats, void* stream);
/* Data gradient towards bn_y = relu(batch_norm(.)) (bf16 [N,H,W,Nn]) with that batch norm's backward sums reduced in the epilogue: out = conv3x3(in, wf)
 * gated by bn_y > 0, stats[tile][2][Nn] = sum(dz), sum(dz * (bn_y - beta)) per workgroup -- kpx_bn_train_bwd_bf16 takes them as tile_stats and skips
 * its reduction pass over (dz, x) (the fp32 configuration's kpx_conv3x3_wino43_f32 with tile_stats + bn_y + bn_beta). */
int kpx_conv3x3_bf16s_bnbwd(const void* in, int N, int H, int W, int K, int ldin, const void* wf, void* out, int Nn, int ldout,
                            const void* bn_y, int ld_bn_y, const float* beta, float* stats, void* stream);

/* dx = d(loss)/dx given dy (gradient of the conv output BEFORE activation).  Writes every element of dx.
 * stride <= 2.  `workspace`: optional split-K scratch, see kpx_conv2d_fwd_f32. */
size_t kpx_conv2d_dgrad_workspace_bytes(int N, int Hi, int Wi, int Cin, int Cout, int KH, int KW, int stride);
int kpx_conv2d_dgrad_f32(const float* dy, int N, int Ho, int Wo, int Cout, int lddy,
                         const float* w_hwio, int KH, int KW,
                         float* dx, int Hi, int Wi, int Cin, int lddx,
                         int stride, int pad_t, int pad_l, int arith,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The same data gradient multiplied by the activation backward of the tensor it belongs to: dx = dgrad(dy) * act_in'(y_in), y_in = the
 * ACTIVATED tensor (same shape as dx, pixel stride ld_y_in), act_in = KPX_ACT_RELU / KPX_ACT_LRELU.  This is the chain
 * conv -> leaky_relu -> conv of models/networks/__init__.py:141-151 (img_discr) walked backwards with the leaky-ReLU backward (tf.gradients
 * of tf.nn.leaky_relu) applied in the epilogue of the data gradient ABOVE it instead of a pass of its own (kpx_act_bwd_f32).  Fused on the
 * implicit-GEMM kernels (and their split-K reduce); the specialised kernels take one extra pass over dx (contiguous tensors). */
int kpx_conv2d_dgrad_act_f32(const float* dy, int N, int Ho, int Wo, int Cout, int lddy,
                             const float* w_hwio, int KH, int KW,
                             float* dx, int Hi, int Wi, int Cin, int lddx,
                             int stride, int pad_t, int pad_l, int arith,
                             const float* y_in, int ld_y_in, int act_in,
                             void* workspace, size_t workspace_bytes, void* stream);

/* dw[r,q,c,k] = sum_{n,oh,ow} x[n, oh*s+r-pad_t, ow*s+q-pad_l, c] * dy[n,oh,ow,k].
 * `workspace` holds split-K partial slabs; query its size with kpx_conv2d_wgrad_workspace_bytes, which covers every call of the three
 * weight-gradient entries (this one, kpx_conv2d_wgrad_bf16, kpx_conv_image_wgrad_bf16) for a layer of that shape.  One plan per call chooses
 * the kernel family and the number of slabs; a workspace smaller than that plan needs is refused with KPX_EINVAL before any device call
 * (no other family is tried in its place). */
size_t kpx_conv2d_wgrad_workspace_bytes(int N, int Ho, int Wo, int Cin, int Cout, int KH, int KW);
int kpx_conv2d_wgrad_f32(const float* x, int N, int Hi, int Wi, int Cin, int ldx,
                         const float* dy, int Ho, int Wo, int Cout, int lddy,
                         float* dw_hwio, int KH, int KW, int stride, int pad_t, int pad_l, int arith,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The plan kpx_conv2d_wgrad_f32 makes for the same arguments, a host question (no device call; KPX_EINVAL for arguments the entry refuses):
 * the kernel family in the order the families are asked, the number of partial slabs (1: the kernel writes dw itself) and the workspace
 * that call needs -- never more than kpx_conv2d_wgrad_workspace_bytes answers for the shape.  For tests and per-layer benchmarks. */
enum KpxWgradFamily {
    KPX_WGRAD_WSMALL = 0,       /* conv_wsmall.hip: tiny filters over very many pixels, the whole gradient in one workgroup's accumulators */
    KPX_WGRAD_WINO,             /* conv_wino.hip: F(2x2,3x3) weight gradient of the stride-1 3x3 SAME layers */
    KPX_WGRAD_ROWS_MERGED,      /* conv_wgrad_rows_merged_kernel: image inputs at high resolution, one tap per filter row */
    KPX_WGRAD_ROWS,             /* conv_wgrad_rows_kernel: few channels at high resolution, all taps from one LDS halo */
    KPX_WGRAD_GEMM3,            /* conv_gemm3.hip: bf16 matrix pipe (bf16x3 or bf16 operands); strided layers, and what TAP_ROWS does not take */
    KPX_WGRAD_TAP_ROWS,         /* conv_wgrad_tap_rows_kernel: Wo a multiple of 32, wave-uniform row chunks */
    KPX_WGRAD_GENERIC           /* conv_wgrad_kernel: any shape */
};
int kpx_conv2d_wgrad_plan(const float* x, int N, int Hi, int Wi, int Cin, int ldx,
                          const float* dy, int Ho, int Wo, int Cout, int lddy,
                          int KH, int KW, int stride, int pad_t, int pad_l, int arith,
                          int* family, int* splits, size_t* workspace_bytes);

/* dz = dy * act'(y) (y = the activated conv output; dz may alias dy): relu / leaky_relu(0.01) / tanh backward
 * (tf.nn.relu vgg.py:54, tf.nn.leaky_relu networks/__init__.py:145,148, tf.tanh layers.py:28 in stage-2 training). */
int kpx_act_bwd_f32(const float* dy, const float* y, float* dz, size_t n, int act, void* stream);

/* ---- per-channel reductions over P pixels: sum[c] = sum_p x[p,c] (double accumulation).
 *      Used for the conv bias gradient (tf.layers.conv2d use_bias, layers.py:9).
 *      `scratch` needs kpx_chan_reduce_scratch_bytes(C) bytes. */
size_t kpx_chan_reduce_scratch_bytes(int C);
int kpx_chan_sum_f32(const float* x, size_t P, int C, int ldx, float* sum_out, void* scratch, void* stream);

/* ---- batch norm: replaces tf.contrib.layers.batch_norm(eps=1e-5, center, scale) (layers.py:13-14) and the tf.nn.relu after it
 *      (networks/__init__.py:12...): act in {KPX_ACT_NONE, KPX_ACT_RELU}.
 *
 * Train mode: `groups` calls with batch statistics of their own, batched along N (the weight-sharing pose_encoder calls of a pair, reference
 * detector_translator_model.py:166-167): x = [groups][P pixels][C], one launch per phase for all groups.  groups = 1 is the single call.  A
 * group's results do not depend on how many groups share the call: `groups` calls with groups = 1, one per slice, give the same bits.
 *   forward: per group the batch mean and biased variance over P pixels (fp64 accumulation in a fixed order) -> mean, invstd = rsqrt(var + eps),
 *     [groups][C] (outputs, kept for the backward); moving_mean / moving_var (or NULL) updated in place once per group, in order, by the TF
 *     fused-BN rule (unbiased variance, moving -= (moving - batch) * (1 - decay)); then y = act((x - mean) * invstd * gamma + beta).
 *     tile_stats, or NULL for a reduction pass over x: the per-tile sums and sums of squares [tile][2][C] a convolution epilogue wrote
 *     (kpx_conv3x3_wino_f32, _wino43(b)_f32, _c16_f32, kpx_conv3x3_bf16s), tiles_per_group tiles per group.
 *   backward: dx, and dgamma / dbeta summed over the groups in order (accumulate != 0: added to what the destinations hold).  tile_stats, or
 *     NULL for a reduction pass over (dy, x): the per-tile sum(dz), sum(dz * (y - beta)) the epilogue of the data-gradient kernel that produced
 *     dy wrote (kpx_conv3x3_wino(43)(b)_f32 with tile_stats + bn_y + bn_beta, kpx_conv3x3_bf16s_bnbwd), tiles_per_group tiles per group; act
 *     must then be KPX_ACT_RELU and dy already zero wherever the output is, which those kernels guarantee.
 *   scratch: kpx_bn_train_scratch_bytes(C, groups) bytes.
 *   _bf16: x bf16; y bf16 (y_f32 = 0) or fp32 (y_f32 = 1: the tensor the fp32 key-point head reads); dy bf16 (dy_f32 = 0) or fp32; dx bf16.
 *     C and the pixel strides (elements) multiples of 8, pointers 16-byte aligned.  Statistics and parameter gradients stay fp32. */
size_t kpx_bn_train_scratch_bytes(int C, int groups);
int kpx_bn_train_fwd_f32(const float* x, size_t P, int groups, int C, int ldx, const float* tile_stats, size_t tiles_per_group,
                         float eps, const float* gamma, const float* beta, float* mean, float* invstd,
                         float* moving_mean, float* moving_var, float decay, float* y, int ldy, int act, void* scratch, void* stream);
int kpx_bn_train_bwd_f32(const float* dy, int lddy, const float* x, int ldx, size_t P, int groups, int C,
                         const float* mean, const float* invstd, const float* gamma, const float* beta, int act,
                         float* dx, int lddx, float* dgamma, float* dbeta, int accumulate,
                         const float* tile_stats, size_t tiles_per_group, void* scratch, void* stream);
int kpx_bn_train_fwd_bf16(const void* x, size_t P, int groups, int C, int ldx, const float* tile_stats, size_t tiles_per_group,
                          float eps, const float* gamma, const float* beta, float* mean, float* invstd,
                          float* moving_mean, float* moving_var, float decay, void* y, int ldy, int y_f32, int act, void* scratch, void* stream);
int kpx_bn_train_bwd_bf16(const void* dy, int lddy, int dy_f32, const void* x, int ldx, size_t P, int groups, int C,
                          const float* mean, const float* invstd, const float* gamma, const float* beta, int act,
                          void* dx, int lddx, float* dgamma, float* dbeta, int accumulate,
                          const float* tile_stats, size_t tiles_per_group, void* scratch, void* stream);
/* Inference mode (is_training = False: models/keypoint_model.py:48-50, final_model.py:62,68,95), from the moving statistics:
 *   kpx_bn_invstd_f32: invstd[c] = rsqrt(moving_var[c] + eps);
 *   kpx_bn_apply_f32: y = act((x - mean) * invstd * gamma + beta) over P pixels;
 *   kpx_bn_fold_conv_f32: the batch norm folded into the convolution in front of it: w_out[r][c] = w[r][c] * s[c], b_out[c] = (bias[c] -
 *     moving_mean[c]) * s[c] + beta[c] with s = gamma * rsqrt(moving_var + eps); w = [rows = kh*kw*Cin][C] (HWIO), bias may be NULL.
 *     conv(x, w_out) + b_out followed by ReLU then equals relu(batch_norm(conv(x, w) + bias)) up to fp32 rounding, without the pass over
 *     the activation. */
int kpx_bn_invstd_f32(const float* var, int C, float eps, float* invstd, void* stream);
int kpx_bn_apply_f32(const float* x, size_t P, int C, int ldx, const float* mean, const float* invstd,
                     const float* gamma, const float* beta, float* y, int ldy, int act, void* stream);
int kpx_bn_fold_conv_f32(const float* w, const float* bias, size_t rows, int C, const float* gamma, const float* beta,
                         const float* moving_mean, const float* moving_var, float eps, float* w_out, float* b_out, void* stream);

/* Fused Winograd F(4x4,3x3): the same contract as kpx_conv3x3_wino_f32 (forward, or data gradient with dgrad-transformed filters) with
 * 36 instead of 144 multiplies per 4x4 outputs; fp32 error ~2-3e-6 rel-L2 (F(2x2,3x3): ~4e-7).  Eligible when H % 16 == 0, W % 32 == 0,
 * K >= 16, Nn > 32 and the usual 16-B alignment; `u` comes from kpx_wino43_filter_transform(_batch)_f32 (kpx_wino43_u_bytes bytes,
 * descriptors as for kpx_wino_filter_transform_batch_f32).  Replaces the same tf.layers.conv2d call sites (reference
 * models/networks/__init__.py:13,22,80-97; models/networks/vgg.py:51). */
int kpx_conv3x3_wino43_eligible(int N, int H, int W, int K, int Nn, int ldin, const void* in_ptr);
size_t kpx_wino43_u_bytes(int Cin, int Cout);
int kpx_wino43_filter_transform_f32(const float* w_hwio, int Cin, int Cout, int dgrad, float* u, void* stream);
int kpx_wino43_filter_transform_batch_f32(const void* descs_dev, int n, void* stream);
/* Epilogue options, the same for kpx_conv3x3_wino43_f32 and kpx_conv3x3_wino43b_f32 (all NULL: the plain convolution):
 *   tile_stats alone: the batch-norm statistics of the output, as kpx_conv3x3_wino_f32's but per 4 x 16-pixel strip: tile_stats[strip][2][Nn],
 *     kpx_conv3x3_wino43_stats_tiles(N, H, W) strips (0 for packed 16 x 16 images: no statistics there), taken by kpx_bn_train_fwd_f32 as
 *     tile_stats;
 *   tile_stats + bn_y + bn_beta: data gradient towards a ReLU'd batch norm's output (the tensor bn_y this convolution read in the forward
 *     pass): out = dgrad * [bn_y > 0] and tile_stats[strip][2][Nn] = per strip sum(out), sum(out * (bn_y - beta)) -- kpx_bn_train_bwd_f32
 *     takes them instead of its own reduction pass (tf.gradients of tf.contrib.layers.batch_norm + tf.nn.relu, models/networks/layers.py:13-14).
 *     No bias, act = KPX_ACT_NONE;
 *   mask_y and / or pool_y, VGG19's options (models/networks/vgg.py:45-55), no tile_stats: mask_y zeroes the output where mask_y <= 0 (the
 *     ReLU backward of the tensor this data gradient belongs to); pool_y receives the 2x2 max-pool of the activated output ([N,H/2,W/2,Nn],
 *     pixel stride ld_pool).
 *   The bn and mask / pool forms need Nn % 64 == 0 and 16-B aligned rows everywhere.  Any other mix returns KPX_EINVAL. */
int kpx_conv3x3_wino43_f32(const float* in, int N, int H, int W, int K, int ldin, const float* u, const float* bias,
                           float* out, int Nn, int ldout, int act, const float* mask_y, int ld_mask, float* pool_y, int ld_pool,
                           float* tile_stats, const float* bn_y, int ld_bn_y, const float* bn_beta, void* stream);
size_t kpx_conv3x3_wino43_stats_tiles(int N, int H, int W);
/* The same F(4x4,3x3) layers FP32-EQUIVALENT ON THE BF16 MATRIX PIPE (csrc/conv_wino43b.hip): U pre-split into three exact bf16 terms in
 * fragment order by kpx_wino43b_filter_transform(_batch)_f32 (kpx_wino43b_u_bytes bytes; descriptors as for
 * kpx_wino_filter_transform_batch_f32), V split in registers after the input transform, six v_mfma_f32_32x32x16_bf16 products per block,
 * fp32 accumulate: the fp32 configuration's arithmetic (error vs float64 as the fp32-MFMA kernel's), not the bf16 mode.  Eligible when
 * (H % 16 == 0 and W % 32 == 0, or 16 x 16 images in even number: two to a workgroup, no tile_stats), K >= 16, K % 4 == 0, Nn > 32, ldin >= K,
 * 16-B alignment.  Arguments and epilogue options are kpx_conv3x3_wino43_f32's.  Replaces the same tf.layers.conv2d call sites (reference models/networks/layers.py:4-10 on
 * models/networks/__init__.py:13,22,80-97; models/networks/vgg.py:51). */
int kpx_conv3x3_wino43b_eligible(int N, int H, int W, int K, int Nn, int ldin, const void* in_ptr);
size_t kpx_wino43b_u_bytes(int Cin, int Cout);
int kpx_wino43b_filter_transform_f32(const float* w_hwio, int Cin, int Cout, int dgrad, void* u, void* stream);
int kpx_wino43b_filter_transform_batch_f32(const void* descs_dev, int n, void* stream);
int kpx_conv3x3_wino43b_f32(const float* in, int N, int H, int W, int K, int ldin, const void* u, const float* bias,
                            float* out, int Nn, int ldout, int act, const float* mask_y, int ld_mask, float* pool_y, int ld_pool,
                            float* tile_stats, const float* bn_y, int ld_bn_y, const float* bn_beta, void* stream);
/* 3x3 stride-1 SAME convolution PRODUCING exactly 16 channels on 16x16x4 MFMA blocks (no cout padding): the forward of the key-point
 * detector's last decoder block (64 -> 16, 16 -> 16 at full resolution, reference models/networks/__init__.py:50-54) and the data gradient
 * of its 16 -> 16 layer.  w_hwio is the layer's own filter: [3][3][K][16] forward, [3][3][16][K] for dgrad (K = gathered channels, a
 * multiple of 16; H, W multiples of 16).  tile_stats (or NULL): per 16x16-pixel tile sums as kpx_conv3x3_wino_f32 writes them. */
int kpx_conv3x3_c16_eligible(int N, int H, int W, int K, int Nn, int ldin, int ldout, const void* in_ptr);
int kpx_conv3x3_c16_f32(const float* in, int N, int H, int W, int K, int ldin, const float* w_hwio, int dgrad, const float* bias,
                        float* out, int ldout, int act, float* tile_stats, void* stream);
/* ---- tf.image.resize_images(x, 2x) legacy bilinear (models/networks/__init__.py:63,98). */
int kpx_resize2x_fwd_f32(const float* x, int N, int H, int W, int C, int ldx, float* y, int ldy, void* stream);
int kpx_resize2x_bwd_f32(const float* dy, int N, int H, int W, int C, int lddy, float* dx, int lddx, void* stream);

/* ---- channel-slice copy: one half of tf.concat(axis=-1) (networks/__init__.py:44, detector_translator_model.py:170). */
int kpx_copy_channels_f32(const float* src, int ldsrc, float* dst, int lddst, size_t P, int C, void* stream);

/* ---- key-point head: model_utils.get_coord twice + tf.stack (utils/model.py:63-70, networks/__init__.py:68-72).
 * logits [B,H,W,K] -> mu [B,K,2] (x,y) in [-1,1]; also the two softmax profiles prob_y [B,H,K], prob_x [B,W,K].
 * scratch: kpx_keypoint_head_scratch_bytes(B,H,W,K). */
size_t kpx_keypoint_head_scratch_bytes(int B, int H, int W, int K);
int kpx_keypoint_head_fwd_f32(const float* logits, int B, int H, int W, int K,
                              float* mu, float* prob_y, float* prob_x, void* scratch, void* stream);
int kpx_keypoint_head_bwd_f32(const float* dmu, const float* mu, const float* prob_y, const float* prob_x,
                              int B, int H, int W, int K, float* dlogits, void* stream);

/* ---- 1x1 head + key-point head in one: layers.conv(x, n_pts, kernel=1) followed by the two get_coord calls
 * (models/networks/__init__.py:54,68-72; utils/model.py:63-70).  The axis means commute with the 1x1 projection, so the logits
 * [B,H,W,K] are never formed.  x [B,H,W,C] contiguous (C % 4 == 0), wk [C,K] (the HWIO 1x1 filter), bias [K] or NULL.
 * Forward also returns the row / column sums of x (xs_y [B,H,C], xs_x [B,W,C]) that the backward needs.
 * Backward: dx [B,H,W,C] (or NULL), dw [C,K] and db [K] (each may be NULL; accumulate != 0 adds into them).
 * scratch: kpx_keypoint_head_proj_scratch_bytes(B,H,W,C,K) for either direction. */
size_t kpx_keypoint_head_proj_scratch_bytes(int B, int H, int W, int C, int K);
/* 1 when the folded operator takes the shape (C % 4 == 0, C <= 256, K <= 64, H, W in [2, 512], its profile rows within 64 KB of LDS);
 * otherwise the caller runs kpx_conv2d_fwd_f32 (1x1) followed by kpx_keypoint_head_fwd_f32 -- the same reference call sites. */
int kpx_keypoint_head_proj_eligible(int B, int H, int W, int C, int K);
int kpx_keypoint_head_proj_fwd_f32(const float* x, const float* wk, const float* bias, int B, int H, int W, int C, int K,
                                   float* mu, float* prob_y, float* prob_x, float* xs_y, float* xs_x, void* scratch, void* stream);
int kpx_keypoint_head_proj_bwd_f32(const float* dmu, const float* mu, const float* prob_y, const float* prob_x,
                                   const float* xs_y, const float* xs_x, const float* wk, int B, int H, int W, int C, int K,
                                   float* dx, float* dw, float* db, int accumulate, void* scratch, void* stream);

/* ---- Gaussian heat-map render: model_utils.get_gaussian_maps (utils/model.py:49-60).
 * mu [B,K,2] (x,y) -> maps [B,H,W,K] written with pixel stride ldy (NHWC directly; no BKHW transpose pass). */
int kpx_gaussian_maps_fwd_f32(const float* mu, int B, int K, int H, int W, double inv_std, float* maps, int ldy, void* stream);
int kpx_gaussian_maps_bwd_f32(const float* dmaps, int lddy, const float* mu, int B, int K, int H, int W, double inv_std,
                              float* dmu, void* stream);

/* ---- colourised key-point maps: colorize_point_maps(get_gaussian_maps(mu, [H,W], inv_std), colors) (utils/model.py:42-60) in one pass.
 * mu [N,K,2] (x,y), colors [K,3] fp32 on the device -> out [N,H,W,3] contiguous: out[n,h,w,c] = max_k g[n,h,w,k] * colors[k][c], g with the
 * bits of kpx_gaussian_maps_fwd_f32.  K in [1,64], H and W in [2,1024], inv_std > 0; nothing else is read or written (no [N,H,W,K] maps).
 * Added in ABI version 5. */
int kpx_point_maps_rgb_f32(const float* mu, int N, int K, int H, int W, double inv_std, const float* colors, float* out, void* stream);

/* ---- a strip of colourised pose frames (motion_generator_model.py:225-248): for every frame t of mu [N,T,K,2] (x,y), the frame of
 * kpx_point_maps_rgb_f32 (same bits) goes to columns [t*W, (t+1)*W) of out [N,H,T*W,3] (tf.concat(axis=2)).  recolour != 0 fuses the
 * reference's second colorize_point_maps over the 3-channel strip: out[...,c] = max_{i<3} strip[...,i] * colors[i][c] in fp32 (needs K >= 3).
 * K in [1,64], H and W in [2,1024], T*W <= 65536, inv_std > 0.  Added in ABI version 7. */
int kpx_point_seq_strip_rgb_f32(const float* mu, int N, int T, int K, int H, int W, double inv_std, const float* colors, int recolour,
                                float* out, void* stream);

/* ---- image summaries: TF 1.12 SummaryImageOp's float -> uint8 conversion (NormalizeFloatImage, summary_image_op.cc) per image, with the
 * reference's pre-map fused into both passes (never written out).  x fp32 NHWC [N,H,W,C], C in {1,3,4}; out uint8 [N,H,W,C].
 *   premap: KPX_PREMAP_IDENTITY x | KPX_PREMAP_X255 x*255 | KPX_PREMAP_UNIT255 (x+1)/2*255 | KPX_PREMAP_UNIT255_CLIP clip((x+1)/2*255, 0, 255)
 *           (clip_by_value = min then max, compare-select: NaN stays NaN, +-inf clips).
 *   A pixel is finite when all its channels are; min / max over finite pixels; min < 0: scale = 127/max(|min|,|max|), offset 128, else
 *   scale = 255/max, offset 0; scale 0 below 1e-6; finite pixels -> uint8(trunc(fl(fl(x*scale) + offset))), others -> (255,0,0,255)[:C].
 * Two launches (per-slice finite min / max into `work`, then per-image reduce + convert); work holds 2 * KPX_SUMMARY_SLICES * N floats.
 * Deterministic; no allocation, copy or synchronisation (capturable).  Added in ABI version 7. */
#define KPX_SUMMARY_SLICES 64
enum { KPX_PREMAP_IDENTITY = 0, KPX_PREMAP_X255 = 1, KPX_PREMAP_UNIT255 = 2, KPX_PREMAP_UNIT255_CLIP = 3 };
int kpx_summary_image_u8_f32(const float* x, int N, int H, int W, int C, int premap, float* work, uint8_t* out, void* stream);

/* ---- video-prediction frame metrics (evaluate.py --metrics): TF 1.12 tf.image.ssim and tf.image.psnr of frame pairs, DESIGN.md section 2.
 * a, b fp32 NHWC [N,H,W,C] contiguous, C in {1,3}, H and W in [11,1024], dynamic range L > 0 (finite) -> out fp32 [N,3] = (ssim, mse, psnr).
 *   SSIM: separable 11-tap Gaussian window (sigma 1.5), VALID, c1 = (0.01 L)^2, c2 = (0.03 L)^2, mean of lum * cs over positions per channel,
 *   then over channels; moments in fp64.  mse = mean (a - b)^2 over H*W*C; psnr = 20 log10(L) - 10 log10(mse) (+inf for mse == 0).
 *   png8 = 1: both inputs quantised as evaluate.py writes PNGs, q = clamp(uint8(trunc(fl(fl(0.5 * fl(x + 1)) * 255))), 0, 255) (NaN -> 0),
 *   and scored as q / 255 with L = 1 (the argument L is then not used beyond its check).
 * One launch, one workgroup per frame; frame n's result is bitwise the same for every N and position in the batch and from run to run.
 * No allocation, copy or synchronisation (capturable).  Added in ABI version 8. */
int kpx_frame_metrics_f32(const float* a, const float* b, int N, int H, int W, int C, float L, int png8, float* out, void* stream);

/* ---- VGG feature-space metrics (evaluate.py --vgg-metrics), DESIGN.md section 2: per frame pair of one layer's features fa, fb (fp32 NHWC
 * [N,H,W,C] contiguous on 16-byte aligned pointers, C % 4 == 0, 4 <= C <= 512, H and W in [1,1024], N >= 1) -> out fp32 [N,2] =
 * (cos_layer, l1_layer).  Per position over the C channels saa = sum a^2, sbb = sum b^2, dot = sum a b (fp32); its cosine is 1 where
 * saa == 0 and sbb == 0, 0 where exactly one of them is 0, else min(1, dot / sqrt(saa sbb)) in fp64; cos_layer = mean over positions,
 * l1_layer = mean |a - b| over positions and channels, both summed in fp64: identical inputs score exactly (1, 0).
 * Two launches: per-slab fp64 partials into `work` (kpx_feature_pair_metrics_workspace_bytes, 8-byte aligned; the slab count depends on
 * (H, W, C) alone), then a fixed-order fold per frame.  No atomics: frame n's result is bitwise the same for every N, every position in the
 * batch and every run.  No allocation, copy or synchronisation (capturable).  KPX_EINVAL before any device call for anything else.
 * Added in ABI version 10. */
size_t kpx_feature_pair_metrics_workspace_bytes(int N, int H, int W, int C);
int kpx_feature_pair_metrics_f32(const float* fa, const float* fb, int N, int H, int W, int C, float* work, float* out, void* stream);

/* ---- motion metrics (evaluate.py --motion-metrics), DESIGN.md section 2: how far the D draws of z of one sample lie apart in the 8-bit
 * frames, and the key-point error of each draw.  All three: no allocation, copy or synchronisation (capturable); no atomics; KPX_EINVAL
 * before any device call for a null pointer (other than the optional outputs), a pointer that is not 4-byte aligned or an argument out of
 * range.  Added in ABI version 13.
 *
 * kpx_draw_moments_add_f32: one draw into the accumulators.  Per value i < n, q = the 8-bit value of kpx_frame_metrics_f32's png8
 *   (clamp(uint8(trunc(fl(fl(0.5 * fl(x + 1)) * 255))), 0, 255), NaN -> 0): sum[i] += q, sumsq[i] += q * q (uint32, zeroed by the caller
 *   before the first draw).  Exact for up to 4096 draws (65025 * 4096 < 2^32).  Element-wise; 16-byte accesses when x, sum and sumsq are all
 *   16-byte aligned, 4-byte accesses otherwise -- the same bits either way.  n == 0 is a no-op.
 *
 * kpx_draw_diversity_f32: the accumulators of D draws of frames [N,H,W,C] (C in {1,3}, H and W in [1,1024], 2 <= D <= 4096, N >= 1).
 *   Per value V = D * sumsq - sum^2 = sum over the pairs i < j of draws of (q_i - q_j)^2, in 64-bit integers; per frame S = sum of V (uint64,
 *   exact: < 2^63 at the largest arguments).  div_mse[n] = fl32(double(S) / denom), denom = fl64(D (D - 1) / 2 * 65025) * fl64(H W C): the
 *   mean over pairs of draws of the MSE between their 8-bit frames on the q / 255 scale.  std_map (uint8 [N,H,W], or NULL for none):
 *   min(255, isqrt((4 * sum_c V) div (C * D^2))) = floor(2 sqrt(mean over channels of the population variance of q)), in 8-bit units, by an
 *   exact integer square root.  One workgroup per frame; integer sums, so frame n's result does not depend on N, its position or the run.
 *   Defined for accumulators that kpx_draw_moments_add_f32 filled with D draws (V >= 0); others wrap modulo 2^64.
 *
 * kpx_keypoint_draw_metrics_f32: pts fp32 [D,N,T,K,2] (the key points of D draws), real fp32 [N,T,K,2] (the labels), 1 <= D <= 4096,
 *   N, T, K >= 1.  l2[d,n,t] = (1/K) sum_k |pts[d,n,t,k] - real[n,t,k]|_2 (fp32 [D,N,T]); div[n,t] = 2 / (D (D - 1) K) * sum_{i<j} sum_k
 *   |pts[i,n,t,k] - pts[j,n,t,k]|_2 (fp32 [N,T], or NULL for none; must be NULL when D == 1).  Differences, squares, square roots and sums
 *   in fp64, one chain per output in ascending (i, j, k), not contracted; the result rounded once to fp32.  Non-finite inputs propagate to
 *   the outputs of their (d, n, t) / (n, t) alone. */
int kpx_draw_moments_add_f32(const float* x, size_t n, uint32_t* sum, uint32_t* sumsq, void* stream);
int kpx_draw_diversity_f32(const uint32_t* sum, const uint32_t* sumsq, int N, int H, int W, int C, int D, float* div_mse /*[N]*/,
                           uint8_t* std_map /*[N,H,W] or NULL*/, void* stream);
int kpx_keypoint_draw_metrics_f32(const float* pts /*[D,N,T,K,2]*/, const float* real /*[N,T,K,2]*/, int D, int N, int T, int K,
                                  float* l2 /*[D,N,T]*/, float* div /*[N,T] or NULL*/, void* stream);

/* ---- Frechet distance in VGG19 feature space (evaluate.py --frechet), DESIGN.md section 2: the two device passes under
 * kpx_amd.frechet.FrechetAccumulator.  Both: no allocation, copy or synchronisation (capturable); no atomics; KPX_EINVAL before any device
 * call for a null or misaligned pointer or an argument out of range.  Added in ABI version 16.
 *
 * kpx_feature_pool_f64: f fp32 NHWC [N,H,W,C] contiguous on a 16-byte aligned pointer, C % 4 == 0, 4 <= C <= 512, H and W in [1,1024],
 *   N >= 1 (kpx_feature_pair_metrics_f32's limits) -> pooled fp64 [N,C], pooled[n,c] = (sum over the H*W positions of f[n,.,.,c]) / (H*W).
 *   Every fp32 value is converted to fp64 (exactly) before its first addition; nothing is summed in fp32.  Two launches: per-slab fp64
 *   partials into `work` (kpx_feature_pool_workspace_bytes, 0 for a shape out of range; 8-byte aligned, as pooled), then a fold of a
 *   frame's slabs in ascending order and one division.  The slab count and the order of every addition depend on (H, W, C) alone: frame
 *   n's row is bitwise the same for every N, every position in the batch and every run.  N may exceed 65535.
 *
 * kpx_moments_add_f64: x fp64 [M,D] row-major, 1 <= M <= 2^20, 1 <= D <= 1024, 8-byte aligned pointers.  sum[j] += sum_m x[m,j] (fp64 [D])
 *   and outer[i,j] += sum_m x[m,i] * x[m,j] (fp64 [D,D], written in full), in place: the caller zeroes the accumulators once and adds
 *   batch after batch.  Each output element is owned by one lane of one workgroup, which reads the old value and adds the rows in ascending
 *   m, one fma per row for outer: bitwise reproducible from run to run, and outer stays bitwise symmetric when it starts symmetric. */
size_t kpx_feature_pool_workspace_bytes(int N, int H, int W, int C);
int kpx_feature_pool_f64(const float* f, int N, int H, int W, int C, double* work, double* pooled /*[N,C]*/, void* stream);
int kpx_moments_add_f64(const double* x /*[M,D]*/, int M, int D, double* sum /*[D]*/, double* outer /*[D,D]*/, void* stream);

/* ---- contact sheets (evaluate.py --actions), DESIGN.md section 4.4: frames of a rollout quantised to the bytes evaluate.py writes and
 * pasted into an 8-bit RGB sheet of rows x cols cells of H x W pixels, on the device.
 *   src fp32 [B,F,H,W,C] contiguous, C in {1,3} (C = 1 is written to the three channels); canvas uint8 [B, rows*H, cols*W, 3] contiguous.
 *   frames: J ints on the HOST (the one pointer of this ABI that is not device memory), each in [0,F), any order, repeats allowed; they
 *   are read before the call returns and travel by value in the launch arguments (no device index buffer: capturable).
 *   For every b < B and j < J: canvas[b, row*H + y, (col + j)*W + x, :] = q(src[b, frames[j], y, x, :]); nothing else is written.
 *   premap: KPX_SHEET_UNIT q = clamp(uint8(trunc(fl(fl(0.5 * fl(x + 1)) * 255))), 0, 255) -- kpx_frame_metrics_f32's png8, the bytes of
 *           _save_img(rescale=True); KPX_SHEET_RAW q = clamp(uint8(trunc(fl(x * 255))), 0, 255), the bytes of _save_img(rescale=False) for
 *           x in [0,1].  NaN -> 0 in both.
 *   Limits: B >= 1, F >= 1, H and W in [1,1024], rows and cols in [1,64], 1 <= J <= KPX_SHEET_MAX_FRAMES, 0 <= row < rows, col >= 0,
 *   col + J <= cols.  KPX_EINVAL before any device call for anything else, a null pointer, a src that is not 4-byte aligned or an unknown
 *   premap.
 * One launch: 16 source values per lane (four 16-byte loads, 16-byte stores) when W % 16 == 0 and src and canvas are 16-byte aligned, 4 per
 * lane (one 16-byte load, 4-byte stores) when W % 4 == 0, src is 16-byte and canvas 4-byte aligned, one value per lane otherwise -- the
 * same bytes on every path.  No allocation, copy or synchronisation.  Added in ABI version 14. */
#define KPX_SHEET_MAX_FRAMES 64
enum { KPX_SHEET_UNIT = 0, KPX_SHEET_RAW = 1 };
int kpx_sheet_paste_u8_f32(const float* src /*[B,F,H,W,C]*/, int B, int F, int H, int W, int C, const int* frames /*host [J]*/, int J,
                           uint8_t* canvas /*[B,rows*H,cols*W,3]*/, int rows, int cols, int row, int col, int premap, void* stream);

/* ---- animated grids (animate.py), DESIGN.md sections 2 and 4.4: one cell of a time-major canvas of rows x cols cells, T + 1 frames deep,
 * composed in one launch, optionally with key-point markers drawn on the frames.
 *   first fp32 [B,H,W,C] and seq fp32 [B,T,H,W,C] contiguous, C in {1,3} (C = 1 is written to the three channels); canvas uint8
 *   [B, T+1, rows*H, cols*W, 3] contiguous, any byte alignment.
 *   Pixels: canvas[b, 0, row*H + y, col*W + x, :] = q(first[b,y,x,:]) and canvas[b, t+1, row*H + y, col*W + x, :] = q(seq[b,t,y,x,:]) with
 *   q = KPX_SHEET_UNIT or KPX_SHEET_RAW exactly as kpx_sheet_paste_u8_f32 defines them (NaN -> 0).  Nothing outside the cell is written.
 *   Markers (radius r >= 1): pts_first fp32 [B,K,2] belongs to frame 0 and pts_seq fp32 [B,T,K,2] to frames 1..T; (x, y) = p[0], p[1] in the
 *   convention of kpx_gaussian_maps_fwd_f32 (index 0 is x -> columns; pixel i of n sits at -1 + 2 i / (n - 1)).  The centre in 1/16 pixel
 *   is cx = (int) rint(fl(fl(fl(x + 1) * 0.5f) * (float)(16 * (W - 1)))) and cy likewise with H: every step rounded to fp32, ties to even,
 *   none contracted into an fma.  A key point with a non-finite coordinate or with |x| > 4 or |y| > 4 draws nothing.  With
 *   d2 = (16 px - cx)^2 + (16 py - cy)^2 in exact integers, pixel (px, py) of the cell is covered by k iff d2 <= (16 r)^2; it takes
 *   colors[k] (device uint8 [K,3], any alignment) iff d2 <= (16 (r - 1))^2 and (0,0,0) otherwise: a one-pixel outline.  A pixel covered by
 *   several key points takes the marker of the LOWEST k.  Markers are clipped to their cell.  r = 0 reads neither the points nor the
 *   colours: those pointers may be NULL and K is ignored.
 *   Limits: B, T >= 1, B (T+1) < 2^31, H and W in [1,1024], C in {1,3}, rows and cols in [1,64], 0 <= row < rows, 0 <= col < cols, r in
 *   [0,16], K in [1,64] when r >= 1.  KPX_EINVAL before any device call for anything else, a null required pointer, an fp32 pointer that is
 *   not 4-byte aligned or an unknown premap.
 * One launch; a workgroup takes rows of one frame at a time and stages that frame's K centres and colours in LDS once.  The vector paths
 * are kpx_sheet_paste_u8_f32's (16 values per lane when W % 16 == 0 and first, seq and canvas are 16-byte aligned; 4 when W % 4 == 0, first
 * and seq are 16-byte and canvas 4-byte aligned; one otherwise) -- the same bytes on every path.  No allocation, copy, synchronisation or
 * atomics (capturable).  Added in ABI version 21. */
int kpx_cell_frames_u8_f32(const float* first /*[B,H,W,C]*/, const float* seq /*[B,T,H,W,C]*/, int B, int T, int H, int W, int C,
                           const float* pts_first /*[B,K,2]*/, const float* pts_seq /*[B,T,K,2]*/, int K,
                           const uint8_t* colors /*device [K,3]*/, int radius,
                           uint8_t* canvas /*[B,T+1,rows*H,cols*W,3]*/, int rows, int cols, int row, int col, int premap, void* stream);

/* ---- animated GIFs (evaluate.py --gif), DESIGN.md sections 2 and 4.4: 8-bit RGB canvases to palette indices on the device, and GIF's LZW on
 * the host.  Integer arithmetic throughout: the same bits in any order of execution.  Added in ABI version 20.
 *   kpx_color_hist_add_u32: rgb uint8 [G,n,3] (any byte alignment), hist uint32 [G,32768,4], updated in place:
 *     hist[g, cell] += (count, sum r, sum g, sum b) over the pixels of group g with cell = (r >> 3) << 10 | (g >> 3) << 5 | b >> 3.
 *     1 <= n <= 2^24 (the sums of one call cannot overflow; the caller zeroes hist, with a memset node under capture), 1 <= G <= 65535.
 *     One launch; LDS and global integer atomics.
 *   kpx_palette_map_u8: rgb uint8 [G,T,H,Wc,3] and idx uint8 [G,T,H,Wc] (any byte alignment, any width), palette uint8 [G,256,3], sizes
 *     DEVICE int32 [G].  With P = min(max(sizes[g], 1), pmax): idx = the smallest j < P that minimises (r - pr)^2 + (g - pg)^2 + (b - pb)^2
 *     in int32.  dither = A in [0,64]: before the search each channel c becomes clamp(c + (((2 M[y & 3][x & 3] - 15) A + 16) >> 5), 0, 255)
 *     (arithmetic shift; M = [[0,8,2,10],[12,4,14,6],[3,11,1,9],[15,7,13,5]]; y the row of the frame, x the column of the canvas); A = 0 is
 *     the plain search.  1 <= pmax <= 256 bounds every group's size on the host; G <= 65535, T H Wc < 2^31.  One launch, no atomics.
 *   Both: no allocation, copy or synchronisation (capturable); KPX_EINVAL before any device call for a null pointer, a hist or sizes that is
 *   not 4-byte aligned, or a size outside the limits.
 *   kpx_gif_lzw_u8 (HOST pointers, no device call): idx[n], every index < 1 << min_code_size, min_code_size in [2,8] -> GIF's LZW byte
 *     stream without sub-blocks (clear code first, least significant bit first, width + 1 when the next free code equals 2^width, up to 12,
 *     clear and reset at 4096 codes, end code last).  Returns the bytes written, or KPX_EINVAL for a bad argument or a stream that does not
 *     fit out_bytes; kpx_gif_lzw_bound(n) bytes always fit.  n <= 2^30. */
int kpx_color_hist_add_u32(const uint8_t* rgb /*[G,n,3]*/, int G, size_t n, uint32_t* hist /*[G,32768,4]*/, void* stream);
int kpx_palette_map_u8(const uint8_t* rgb /*[G,T,H,Wc,3]*/, int G, int T, int H, int Wc, const uint8_t* palette /*[G,256,3]*/,
                       const int* sizes /*device [G]*/, int pmax, int dither, uint8_t* idx /*[G,T,H,Wc]*/, void* stream);
size_t kpx_gif_lzw_bound(size_t n);
int kpx_gif_lzw_u8(const uint8_t* idx /*host [n]*/, size_t n, int min_code_size, uint8_t* out /*host*/, size_t out_bytes);

/* ---- key-point retargeting (FinalModel.run(drive=...), evaluate.py --drive), DESIGN.md sections 2 and 4.4: the key-point sequence of a
 * rollout whose motion comes from outside the motion generator.  src_first fp32 [B,K,2]: the source images' detected key points; drv_first
 * fp32 [B,K,2] and drv_seq fp32 [B,T,K,2]: the drivers' key points at frame 0 and at frames 1..T; out fp32 [B,T,K,2].  Sample b is driven by
 * sample j = (b + shift) mod B.  For every (b, t, k, axis):
 *   KPX_RETARGET_HOLD             out = src_first[b,k]                                                      (a bit copy)
 *   KPX_RETARGET_ABSOLUTE         out = drv_seq[j,t,k]                                                      (a bit copy)
 *   KPX_RETARGET_RELATIVE         out = src_first[b,k] + (drv_seq[j,t,k] - drv_first[j,k])
 *   KPX_RETARGET_RELATIVE_SCALED  out = src_first[b,k] + s_b * (drv_seq[j,t,k] - drv_first[j,k])
 * s_b = sqrt(v_src / v_drv) with v = sum_k |p_k - c|^2 and c = (sum_k p_k) / K of src_first[b] and of drv_first[j]; s_b = 1 unless both v
 * are finite and > 0.  The last two modes in fp64, every operation rounded once (no fma), the sums in the order k = 0..K-1, the result
 * rounded to fp32 once, at the store.  A sample reads its own source and its own driver alone: non-finite inputs reach the outputs that
 * read them and no others.  Pointers a mode does not read may be NULL (HOLD: drv_first, drv_seq; ABSOLUTE: src_first, drv_first).
 *   Limits: B, T >= 1, 1 <= K <= 1024, 0 <= shift < B, B*T*K*2 < 2^31; every pointer the mode uses 4-byte aligned.  KPX_EINVAL before any
 *   device call for anything else, a null pointer the mode uses or an unknown mode.
 * One launch, one workgroup per sample; 16-byte accesses when K is even and every pointer the mode uses is 16-byte aligned, 4-byte accesses
 * otherwise -- the same values on both paths.  No allocation, copy, synchronisation or atomics (capturable).  Added in ABI version 15. */
enum { KPX_RETARGET_HOLD = 0, KPX_RETARGET_ABSOLUTE = 1, KPX_RETARGET_RELATIVE = 2, KPX_RETARGET_RELATIVE_SCALED = 3 };
int kpx_points_retarget_f32(const float* src_first /*[B,K,2]*/, const float* drv_first /*[B,K,2]*/, const float* drv_seq /*[B,T,K,2]*/,
                            int B, int T, int K, int shift, int mode, float* out /*[B,T,K,2]*/, void* stream);

/* ---- key-point resampling in time and the speed of a key-point sequence (csrc/resample.hip; FinalModel.run(frames=, rate=), animate.py and
 * evaluate.py --frames / --rate), DESIGN.md sections 2 and 4.4.  No reference counterpart.  Two entries added to ABI version 25: no existing
 * signature changed, so the number stays.
 *
 * kpx_points_resample_f32: the knots P_0 = first fp32 [B,K,2] and P_1..P_N = seq fp32 [B,N,K,2] stand at the times 0..N.  Output frame
 * j = 1..N*F stands at the time j / F and is stored at index j - 1 of out fp32 [B,N*F,K,2].  With i = j div F and r = j mod F, for every
 * (b, k, axis):
 *   r == 0                out = P_i                                                 (a bit copy: F = 1 is the identity, every knot survives,
 *                                                                                    NaN payloads included)
 *   KPX_RESAMPLE_LINEAR   out = P_i + s * (P_{i+1} - P_i),  s = (double)r / (double)F
 *   KPX_RESAMPLE_CUBIC    out = h00 * P_i + h10 * m_i + h01 * P_{i+1} + h11 * m_{i+1}   (the cubic Hermite form, added from the left)
 *                         s2 = s * s, s3 = s2 * s, h00 = (2 s3 - 3 s2) + 1, h10 = (s3 - 2 s2) + s, h01 = -2 s3 + 3 s2, h11 = s3 - s2;
 *                         Catmull-Rom tangents m_i = (P_{i+1} - P_{i-1}) / 2 for 0 < i < N, one-sided at the ends: m_0 = P_1 - P_0,
 *                         m_N = P_N - P_{N-1}.  A straight-line motion is reproduced on the whole range, a parabola on the interior
 *                         intervals 1 <= i <= N - 2.
 * In fp64 from the fp32 knots, every operation rounded once (no fma), in the order written, the result rounded to fp32 once, at the store.
 * NOTHING IS CLAMPED: a cubic may overshoot [-1, 1] slightly between knots that touch the border; the Gaussian maps and the markers take any
 * value.  An output reads the knots of its own sample, point and stencil alone (P_i, P_{i+1}; CUBIC also P_{i-1} and P_{i+2} where they
 * exist): a non-finite knot reaches exactly the frames whose stencil holds it and no others.
 *   Limits: B, N, K, F >= 1, K <= KPX_RESAMPLE_MAX_POINTS, F <= KPX_RESAMPLE_MAX_RATE, N >= 2 for CUBIC, B*N*F*K*2 < 2^31; the three pointers
 *   4-byte aligned.  KPX_EINVAL before any device call for anything else, a null pointer or an unknown mode.
 * One launch, one thread per output item; 16-byte accesses when K is even and the three pointers are 16-byte aligned, 4-byte accesses otherwise
 * -- the same values on both paths.  No allocation, copy, synchronisation or atomics (capturable).
 *
 * kpx_points_speed_f64: speed[b,t] = scale * ((sum_k |P_t[k] - P_{t-1}[k]|) / K) for t = 1..T, stored at index t - 1 of speed double [B,T], with
 * P_0 = first fp32 [B,K,2] and P_1..P_T = seq fp32 [B,T,K,2]: the mean distance the points move between consecutive frames.  In fp64: the
 * differences dx, dy, then dx * dx + dy * dy, then sqrt, the terms added in the order k = 0..K-1, one division by K, one multiplication by
 * `scale`, every operation rounded once.  `scale` is the rate F of a resampled sequence, so the unit stays "per source frame".
 *   Limits: B, T >= 1, 1 <= K <= KPX_RESAMPLE_MAX_POINTS, B*T*K*2 < 2^31; first and seq 4-byte, speed 8-byte aligned; KPX_EINVAL before any
 *   device call otherwise.  One launch, one thread per (b, t), no atomics (capturable). */
enum { KPX_RESAMPLE_LINEAR = 0, KPX_RESAMPLE_CUBIC = 1 };
#define KPX_RESAMPLE_MAX_POINTS 1024
#define KPX_RESAMPLE_MAX_RATE 64
int kpx_points_resample_f32(const float* first /*[B,K,2]*/, const float* seq /*[B,N,K,2]*/, int B, int N, int K, int F, int mode,
                            float* out /*[B,N*F,K,2]*/, void* stream);
int kpx_points_speed_f64(const float* first /*[B,K,2]*/, const float* seq /*[B,T,K,2]*/, int B, int T, int K, double scale,
                         double* speed /*[B,T]*/, void* stream);

/* ---- translator heads + blend: mask = sigmoid(raw[...,3]); final = im*mask + crude*(1-mask)
 *      (networks/__init__.py:87-89, detector_translator_model.py:174).  raw4 [P,4] = crude(3) ‖ mask logit(1). */
int kpx_head_blend_fwd_f32(const float* im, const float* raw4, size_t P, float* final_out, float* crude_out, float* mask_out, void* stream);
int kpx_head_blend_bwd_f32(const float* dfinal, const float* im, const float* raw4, size_t P, float* draw4, void* stream);

/* ---- VGG input transform: rgb in [-1,1] -> (x+1)/2*255 -> BGR - mean
 *      (detector_translator_model.py:262-263, vgg.py:16-19). */
int kpx_vgg_prep_fwd_f32(const float* rgb, size_t P, float* bgr, void* stream);
int kpx_vgg_prep_bwd_f32(const float* dbgr, size_t P, float* drgb, void* stream);
/* The same transform of the 8-bit frame evaluate.py writes: q = clamp(uint8(trunc(fl(fl(0.5 * fl(x + 1)) * 255))), 0, 255) (NaN -> 0) as
 * kpx_frame_metrics_f32's png8, bgr = q - mean on the 0..255 scale (no round trip through [-1,1]).  Added in ABI version 10. */
int kpx_vgg_prep_png8_f32(const float* rgb, size_t P, float* bgr, void* stream);

/* ---- tf.nn.max_pool 2x2 s2 SAME (vgg.py:45-46). */
int kpx_maxpool2_fwd_f32(const float* x, int N, int H, int W, int C, float* y, void* stream);
int kpx_maxpool2_bwd_f32(const float* dy, const float* x, int N, int H, int W, int C, float* dx, void* stream);

/* ---- perceptual L1 term: loss = mean|f[0:half] - f[half:2*half]| (detector_translator_model.py:280-284).
 * fwd writes one float; bwd writes d/d f_pred (second half only) = -sign(gt-pred) * g,
 * g = gscale_host * (gscale_dev ? *gscale_dev : 1).  scratch >= 8 KiB. */
int kpx_l1_pair_fwd_f32(const float* f, size_t half, float* loss_out, void* scratch, void* stream);
int kpx_l1_pair_bwd_f32(const float* f, size_t half, const float* gscale_dev, float gscale_host, float* dpred, void* stream);
/* Gradient arriving at a VGG19 feature y = relu(conv) in one pass: ReLU mask of (max-pool backward of dy_pooled + L1 backward), i.e.
 * kpx_maxpool2_bwd_f32 + kpx_l1_pair_bwd_f32 + their sum + the ReLU backward fused (reference vgg.py:43,45-55 and
 * detector_translator_model.py:274-289).  f = [gt; pred] halves of the feature [2B,H,W,C], C % 4 == 0; dy_pooled [B,ceil(H/2),ceil(W/2),C]
 * or NULL for the last feature; d [B,H,W,C]. */
int kpx_vgg_feat_bwd_f32(const float* f, size_t half, const float* gscale_dev, float gscale_host, const float* dy_pooled,
                         int B, int H, int W, int C, float* d, void* stream);

/* ---- tf.nn.sigmoid_cross_entropy_with_logits + reduce_mean (detector_translator_model.py:249-254,265-267).
 * labels: the first n0 logits get label0, the next n1 get label1 (n1 may be 0).
 * loss_out[3] = { mean(group0) + mean(group1), mean(group0), mean(group1) }.
 * bwd: dlogits = (sigmoid(x) - label) * g / n_group, g = gscale_host * (gscale_dev ? *gscale_dev : 1). */
int kpx_sigmoid_xent_fwd_f32(const float* logits, size_t n0, float label0, size_t n1, float label1, float* loss_out, void* stream);
int kpx_sigmoid_xent_bwd_f32(const float* logits, size_t n0, float label0, size_t n1, float label1,
                             const float* gscale_dev, float gscale_host, float* dlogits, void* stream);

/* ---- tf.train.AdamOptimizer.apply (detector_translator_model.py:198-202) over one flat bucket.
 * alpha = lr*sqrt(1-b2^t)/(1-b1^t) (host); g is pre-scaled by gscale (1/world_size for DP). */
int kpx_adam_tf_flat_f32(float* p, const float* g, float* m, float* v, size_t n,
                         float alpha, float beta1, float beta2, float eps, float gscale, void* stream);
/* The same update with alpha read from DEVICE memory (one float): for launches captured into a HIP graph, whose arguments are frozen at
 * capture time while alpha (learning-rate decay :193-195, bias correction) changes every step; the caller refreshes *alpha_dev before each replay. */
int kpx_adam_tf_flat_dev_alpha_f32(float* p, const float* g, float* m, float* v, size_t n,
                                   const float* alpha_dev, float beta1, float beta2, float eps, float gscale, void* stream);

/* ---- the step guard (train.py --guard), DESIGN.md section 4.4: a bucket whose gradient holds a NaN or an Inf skips its update.  The
 * verdict is a record in DEVICE memory, one per bucket, written by the health pass and read by the update and the restore themselves, so
 * the captured step needs no host synchronisation.  All three entries: no allocation, copy or synchronisation (capturable); no atomics;
 * KPX_EINVAL before any device call for a null or misaligned pointer or n == 0.  Added in ABI version 22. */
typedef struct KpxGuardHealth {      /* 32 bytes, 8-byte aligned */
    uint32_t nonfinite;              /* this step's gradient values that are NaN or +-Inf (saturates at 2^32 - 1) */
    uint32_t skipped_total;          /* updates skipped so far */
    uint32_t skipped_run;            /* consecutive skips; a clean update resets it to 0 */
    uint32_t updates;                /* guarded updates so far, skipped ones included */
    double sumsq;                    /* sum of g^2 over the finite values */
    float maxabs;                    /* max |g| over the finite values */
    float pad_;
} KpxGuardHealth;
/* kpx_grad_health_f32: one read pass over g fp32 [n] (4-byte aligned, n >= 1; sizes beyond 2^31 are fine) -> health->nonfinite, ->sumsq
 *   and ->maxabs; the four counters are left alone, a second call overwrites the first call's result.  Two launches: per-slab partials into
 *   `work` (kpx_grad_health_workspace_bytes(n) bytes, 8-byte aligned), then a one-workgroup fold.  Every value is converted to fp64 before
 *   it is squared (the square is exact), a slab is 16384 consecutive elements whatever the grid, and the order of every addition depends
 *   on n alone: the record is bitwise the same from run to run and whether g is 16-byte aligned (16-byte loads) or not (4-byte loads).
 * kpx_adam_tf_flat_guarded_f32: with health->nonfinite == 0, kpx_adam_tf_flat_dev_alpha_f32 bit for bit (one shared definition of the
 *   arithmetic); otherwise p, m and v are left bitwise untouched.  One lane bumps ->updates and either ->skipped_total and ->skipped_run,
 *   or clears ->skipped_run.  p, g, m, v 16-byte aligned, n >= 1.
 * kpx_guard_restore_f32: dst[0:n] = src[0:n] bit for bit if health->nonfinite != 0, nothing otherwise (4-byte aligned pointers; 16-byte
 *   accesses when both are 16-byte aligned). */
size_t kpx_grad_health_workspace_bytes(size_t n);
int kpx_grad_health_f32(const float* g, size_t n, void* work, KpxGuardHealth* health, void* stream);
int kpx_adam_tf_flat_guarded_f32(float* p, const float* g, float* m, float* v, size_t n, const float* alpha_dev,
                                 float beta1, float beta2, float eps, float gscale, KpxGuardHealth* health, void* stream);
int kpx_guard_restore_f32(float* dst, const float* src, size_t n, const KpxGuardHealth* health, void* stream);

/* ---- gradient norms (train.py --clip-norm / --grad-stats), DESIGN.md section 4.4.  Added in ABI version 24.
 * kpx_adam_tf_flat_clipped_f32: kpx_adam_tf_flat_guarded_f32 with tf.clip_by_global_norm over the bucket.  The launch reads the record the
 *   health pass wrote: N = (double)gscale * sqrt(health->sumsq) in fp64 (gscale = 1 / world, so every rank derives the same N from the
 *   exchanged sum).  health->nonfinite != 0: the guarded kernel's skip bit for bit (counters bumped; p, m, v and *clip untouched).
 *   N <= clip_norm (N == clip_norm, sumsq == 0 and clip_norm = +Inf included): the guarded update bit for bit, clip->scale = 1.  Otherwise
 *   the walk runs with gs = (float)((double)gscale * ((double)clip_norm / N)), clip->scale = (float)(clip_norm / N) and
 *   clip->clipped_total += 1.  Every lane derives gs from the same record; one lane writes clip->norm = (float)N, ->scale and the counters.
 *   No allocation, copy, synchronisation or atomics (capturable).  p, g, m, v 16-byte aligned, alpha_dev and clip 4-byte, health 8-byte,
 *   n >= 1, clip_norm > 0 (+Inf allowed); KPX_EINVAL before any device call for anything else (a NaN clip_norm included). */
typedef struct KpxClipState {        /* 16 bytes */
    float norm;                      /* N of the last update that was not skipped */
    float scale;                     /* what that update multiplied the gradient by on top of gscale: 1, or clip_norm / N < 1 */
    uint32_t clipped_total;          /* updates so far with N > clip_norm */
    uint32_t pad_;
} KpxClipState;
int kpx_adam_tf_flat_clipped_f32(float* p, const float* g, float* m, float* v, size_t n, const float* alpha_dev,
                                 float beta1, float beta2, float eps, float gscale, float clip_norm,
                                 KpxGuardHealth* health, KpxClipState* clip, void* stream);

/* kpx_grad_segment_stats_f32: per-variable statistics of a flat bucket, one deterministic segmented reduction (csrc/grad_stats.hip).
 *   The caller cuts every variable [offset, offset + numel) of the bucket into chunks of at most KPX_SEG_CHUNK elements, counted from the
 *   variable's own start, and lists them in DEVICE memory: chunks[c] = (start, len, seg) in ascending order of (seg, start), and
 *   ranges[s] = (first chunk, chunk count) of variable s.  Launch 1 takes one chunk per workgroup and writes one partial per chunk into
 *   `work` (kpx_grad_segment_stats_workspace_bytes(n_chunks) bytes, 8-byte aligned); launch 2 folds each variable's partials in ascending
 *   order with a fixed tree into out[s].  Every value is converted to fp64 before it is squared; which lane owns an element is counted
 *   from the chunk's start, so the result is a function of the values and the table alone: bitwise the same from run to run and whether a
 *   chunk starts 16-byte aligned (16-byte loads) or only 4-byte aligned (4-byte loads).  Elements outside every chunk are never read.
 *   The kernels clamp every table entry to [0, n) and KPX_SEG_CHUNK, so a wrong table gives wrong numbers, never an access outside g[0:n].
 *   p may be NULL (sumsq_p = 0).  No allocation, copy, synchronisation or atomics (capturable).  g, p 4-byte aligned, chunks 8-byte,
 *   ranges 4-byte, work and out 8-byte; n, n_chunks, n_segs >= 1, n_chunks and n_segs < 2^31; KPX_EINVAL before any device call otherwise. */
#define KPX_SEG_CHUNK 16384
typedef struct KpxSegChunk {         /* 16 bytes */
    uint64_t start;                  /* first element, an index into the bucket */
    uint32_t len;                    /* 1 .. KPX_SEG_CHUNK */
    uint32_t seg;                    /* the variable it belongs to */
} KpxSegChunk;
typedef struct KpxSegRange {         /* 8 bytes */
    uint32_t first;                  /* the variable's first chunk */
    uint32_t count;                  /* and how many it has */
} KpxSegRange;
typedef struct KpxSegStats {         /* 32 bytes */
    double sumsq_g;                  /* sum of g^2 over the variable's finite gradient values */
    double sumsq_p;                  /* sum of p^2 over its finite parameter values; 0 when p == NULL */
    float maxabs_g;                  /* max |g| over the finite values */
    uint32_t nonfinite_g;            /* gradient values that are NaN or +-Inf (saturates at 2^32 - 1) */
    uint32_t pad_[2];
} KpxSegStats;
size_t kpx_grad_segment_stats_workspace_bytes(size_t n_chunks);
int kpx_grad_segment_stats_f32(const float* g, const float* p /* may be NULL */, size_t n, const KpxSegChunk* chunks, size_t n_chunks,
                               const KpxSegRange* ranges, size_t n_segs, void* work, KpxSegStats* out, void* stream);

/* ---- the averaged generator (train.py --ema), DESIGN.md section 4.4: an exponential moving average of a bucket's parameters, kept beside
 * training and read only for inference.  Both entries: no allocation, copy or synchronisation (capturable); no atomics; the result is a
 * function of the operands alone.  They return KPX_EINVAL before any device call on a null or misaligned pointer or n == 0.
 * kpx_ema_flat_f32: ema[i] += (p[i] - ema[i]) * *rate_dev for i < n (tf assign_moving_average with rate = 1 - decay), computed as
 *   d = p - ema (one rounding), ema = fma(d, rate, ema) (one rounding).  rate_dev is read on the device.  health may be NULL; otherwise the
 *   launch writes nothing when health->nonfinite != 0 (the guarded update was skipped).  health is only read, p is never written.
 *   ema, p 16-byte aligned, rate_dev 4-byte, health 8-byte aligned, n >= 1 (sizes beyond 2^31 are fine).
 * kpx_swap_flat_f32: exchanges a[0:n] and b[0:n] word for word (NaN payloads and -0 survive).  a, b 16-byte aligned, a != b, n >= 1; the
 *   ranges must not overlap. */
int kpx_ema_flat_f32(float* ema, const float* p, size_t n, const float* rate_dev, const KpxGuardHealth* health /* may be NULL */, void* stream);
int kpx_swap_flat_f32(float* a, float* b, size_t n, void* stream);

/* ---- evaluate.py / FinalModel rollout (forward only).  Dense layers run as 1x1 kpx_conv2d_fwd_f32.
 * LSTMCell pointwise part (models/networks/layers.py:17-21): gates [B,4U] = (i,j,f,o) pre-activations. */
int kpx_lstm_pointwise_f32(const float* gates, const float* c_prev, float forget_bias, float* c_out, float* h_out,
                           int B, int U, void* stream);
/* tf.tile over a new time axis (models/final_model.py:58-66,85-87): dst[((b*T+t)*pix+p)*lddst+c] = src[(b*pix+p)*ldsrc+c]. */
int kpx_tile_batch_f32(const float* src, int ldsrc, int B, int T, int pix, int C, float* dst, int lddst, void* stream);
/* blend with the T-times tiled source image + optional clip_by_value(-1,1) of crude and final (final_model.py:95-99). */
int kpx_head_blend_tiled_fwd_f32(const float* im, const float* raw4, size_t P, int HW, int T, int clip,
                                 float* final_out, float* crude_out, float* mask_out, void* stream);

/* ---- utilities */
int kpx_fill_f32(float* p, size_t n, float value, void* stream);
int kpx_axpy_f32(float* y, const float* x, size_t n, float a, void* stream);   /* y += a*x (gradient accumulation) */

/* Stage-2 training (next row, SURVEY 8f-4 last item: models/motion_generator_model.py).
 * LSTMCell backward of one step (layers.py:17-21): gates [B,4U] pre-activations (i,j,f,o), c_prev [B,U] (NULL = zeros),
 * dh [B,U], dc_in [B,U] (NULL = zeros) -> dgates [B,4U], dc_prev [B,U]. */
int kpx_lstm_pointwise_bwd_f32(const float* gates, const float* c_prev, const float* dh, const float* dc_in, float forget_bias,
                               float* dgates, float* dc_prev, int B, int U, void* stream);
/* Whole-sequence LSTM layer with zero initial state (dynamic_rnn / unrolled cells, networks/__init__.py:105-138); the time loop
 * runs inside the library.  x [T,B,In], kernel [In+U,4U], bias [4U]; xin [T,B,In+U], gates [T,B,4U], cs, hs [T,B,U] are written
 * (and are what the backward needs); zeros_bu = B*U zero floats; workspace as for kpx_conv2d_fwd_f32 / _dgrad_f32 of a
 * [B,1,1,In+U] x [1,1,In+U,4U] convolution.  Backward: dhs [T,B,U] -> dgates [T,B,4U] and (if non-NULL) dx [T,B,In];
 * scratch dxin [B,In+U], dh [B,U], dc0 [B,U] (zero-filled by the caller), dc1 [B,U].  The weight gradient is then ONE
 * kpx_conv2d_wgrad_f32 over xin / dgates viewed as [T*B,1,1,.], the bias gradient one kpx_chan_sum_f32 of dgates. */
int kpx_lstm_layer_fwd_f32(const float* x, int T, int B, int In, const float* kernel, const float* bias, int U,
                           float* xin, float* gates, float* cs, float* hs, const float* zeros_bu,
                           void* workspace, size_t workspace_bytes, void* stream);
int kpx_lstm_layer_bwd_f32(const float* dhs, int T, int B, int In, const float* kernel, int U,
                           const float* gates, const float* cs, float* dgates, float* dx,
                           float* dxin, float* dh, float* dc0, float* dc1,
                           void* workspace, size_t workspace_bytes, void* stream);
/* z = mu + stddev*eps and the KL term of motion_generator_model.py:146,291-293 on logit = [mu | stddev] [B,2V]; backward from dz
 * (NULL = zeros) and the KL gradient gkl_dev[0] * gkl_host. */
int kpx_vae_sample_kl_fwd_f32(const float* logit, const float* eps, float* z, float* kl_out, int B, int V, void* stream);
int kpx_vae_sample_kl_bwd_f32(const float* logit, const float* eps, const float* dz, const float* gkl_dev, float gkl_host,
                              float* dlogit, int B, int V, void* stream);

/* Input pipeline (next row): uint8 frames -> float32 in [-1,1] on the device, with the reference's arithmetic
 * dst = float32(src / 255.0) * 2 - 1  (data/image_pair_dataloader.py:163-164 float64 division, tf.data float32 cast,
 * map_fn :64-69 in float32).  Lets the loader ship uint8 over PCIe (a quarter of the bytes). */
int kpx_u8_to_unit_f32(const unsigned char* src, size_t n, float* dst, void* stream);

/* Host utility (no device access): CRC-32C of n bytes continuing from `crc` (0 to start) -- the checksum of TensorFlow V2
 * checkpoint bundles (next row; models/base_model.py:74-91 saves / restores through tf.train.Saver). */
unsigned int kpx_crc32c_host(unsigned int crc, const void* data, size_t n);

/* The strided / 4x4 / 1x1 layers (discriminator, the encoders' stride-2 layers: networks/__init__.py:16-24,141-151) in the bf16 configuration:
 * the gather convolution of kpx_conv2d_fwd_f32 / _dgrad_f32 / _wgrad_f32 with KPX_ARITH_BF16 on bf16 TENSORS (pixel strides in elements, multiples
 * of 8; 16-byte aligned).  y / dx are bf16 (y_f32 / dx_f32 = 0) or fp32; y_in (dgrad, optional): the bf16 activated tensor dx is the gradient
 * of (as kpx_conv2d_dgrad_act_f32).  Workspaces: the fp32 entries' queries.  KPX_EINVAL for shapes the bf16-pipe kernels do not take (Cin, Cout
 * multiples of 8 / 4 and >= 16): convert and use the fp32 entry. */
int kpx_conv2d_fwd_bf16(const void* x, int N, int Hi, int Wi, int Cin, int ldx, const float* w, int KH, int KW, const float* bias,
                        void* y, int y_f32, int Ho, int Wo, int Cout, int ldy, int stride, int pad_t, int pad_l, int act,
                        void* workspace, size_t workspace_bytes, void* stream);
int kpx_conv2d_dgrad_bf16(const void* dy, int N, int Ho, int Wo, int Cout, int lddy, const float* w, int KH, int KW,
                          void* dx, int dx_f32, int Hi, int Wi, int Cin, int lddx, int stride, int pad_t, int pad_l,
                          const void* y_in, int ld_y_in, int act_in, void* workspace, size_t workspace_bytes, void* stream);
int kpx_conv2d_wgrad_bf16(const void* x, int N, int Hi, int Wi, int Cin, int ldx, const void* dy, int Ho, int Wo, int Cout, int lddy,
                          float* dw, int KH, int KW, int stride, int pad_t, int pad_l, void* workspace, size_t workspace_bytes, void* stream);

/* Image-input layers in the bf16 configuration (models/networks/pose_encoder.py conv_1 7x7x3 -> 32, img_discriminator.py conv_0 4x4/s2 3 -> 64,
 * vgg.py:51 conv1_1 3x3x3 -> 64): the image stays fp32, what the layer produces / receives is bf16.  KPX_EINVAL (-1) for shapes the LDS-resident
 * image kernels do not take (the caller converts and uses the fp32 entries).
 *   fwd:   x fp32 [N,Hi,Wi,Cin<=4] contiguous -> y bf16 (pixel stride ldy elements), Cout <= 64
 *   dgrad: dy bf16 (pixel stride lddy, a multiple of 8; Cout a multiple of 16) -> dx fp32 [N,Hi,Wi,Cin] (3x3/s1 and 4x4/s2 filters)
 *   wgrad: x fp32, dy bf16 (pixel stride a multiple of 4) -> dw fp32 HWIO; workspace = kpx_conv2d_wgrad_workspace_bytes */
int kpx_conv_image_fwd_bf16(const float* x, int N, int Hi, int Wi, int Cin, const float* w, int KH, int KW, const float* bias,
                            void* y, int Ho, int Wo, int Cout, int ldy, int stride, int pad_t, int pad_l, int act, void* stream);
int kpx_conv_image_dgrad_bf16(const void* dy, int N, int Ho, int Wo, int Cout, int lddy, const float* w, int KH, int KW,
                              float* dx, int Hi, int Wi, int Cin, int lddx, int stride, int pad_t, int pad_l, void* stream);
int kpx_conv_image_wgrad_bf16(const float* x, int N, int Hi, int Wi, int Cin, int ldx, const void* dy, int Ho, int Wo, int Cout, int lddy,
                              float* dw, int KH, int KW, int stride, int pad_t, int pad_l, void* workspace, size_t workspace_bytes, void* stream);

/* Weight gradient of a 3x3 stride-1 SAME layer in the bf16 configuration (gradient of layers.py:6-9): x bf16 [N,H,W,>=Cin] (pixel stride ldx;
 * the pad channels up to the next multiple of 8 must hold finite values), dy bf16 [N,H,W,>=Cout], dw fp32 HWIO [3,3,Cin,Cout], written.
 * W a multiple of 16; workspace = kpx_conv3x3_wgrad_bf16_workspace_bytes (partial slabs of the pixel splits, summed in fixed order). */
int kpx_conv3x3_wgrad_bf16_eligible(int N, int H, int W, int Cin, int ldx, int Cout, int lddy, const void* x, const void* dy);
size_t kpx_conv3x3_wgrad_bf16_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int kpx_conv3x3_wgrad_bf16(const void* x, int N, int H, int W, int Cin, int ldx, const void* dy, int Cout, int lddy,
                           float* dw, void* workspace, size_t workspace_bytes, void* stream);

/* ---- bf16 STORAGE variants of the streaming kernels (BASELINE configs[2]): bf16 tensors in HBM, fp32 arithmetic, fp64 reductions, fp32
 *      statistics / parameter gradients.  C and the pixel strides (in ELEMENTS) are multiples of 8, pointers 16-byte aligned, unless an
 *      entry says otherwise.  Reference call sites as the fp32 entries of the same name above. */
/* dst[p][0:C] = src[p][0:C] with conversion: kind 0 = f32 -> bf16, 1 = bf16 -> f32, 2 = bf16 -> bf16 (tf.concat channel slices); any C.
 * kind 3 = f32 -> bf16 into a contiguous 8-channel tensor (lddst = 8, C <= 8) whose channels C .. 7 are written as zeros. */
int kpx_cast_channels(const void* src, int ldsrc, void* dst, int lddst, size_t P, int C, int kind, void* stream);
int kpx_chan_sum_bf16(const void* x, size_t P, int C, int ldx, float* sum_out, void* scratch, void* stream);
/* dz = dy * act'(y) on bf16 tensors, n % 8 == 0; act in {KPX_ACT_NONE, KPX_ACT_RELU, KPX_ACT_LRELU}.  Unlike kpx_act_bwd_f32 it has no tanh
 * backward: KPX_ACT_TANH and any other value are refused with KPX_EINVAL (nothing is written). */
int kpx_act_bwd_bf16(const void* dy, const void* y, void* dz, size_t n, int act, void* stream);
int kpx_resize2x_fwd_bf16(const void* x, int N, int H, int W, int C, int ldx, void* y, int ldy, void* stream);
int kpx_resize2x_bwd_bf16(const void* dy, int N, int H, int W, int C, int lddy, void* dx, int lddx, void* stream);
int kpx_maxpool2_fwd_bf16(const void* x, int N, int H, int W, int C, void* y, void* stream);
int kpx_vgg_feat_bwd_bf16(const void* f, size_t half, const float* gscale_dev, float gscale_host, const void* dy_pooled,
                          int B, int H, int W, int C, void* d, void* stream);
int kpx_l1_pair_fwd_bf16(const void* f, size_t half, float* loss_out, void* scratch, void* stream);

/* ---- The image-pair augmentation on frames resident in HBM (ABI 9): what ImagePairDataLoader.render does with PIL
 *      (data/image_pair_dataloader.py:71-165: rotate, resize to short side 128, crop, flip; utils/data.py:8-35: one of ten filters),
 *      byte for byte, from a table of per-frame decisions the host draws (kpx_amd/resident.py).
 *
 *   frames     one flat uint8 buffer of decoded RGB frames in HWC order; frame_off[i] = byte offset of frame i (a multiple of 16)
 *   rows       [n_rows][KPX_AUG_ROW_INTS] int32, one row per output frame:
 *                0 frame number      1 w   2 h (size of the source frame)      3 x0   4 y0 (crop origin in the RESIZED frame)
 *                5 flags (KPX_AUG_FLIP | KPX_AUG_ROTATE | KPX_AUG_IDENTITY = the enhancer's factor is 1.0: the tile passes unchanged)
 *                6 filter id: -1 none, 0..5 the ImageFilter kernels of `kernels`, 6..9 Sharpness / Brightness / Color / Contrast
 *                7 the enhancer's factor (the bits of the float32 nearest to filt_val * 0.1)
 *                8..13 a0..a5: Pillow's 16.16 fixed-point NEAREST rotation, xin = (a2 + a1*y + a0*x) >> 16, yin = (a5 + a4*y + a3*x) >> 16
 *                14 / 15 offset into resize_tabs and entry stride of the horizontal pass (w -> resized width), 16 / 17 of the vertical pass
 *                18.. unused (the loader records the resized size there)
 *   resize_tabs  int32; a table of a pass is n_out entries of `stride` ints: first input index, tap count, the taps' 22-bit coefficients
 *                (a pass Pillow skips, n_in == n_out, is the table {i, 1, 1 << 22})
 *   kernels    [6][KPX_AUG_KERNEL_FLOATS] float32: size (3 or 5), float32(offset) + 0.5f, size*size coefficients float32(k / scale)
 *   band_rows_cap  rows of the horizontally resized frame one 16-row band of the tile may need (LDS: cap * 384 bytes)
 *   tiles      uint8 [n_rows][128][128][3], lsum int32 [n_rows][KPX_AUG_BANDS] (luminance sums): written by geometry, read by filter
 *   out        float32 [n_rows][128][128][3] in [-1,1] (the arithmetic of kpx_u8_to_unit_f32)
 *
 * The kernels trust the table: the HOST rejects, before the launch, a frame number outside the store, a crop window outside the resized
 * frame, a filter id outside -1..9, a frame side above KPX_AUG_MAX_SIDE, a pass with more than KPX_AUG_MAX_TAPS taps or with
 * 255 * sum|k| >= 2^31, and a band that needs more than KPX_AUG_MAX_BAND_ROWS rows (kpx_amd.resident.check_rows).  With those bounds
 * no 32-bit sum overflows (rotation: |a1*y + a0*x + a2| < 2^29). */
#define KPX_AUG_ROW_INTS 24
#define KPX_AUG_FLIP 1
#define KPX_AUG_ROTATE 2
#define KPX_AUG_IDENTITY 4
#define KPX_AUG_BAND 16
#define KPX_AUG_BANDS 8
#define KPX_AUG_KERNEL_FLOATS 32
#define KPX_AUG_MAX_SIDE 2048
#define KPX_AUG_MAX_TAPS 32
#define KPX_AUG_MAX_BAND_ROWS 160
#define KPX_AUG_MAX_ROWS 32768
int kpx_augment_geometry_u8(const unsigned char* frames, const int64_t* frame_off, const int32_t* rows, int n_rows,
                            const int32_t* resize_tabs, int band_rows_cap, unsigned char* tiles, int32_t* lsum, void* stream);
int kpx_augment_filter_f32(const unsigned char* tiles, const int32_t* lsum, const int32_t* rows, int n_rows, const float* kernels,
                           float* out, void* stream);

/* The same two launches on square tiles of `side` x `side` pixels (model.image_size; the two entries above are side = 128, bit for bit).
 * Added to ABI version 25; no signature above changes.
 *
 *   side       a multiple of KPX_AUG_BAND in [KPX_AUG_TILE_MIN, KPX_AUG_TILE_MAX]: the tile has side / KPX_AUG_BAND bands
 *   tiles      uint8 [n_rows][side][side][3], lsum int32 [n_rows][side / KPX_AUG_BAND], out float32 [n_rows][side][side][3]
 *   band_rows_cap  as above; the workgroup keeps cap * side * 3 bytes in LDS, at most KPX_AUG_LDS_BYTES (above 64 KB the launch opts in
 *                  with hipFuncAttributeMaxDynamicSharedMemorySize).  The host refuses a video whose band needs more
 *                  (kpx_amd.resident.check_rows) and the entry answers KPX_EINVAL before any launch.
 *   Contrast   the degenerate grey is int(mean luminance + 0.5) over side * side pixels, computed as (2 * sum + side^2) / (2 * side^2)
 *              in integers: exact for every side. */
#define KPX_AUG_TILE_MIN 32
#define KPX_AUG_TILE_MAX 256
#define KPX_AUG_LDS_BYTES 122880
int kpx_augment_geometry_sq_u8(const unsigned char* frames, const int64_t* frame_off, const int32_t* rows, int n_rows,
                               const int32_t* resize_tabs, int band_rows_cap, int side, unsigned char* tiles, int32_t* lsum, void* stream);
int kpx_augment_filter_sq_f32(const unsigned char* tiles, const int32_t* lsum, const int32_t* rows, int n_rows, const float* kernels,
                              int side, float* out, void* stream);

/* ---- The key-point half of the sequence loader on pseudo labels resident in HBM (ABI 12): what SequenceDataLoader.render does to the
 *      key points with numpy (data/sequence_dataloader.py:105-198: gather 33 sets, rotate, flip, scale; the one-hot action code),
 *      bit for bit, from a table of per-sample decisions the host draws (kpx_amd/resident.py).  One launch per batch.
 *
 *   labels     one flat float32 buffer: every stored video's pseudo-label array [len_v][n_points][2], one after the other
 *   label_off  label_off[v] = element offset of video v's array in `labels`
 *   rows       [n_rows][KPX_SEQ_ROW_INTS] int32, one row per sample:
 *                0 video number      1 im_idx (label row of the start frame)
 *                2 gap: >= 1 reads the rows im_idx + gap * i, i = 0..32, and computes in float32; 0 is the short-video form, rows
 *                  im_idx .. im_idx + 16 with every odd entry the float32 mean of its neighbours, then float64 arithmetic rounded once
 *                3 flags (KPX_SEQ_ROTATE | KPX_SEQ_FLIP | KPX_SEQ_SCALE): an operation whose flag is set is PERFORMED, also for angle 0 and
 *                  scale 1.0 (the host does, and it decides signs of zero); none set: the gathered values pass through
 *                4 the angle's index into `trig` (angle + 15)
 *                5 / 6 low and high 32 bits of the scale, a double (randint(70, 120) / 100.0 on the host)
 *                7 action index: action_code[row] is its one-hot vector
 *   trig       [KPX_SEQ_ANGLES][2] double: cos and sin of radians(-angle), angle = -15..15, from the host's libm
 *   keypoints  float32 [n_rows][n_points][2] (set 0), real_seq float32 [n_rows][32][n_points][2] (sets 1..32),
 *   action_code float32 [n_rows][n_action]
 *
 * No product or sum is fused and nothing but the halving of the short form divides.  The kernel trusts the table: the HOST rejects, before
 * the launch, a video number outside the store, im_idx + 32 * gap (or im_idx + 16) beyond the video's label rows, an angle index outside
 * 0..30, an action index outside 0..n_action-1 and more than KPX_SEQ_MAX_ROWS rows (kpx_amd.resident.SequencePlanner.check_rows). */
#define KPX_SEQ_ROW_INTS 8
#define KPX_SEQ_ROTATE 1
#define KPX_SEQ_FLIP 2
#define KPX_SEQ_SCALE 4
#define KPX_SEQ_LEN 33
#define KPX_SEQ_ANGLES 31
#define KPX_SEQ_MAX_ROWS 4096
#define KPX_SEQ_MAX_POINTS 256
#define KPX_SEQ_MAX_ACTIONS 256
int kpx_keypoint_seq_augment_f32(const float* labels, const int64_t* label_off, const int32_t* rows, int n_rows, int n_points,
                                 int n_action, const double* trig, float* keypoints, float* real_seq, float* action_code, void* stream);

/* ---- key-point action classifier (csrc/classify.hip) ---------------------------------------------------------------------------------
 * Softmax cross-entropy of logits [B][A] against label rows [B][A] (tf.nn.softmax_cross_entropy_with_logits + reduce_mean) and the scores
 * evaluate.py --action-accuracy reads.  1 <= A <= 1024, 1 <= B, M <= 2^20; every pointer 4-byte aligned; null or out-of-range arguments
 * return KPX_EINVAL before any device call.  Each entry is ONE launch on `stream` (capturable), uses no float atomics and computes in
 * fp64 in a fixed order, rounding to fp32 once.
 *   fwd    lse_out[i] = max_j + log(sum_j exp(logits_ij - max_j)); loss_out[0] = (sum_i -sum_j labels_ij (logits_ij - lse_i)) / B, the
 *          rows added in ascending order (lse_i unrounded inside the loss).
 *   bwd    dlogits_ij = g / B * (exp(logits_ij - lse_i) - labels_ij), lse the fp32 values fwd wrote, g = gscale_host * (gscale_dev ?
 *          *gscale_dev : 1) as in kpx_l1_pair_bwd_f32.  (TensorFlow's gradient: exact when every label row sums to 1.)
 *   scores pred_i = the lowest index among the row's maxima; rank_i = 1 + #{j != t : logits_ij >= logits_it}, t = target[i] (a tie counts
 *          against the model); logp_i = logits_it - lse_i; confusion[t][pred_i] += 1 (int32 [A][A], integer atomics, may be NULL).
 *          A row with a non-finite logit gets pred = -1, rank = A, logp = NaN and is left out of `confusion`.  The caller keeps
 *          target inside [0, A) (kpx_amd.ops.class_scores refuses others); the kernel reads nothing for such a row and answers
 *          rank = A, logp = NaN. */
int kpx_softmax_xent_fwd_f32(const float* logits, const float* labels, int B, int A, float* loss_out, float* lse_out, void* stream);
int kpx_softmax_xent_bwd_f32(const float* logits, const float* labels, const float* lse, int B, int A, const float* gscale_dev,
                             float gscale_host, float* dlogits, void* stream);
int kpx_class_scores_f32(const float* logits, const int32_t* target, int M, int A, int32_t* pred, int32_t* rank, float* logp,
                         int32_t* confusion, void* stream);

/* ---- equivariance score of the key-point detector (csrc/stability.hip; make_pseudo_labels.py --stability, kpx_amd/stability.py), DESIGN.md
 * section 2: warp every frame by a known affine map, detect again, and compare the detected points with the mapped originals.  No reference
 * counterpart (the reference never scores its detector).  Both entries: ONE launch on `stream`, no allocation, copy, synchronisation or
 * atomics (capturable), nothing written outside their outputs; KPX_EINVAL before any device call for a null or misaligned pointer (4 bytes;
 * 8 for the double tables) or a size out of range.  Added in ABI version 18.
 *
 * kpx_affine_warp_f32: in fp32 [N,H,W,C] contiguous, C in {1,3}, H and W in [1,1024], N >= 1; rows int32 [R], the source frame of each
 *   output row (any order, repeats allowed); coef double [R][6], the INVERSE map of each row in pixel units; out fp32 [R,H,W,C];
 *   1 <= R <= KPX_WARP_MAX_ROWS.  For output pixel (x, y) of row r, with c = coef[r] and v = in[rows[r]]:
 *     sx = (c0*x + c1*y) + c2,  sy = (c3*x + c4*y) + c5, clamped to [0, W-1] and [0, H-1] (edge replication; NaN -> 0)
 *     x0 = floor(sx), lowered to max(W-2, 0) if it exceeds W-2;  fx = sx - x0;  x1 = min(x0 + 1, W-1);  y0, fy, y1 alike
 *     top = (1-fx)*v[y0,x0] + fx*v[y0,x1],  bot = (1-fx)*v[y1,x0] + fx*v[y1,x1],  out = (1-fy)*top + fy*bot
 *   Everything in fp64, no product or sum fused (as kpx_keypoint_seq_augment_f32), the result cast to fp32 once: bit for bit what numpy
 *   float64 gives in this order.  Maps that send pixels to pixels (identity, integer shifts, flips, quarter turns of a square frame) copy
 *   input bits (fx, fy in {0, 1}; only a -0.0 beside a value of the other sign comes out as +0.0).  Frames are finite by contract (0 * inf
 *   is NaN).  The clamp keeps every tap inside the frame for any coefficients; the frame numbers are trusted: the HOST rejects, before the
 *   launch, a frame number outside [0, N) and a non-finite coefficient (kpx_amd.ops.affine_warp).
 *   A workgroup writes a 16-row tile of one output row; 16-byte stores when W % 4 == 0 and out is 16-byte aligned, 4-byte stores otherwise
 *   -- the same bits on both paths; `in` needs 4-byte alignment only.
 *
 * kpx_equivariance_scores_f32: pts fp32 [N][K][2] (x, y), the detector on the original frames; pts_w fp32 [R][K][2], the detector on the
 *   warped frames; rows int32 [R] as above (trusted alike); fwd double [R][6], the FORWARD map of each row in the normalised coordinates of
 *   the key points ([-1,1], pixel i at -1 + 2i/(res-1)); 1 <= K <= 1024, 1 <= R <= KPX_EQUIV_MAX_ROWS.  For row r and point k, p =
 *   pts[rows[r]][k], q = pts_w[r][k], m = fwd[r]:
 *     target = ((m0*p.x + m1*p.y) + m2, (m3*p.x + m4*p.y) + m5)
 *     out[r][k] = (err, moved) (fp32 [R][K][2]): err = |q - target|, moved = |target - p|, Euclidean, in fp64 (no fma), each rounded once
 *     valid[r][k] (uint8 [R][K]) = 1 when p, q and target are finite and target lies in [-1,1] x [-1,1], bounds included; else 0
 *     frame_mean[r] (fp32 [R][2]) = (mean err, mean moved) over the row's valid points: the unrounded fp64 values added in ascending k,
 *       divided by their number, rounded once; (NaN, NaN) when there are none.  n_valid[r] (int32 [R]) = their number.
 *   One wavefront per row; the order of every addition is fixed. */
#define KPX_WARP_MAX_ROWS 65536
#define KPX_EQUIV_MAX_ROWS (1 << 20)
int kpx_affine_warp_f32(const float* in /*[N,H,W,C]*/, int N, int H, int W, int C, const int32_t* rows /*[R]*/, const double* coef /*[R][6]*/,
                        int R, float* out /*[R,H,W,C]*/, void* stream);
int kpx_equivariance_scores_f32(const float* pts /*[N,K,2]*/, const float* pts_w /*[R,K,2]*/, const int32_t* rows /*[R]*/,
                                const double* fwd /*[R][6]*/, int R, int K, float* out /*[R,K,2]*/, uint8_t* valid /*[R,K]*/,
                                float* frame_mean /*[R,2]*/, int32_t* n_valid /*[R]*/, void* stream);

/* ---- landmark regression from the key points to annotated joints (csrc/joints.hip; make_pseudo_labels.py --joints, kpx_amd/joints.py),
 * a linear map from the K points the detector found on a frame to the frame's J annotated joints, fitted per joint on the
 * train split and scored on both.  No reference counterpart (the reference never reads Penn Action's annotations).  phi_f = (x_0, y_0, ...,
 * x_{K-1}, y_{K-1}, 1) is the feature row of frame f, the fp32 key points pts[f] widened to fp64, and D = 2K + 1.  All three entries: ONE
 * launch on `stream`, no allocation, copy, synchronisation or atomics (capturable), every sum in an order that does not depend on the
 * launch, nothing written outside their outputs, all arithmetic in fp64; KPX_EINVAL before any device call for a null or misaligned pointer
 * (4 bytes for fp32, 8 for double and int64 arrays, none for uint8) or a size out of range: 1 <= K <= KPX_JOINT_MAX_POINTS, 1 <= J <=
 * KPX_JOINT_MAX_JOINTS, 1 <= F <= KPX_JOINT_MAX_FRAMES, 1 <= A <= KPX_JOINT_MAX_ALPHAS.  Added in ABI version 19.
 *
 * kpx_joint_targets_f32: xy fp32 [F][J][2], the annotated joints in the original frame's pixel coordinates; vis uint8 [F][J]; bbox fp32
 *   [F][4] = (x0, y0, x1, y1) in the same pixels; map double [4] = (ax, bx, ay, by) (kpx_amd.joints.crop_map).  For frame f and joint j:
 *     t = (ax*x + bx, ay*y + by), the product and the sum each rounded once in fp64 (no fma);  target[f][j] (fp32 [F][J][2]) = t, cast once
 *     mask[f][j] (uint8 [F][J]) = 1 when vis[f][j] != 0, x and y are finite and the unrounded t lies in [-1,1] x [-1,1], bounds included;
 *       else 0 (a non-finite map gives a NaN t and so 0)
 *     norm[f] (fp32 [F]) = max(|ax|*(x1-x0), |ay|*(y1-y0)), each difference and product rounded once, cast once: the longer side of the box
 *       in the normalised units of the crop, the frame's PCK normaliser.  NaN unless the four numbers are finite and x1 > x0 and y1 > y0.
 *
 * kpx_joint_moments_add_f64: pts fp32 [F][K][2]; target fp32 [F][J][2]; mask uint8 [F][J].  In place, for every joint j:
 *     G[j]  (double [J][D][D]) += sum_f use[f][j] phi_f phi_f^T
 *     Bm[j] (double [J][D][2]) += sum_f use[f][j] phi_f target[f][j]^T
 *     n[j]  (int64 [J])        += sum_f use[f][j],      use[f][j] = mask[f][j] != 0 and all 2K coordinates of pts[f] are finite
 *   Each element starts from its stored value and takes the frames with use = 1 in ascending f, ONE fma each: G[j][a][b] = fma(phi_f[a],
 *   phi_f[b], G[j][a][b]), Bm[j][a][c] = fma(phi_f[a], target[f][j][c], Bm[j][a][c]); a frame with use = 0 touches nothing.  So F frames in
 *   one call and the same frames in any split into consecutive calls give the same bits, a G that starts bitwise symmetric stays so, and a
 *   frame with a non-finite key point contributes to no joint.  The caller zeroes the accumulators before the first call and keeps the
 *   targets of the frames it masks in finite (kpx_joint_targets_f32 does).
 *
 * kpx_joint_scores_f32: pts, target, mask as above; norm fp32 [F]; W double [J][D][2], the regressor; alpha double [A], the PCK thresholds.
 *   Per frame and joint, every product and sum rounded once (no fma):
 *     p = (0 + phi_f[0]*W[j][0] + phi_f[1]*W[j][1] + ...) in ascending d, both components;  pred[f][j] (fp32 [F][J][2]) = p, cast once
 *     e = sqrt(dx*dx + dy*dy), (dx, dy) = p - target[f][j];  err[f][j] (fp32 [F][J]) = e, cast once
 *     valid = mask[f][j] != 0 and all 2K coordinates of pts[f] are finite;  pck = valid and norm[f] is finite
 *     hits[f][j] (uint8 [F][J]): bit a set when pck and e <= alpha[a]*norm[f] (the unrounded e); 0 for an entry that is not pck
 *   Per call and joint, written (not added to):
 *     sum_err[j] (double [J]) = the unrounded e of the valid entries, added in ascending f from 0;  count[j] (int64 [J]) = their number
 *     pck_count[j] (int64 [J]) = the number of pck entries;  hit_count[j][a] (int64 [J][A]) = the number of entries with bit a set
 *   pred and err of an entry that is not valid are written as computed (NaN for a non-finite key point).  A W[j] of NaN (a joint without a
 *   train frame) gives sum_err[j] = NaN and no hits wherever it has valid entries. */
#define KPX_JOINT_MAX_POINTS 64
#define KPX_JOINT_MAX_JOINTS 32
#define KPX_JOINT_MAX_FRAMES (1 << 20)
#define KPX_JOINT_MAX_ALPHAS 8
int kpx_joint_targets_f32(const float* xy /*[F,J,2]*/, const uint8_t* vis /*[F,J]*/, const float* bbox /*[F,4]*/, const double* map /*[4]*/,
                          int F, int J, float* target /*[F,J,2]*/, uint8_t* mask /*[F,J]*/, float* norm /*[F]*/, void* stream);
int kpx_joint_moments_add_f64(const float* pts /*[F,K,2]*/, const float* target /*[F,J,2]*/, const uint8_t* mask /*[F,J]*/, int F, int K, int J,
                              double* G /*[J,D,D]*/, double* Bm /*[J,D,2]*/, int64_t* n /*[J]*/, void* stream);
int kpx_joint_scores_f32(const float* pts /*[F,K,2]*/, const float* target /*[F,J,2]*/, const uint8_t* mask /*[F,J]*/, const float* norm /*[F]*/,
                         const double* W /*[J,D,2]*/, const double* alpha /*[A]*/, int F, int K, int J, int A, float* pred /*[F,J,2]*/,
                         float* err /*[F,J]*/, uint8_t* hits /*[F,J]*/, double* sum_err /*[J]*/, int64_t* count /*[J]*/,
                         int64_t* pck_count /*[J]*/, int64_t* hit_count /*[J,A]*/, void* stream);

/* ---- nearest training motion of a key-point sequence (csrc/novelty.hip; evaluate.py --novelty, kpx_amd/novelty.py), DESIGN.md section 2.
 * No reference counterpart.  Added in ABI version 25.
 *
 *   labels, label_off   the resident label store of kpx_keypoint_seq_augment_f32
 *   windows     int32 [W][KPX_NEAREST_ROW_INTS] = (video number, im_idx, gap, action index): the candidate windows, in listing order; the
 *               window id w is the row number.  Frame t = 1..32 of window w is the loader's un-augmented real_seq[t - 1] in fp32: for gap >= 1
 *               label row im_idx + gap * t, for gap == 0 rows im_idx + (t >> 1) with every odd t the float32 mean of its neighbours (float32
 *               add, float32 halving) -- the values kpx_keypoint_seq_augment_f32 delivers with no flag set, bit for bit.
 *   order       int32 [n_groups][KPX_NEAREST_GROUP]: the window ids grouped by action class, ascending inside a class, every class starting a
 *               new block and its last block closed with -1 pads; group_first int32 [n_action + 1]: class a owns the blocks group_first[a] ..
 *               group_first[a + 1] - 1 (kpx_amd.novelty.WindowIndex.plan builds both)
 *   queries     fp32 [Q][32][n_points][2]; exclude int32 [Q] or NULL: the windows of that video number are skipped for the query (-1: none)
 *   d2          double [Q][n_action], code int32 [Q][n_action]
 *
 * d2(q, w, m) = (sum_t sum_k ex^2 + ey^2) / (32 n_points), ex = (double)q.x - (double)v.x, ey = (double)q.y - (double)v.y, and for the mirrored
 * candidate (m = 1, only with `mirror`) ex = (double)q.x + (double)v.x.  All in fp64: the conversions and differences are exact; lane l of one
 * wavefront adds the points j = l, l + 64, ... (j = (t - 1) n_points + k) in ascending order with s = fma(ex, ex, s), s = fma(ey, ey, s) from
 * s = 0, the 64 lane sums are added in the xor butterfly 32, 16, 8, 4, 2, 1, and the total is divided by 32 n_points once.  The bits of
 * d2(q, w, m) therefore depend on the query's and the window's values and on n_points alone: not on w, q, Q, W or the grid.
 * Per query and class a the result is the minimum of d2 over the candidates of class a and code = 2 w + m of the minimising one; ties go to the
 * lowest code; a candidate whose d2 is not finite is never chosen; a class without a chosen candidate gets d2 = +inf and code = -1.
 * Two launches on `stream`, no atomics: per block of `order` and query one partial (d2, code) goes into `workspace`, then one thread per (q, a)
 * combines the class's blocks in ascending order.  workspace: kpx_seq_nearest_workspace_bytes(n_groups, Q) bytes (0 for sizes out of range),
 * 8-byte aligned.  Capturable.
 * Limits: 1 <= n_points <= KPX_SEQ_MAX_POINTS, 1 <= n_action <= KPX_SEQ_MAX_ACTIONS, 1 <= Q <= KPX_NEAREST_MAX_QUERIES, 1 <= W <=
 * KPX_NEAREST_MAX_WINDOWS (W < 2^30: a code fits an int32), n_groups <= ceil(W / KPX_NEAREST_GROUP) + n_action; labels, label_off, queries,
 * workspace and d2 8-byte aligned, the int32 tables 4-byte.  Anything else is KPX_EINVAL before any device call.  The kernel trusts the tables
 * and clamps nothing: the HOST rejects, before the launch, a video number outside the store, a window that leaves its video's label rows and an
 * action index outside 0..n_action-1 (kpx_amd.novelty.WindowIndex.check). */
#define KPX_NEAREST_ROW_INTS 4
#define KPX_NEAREST_GROUP 64
#define KPX_NEAREST_MAX_QUERIES 4096
#define KPX_NEAREST_MAX_WINDOWS ((1 << 30) - 1)
size_t kpx_seq_nearest_workspace_bytes(int n_groups, int Q);
int kpx_seq_nearest_f32(const float* labels, const int64_t* label_off, const int32_t* windows /*[W][4]*/, int W, const int32_t* order,
                        const int32_t* group_first /*[n_action + 1]*/, int n_groups, const float* queries /*[Q,32,K,2]*/,
                        const int32_t* exclude /*[Q] or NULL*/, int Q, int n_points, int n_action, int mirror, void* workspace,
                        size_t workspace_bytes, double* d2 /*[Q,A]*/, int32_t* code /*[Q,A]*/, void* stream);

/* ---- k nearest rows of a set, exact in fp64 (csrc/prdc.hip; evaluate.py --prdc, kpx_amd/prdc.py), DESIGN.md sections 2 and 4.4.  No reference
 * counterpart.  Added without a version change: no existing signature moves.
 *
 *   q           double [M][D], the queries; r double [N][D], the references; both dense
 *   q_group, r_group   int32 [M] / [N], both or neither: a pair is eligible only when q_group[j] == r_group[i]
 *   q_skip      int32 [M] or NULL: reference q_skip[j] is not eligible for query j (-1: none)
 *   r_radius2   double [N] or NULL; inside int32 [M], required exactly when r_radius2 is given
 *   nn_d2       double [M][k], nn_idx int32 [M][k]
 *
 * d2(j, i) = sum_d (q[j,d] - r[i,d])^2 in fp64, the direct form: lane l of one wavefront takes d = l, l + 64, ... in ascending order with
 * e = q - r, s = fma(e, e, s) from s = 0, and the 64 lane sums are added in the xor butterfly 32, 16, 8, 4, 2, 1; no division.  The bits of
 * d2(j, i) depend on the two rows and on D alone: not on j, i, M, N or the grid.  A pair is eligible when d2 is finite, i != q_skip[j] and
 * the groups are absent or equal.  nn_d2[j] / nn_idx[j] hold the k lexicographically lowest (d2, i) of the eligible pairs in ascending order,
 * +inf / -1 in the places that stay empty, so ties go to the lowest index whatever the order of arrival and a row with a NaN is never chosen.
 * inside[j] = the number of eligible i with r_radius2[i] finite and d2(j, i) <= r_radius2[i].
 * Two launches on `stream`, no atomics: per block of KPX_SET_BLOCK references and query one sorted k-list and one count go into `workspace`,
 * then one thread per query merges the blocks in ascending order (the counts are integer sums).  workspace:
 * kpx_set_neighbours_workspace_bytes(M, N, k) bytes (0 for sizes out of range), 8-byte aligned.  Capturable.
 * Limits: 1 <= M <= KPX_SET_MAX_QUERIES, 1 <= N <= KPX_SET_MAX_REFS, 1 <= D <= KPX_SET_MAX_DIM, 1 <= k <= KPX_SET_MAX_K; q, r, r_radius2,
 * workspace and nn_d2 8-byte aligned, the int32 arrays 4-byte.  Anything else is KPX_EINVAL before any device call. */
#define KPX_SET_MAX_K 8
#define KPX_SET_MAX_DIM 16384
#define KPX_SET_MAX_QUERIES 4096
#define KPX_SET_MAX_REFS (1 << 20)
#define KPX_SET_BLOCK 64
size_t kpx_set_neighbours_workspace_bytes(int M, int N, int k);
int kpx_set_neighbours_f64(const double* q /*[M,D]*/, int M, const double* r /*[N,D]*/, int N, int D, const int32_t* q_group /*[M] or NULL*/,
                           const int32_t* r_group /*[N] or NULL*/, const int32_t* q_skip /*[M] or NULL*/, const double* r_radius2 /*[N] or NULL*/,
                           int k, void* workspace, size_t workspace_bytes, double* nn_d2 /*[M,k]*/, int32_t* nn_idx /*[M,k]*/,
                           int32_t* inside /*[M] or NULL*/, void* stream);

/* ---- Motion-JPEG: baseline JPEG scans of 8-bit RGB frames (csrc/mjpeg.hip; evaluate.py --video, animate.py --video, kpx_amd/mjpeg.py), DESIGN.md
 * sections 2 and 4.4.  No reference counterpart.  Added without a version change, as the entries of csrc/prdc.hip were: no existing signature moves.
 *
 *   rgb         uint8 [N][H][W][3], dense, any alignment
 *   qtables     uint8 [2][64] ON THE HOST (read during the call): the luma and the chroma quantisation table in natural order, each in 1..255
 *   scans       N * kpx_jpeg_scan_bound(H, W) bytes on the device; offsets int64 [N + 1] on the device
 *
 * Frame n's scan -- the bytes between the SOS segment and EOI of a baseline JPEG whose headers kpx_amd.mjpeg.frame_prefix writes -- is
 * scans[offsets[n] .. offsets[n + 1]), the frames packed back to back, offsets[0] = 0.  Integers only (int32 / int64):
 *   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32768) >> 16,
 *   Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32768) >> 16 (arithmetic shifts), Cb and Cr clamped to [0, 255]; a chroma sample is
 *   (a + b + c + d + 2) >> 2 over its 2 x 2 clamped values; 128 is subtracted; F = T S T^t with T[u][x] = rint(8192 alpha(u) cos((2x + 1) u pi / 16))
 *   exactly; the coefficient is sgn(F) floor((|F| + Q 2^25) / (Q 2^26)).  One interleaved scan of 16 x 16 MCUs (four Y blocks in raster order,
 *   Cb, Cr) coded with the four typical Huffman tables of ITU T.81 Annex K.3 - K.6; a restart interval is one row of MCUs (DRI = W / 16),
 *   RSTm with m = row & 7 follows every row but the last, the DC predictors restart at 0, the last byte of an interval is padded with 1 bits,
 *   0x00 follows every 0xFF data byte, 16 zeros are ZRL, EOB is coded unless coefficient 63 is non-zero.
 * The bytes depend on the pixels and the tables alone, not on N, the grid or the order of execution.  Five launches on `stream`, no allocation,
 * copy or synchronisation and no atomics (capturable).  workspace: kpx_jpeg_workspace_bytes(N, H, W) bytes (0 for sizes out of range), 8-byte
 * aligned -- about 4.3 times the frames, and `scans` 3.25 times, so a caller with many frames encodes them in chunks (kpx_amd.ops.jpeg_encode).
 * Limits: 16 <= H, W <= 4096, both multiples of 16, N >= 1, N H W < 2^31.  KPX_EINVAL before any device call for anything else, a null pointer,
 * an offsets or workspace that is not 8-byte aligned, a workspace that is too small or a table entry of 0. */
size_t kpx_jpeg_scan_bound(int H, int W);                 /* bytes that always hold one frame's scan, markers included; 0 for sizes out of range */
size_t kpx_jpeg_workspace_bytes(int N, int H, int W);
int kpx_jpeg_encode_u8(const uint8_t* rgb /*[N,H,W,3]*/, int N, int H, int W, const uint8_t* qtables /*HOST [2,64]*/, uint8_t* scans,
                       int64_t* offsets /*[N+1]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---- The approximate posterior of the sequence VAE at inference (csrc/posterior.hip; evaluate.py --posterior, animate.py --interpolate and
 * --motion-from, kpx_amd/posterior.py), DESIGN.md sections 2 and 4.4.  No reference counterpart: the reference drops vae_encoder at inference.
 * Added without a version change, as the entries of csrc/prdc.hip and csrc/mjpeg.hip were: no existing signature moves.
 *
 * All three read logit = [mu | sigma] fp32 [B][2V], the output of networks.vae_encoder, exactly as kpx_vae_sample_kl_fwd_f32 reads it.
 * Limits of all three: 1 <= V <= KPX_LATENT_MAX_DIM, B >= 1, B*2V < 2^31; fp32 and int32 arrays 4-byte, fp64 and int64 arrays 8-byte aligned.
 * Anything else, or a null pointer that is not marked optional, is KPX_EINVAL before any device call.  One launch each on `stream`, no
 * allocation, copy, synchronisation or atomics (capturable).
 *
 * kpx_latent_stats_add_f64 ADDS the B posteriors to a running set.
 *   group     int32 [B] or NULL.  NULL: every row belongs to group 0 and G must be 1.
 *   state     double [G][V][KPX_LATENT_STATE_FIELDS], read and written.  Per (group g, dimension v), over the rows added so far:
 *               [0] sum mu   [1] sum mu^2   [2] sum sigma   [3] sum sigma^2   [4] sum kl   [5] #{mu == 0}   [6] #{sigma == 0}   [7] n
 *             kl = 0.5 * ((((m * m) + s * s) - log((double)1e-8f + s * s)) - 1.0) with m = (double)mu, s = (double)sigma, every operation in
 *             fp64 and rounded once in this order (no fma): the term of kpx_vae_sample_kl_fwd_f32 without its fp32 roundings.  The squares of
 *             fp32 values are exact in fp64.  -0 counts as 0.  The counters [5], [6], [7] are whole numbers held in doubles.
 *   counts    int64 [G][3], read and written.  [g][0] rows added to group g; [g][1] rows of group g left out because one of their 2V values
 *             is NaN or +-Inf; [0][2] -- GROUP 0's third field, whatever G is -- rows left out because group[b] lies outside [0, G) (such
 *             a row has no group of its own; its values are not looked at).  [g][2] for g > 0 is never written.
 *   kl_rows   double [B] or NULL: sum_v kl of row b -- each wavefront's 64 terms (v = 64 w + lane, zeros past V) in the xor butterfly 32, 16, 8,
 *             4, 2, 1, then the wavefronts' sums added in ascending w -- or NaN for a row that was left out.  A row's value depends on
 *             that row and V alone.
 *   A row that is left out changes nothing but its counter and its kl_rows entry.  Determinism is the contract: each column (g, v) is
 *   summed in ascending b starting from the value `state` held (one thread owns it for the whole call), so a set fed in pieces of any
 *   sizes leaves the bits that one call on the concatenation leaves.  G >= 1, G*V*8 < 2^31.
 *
 * kpx_latent_sample_f32: z[b][v] = fmaf(fl32(tau * sigma), eps, mu).  eps fp32 [B][V] or NULL.  With eps == NULL or tau == 0, z is mu bit
 *   for bit and neither sigma nor eps is read, so a NaN there does not reach z.  With tau == 1 it is the z of kpx_vae_sample_kl_fwd_f32
 *   bit for bit.  A NaN tau is KPX_EINVAL.
 *
 * kpx_latent_path_f32: S steps from za to zb, fp32 [B][V] each, out fp32 [S][B][V], 2 <= S <= KPX_LATENT_PATH_MAX_STEPS, S*B*V < 2^31.
 *   out[0] = za and out[S-1] = zb bit for bit.  Step 0 < s < S-1 stands at t = (double)s / (double)(S - 1) and is
 *   fl32(ca * (double)a + cb * (double)b), the two products and the sum in fp64, rounded once each (no fma), with
 *     KPX_LATENT_PATH_LERP    ca = 1 - t, cb = t
 *     KPX_LATENT_PATH_SLERP   per row: omega = acos(min(max(<a,b> / (sqrt(<a,a>) * sqrt(<b,b>)), -1), 1)), ca = sin((1 - t) * omega) / sin(omega),
 *                             cb = sin(t * omega) / sin(omega).  The three dot products are fp64 sums of exact products: lane l of one
 *                             wavefront adds v = l, l + 64, ... in ascending order from 0, then the 64 lane sums in the xor butterfly.
 *   A SLERP row falls back to LERP (its bits) when <a,a> or <b,b> is not > 0 or when sin(omega) >= KPX_LATENT_PATH_MIN_SIN does not hold:
 *   that is a = b, but also a = -b (omega = pi), whose path is then the straight line THROUGH 0, and any V = 1 row. */
#define KPX_LATENT_MAX_DIM 1024
#define KPX_LATENT_STATE_FIELDS 8
#define KPX_LATENT_PATH_MAX_STEPS 64
#define KPX_LATENT_PATH_MIN_SIN 1e-6
enum { KPX_LATENT_PATH_LERP = 0, KPX_LATENT_PATH_SLERP = 1 };
int kpx_latent_stats_add_f64(const float* logit /*[B,2V]*/, int B, int V, const int32_t* group /*[B] or NULL*/, int G,
                             double* state /*[G,V,8]*/, int64_t* counts /*[G,3]*/, double* kl_rows /*[B] or NULL*/, void* stream);
int kpx_latent_sample_f32(const float* logit /*[B,2V]*/, const float* eps /*[B,V] or NULL*/, float tau, float* z /*[B,V]*/, int B, int V,
                          void* stream);
int kpx_latent_path_f32(const float* za /*[B,V]*/, const float* zb /*[B,V]*/, int S, int mode, float* out /*[S,B,V]*/, int B, int V,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KPX_H */

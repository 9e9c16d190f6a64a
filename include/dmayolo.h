/* dmayolo.h — C ABI of the MI355X-native (gfx950) DMA-YOLO detection path.
 *
 * The reference (Yaling-Li/DMA-YOLO) is pure Python: its plugin boundary is the YAML module
 * namespace that models/yolo.py:377 resolves with eval(name), plus ComputeLoss
 * (utils/loss.py:135-218) and non_max_suppression (utils/general.py:633-725).  Every ATen kernel
 * those Python entry points reach is replaced by one entry point below; the Python host side
 * (dma-yolo_amd/dmayolo) binds them with ctypes.
 *
 * Conventions
 *   dtype      0 = float32 storage (parity mode), 1 = bfloat16 storage (throughput mode)
 *   layout     activations are NHWC; `*ps` is the pixel stride in elements (>= C), so a channel
 *              slice of a concatenation buffer is (base + c0, ps = Ctot)
 *   weights    fp32 master weights are OIHW (torch layout); conv kernels consume OHWI / IHWO copies
 *   stream     hipStream_t passed as void*; every call is stream-ordered and never synchronises
 *   return     0 on success, else the hipError_t of the launch.  *_partial_rows / *_blocks return sizes.
 */
#ifndef DMAYOLO_H
#define DMAYOLO_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- convolution: replaces nn.Conv2d in models/cspcm.py:15 (YAML Conv), models/common.py:67 (Conv),
 *      :1283-1304 (SCConv k2/k3/k4), :1172-1178 (CoorAttention conv1/conv_h/conv_w), models/yolo.py:63
 *      (Detect.m), and nn.Linear (common.py:105-108, 483-484) as a 1x1 conv over tokens. */
int dmy_conv_fwd_partial_rows(long M, int K);
/* BN partial rows dmy_conv_fwd writes for exactly these arguments (psum / psq must hold that many rows of K floats):
 * the per-tile count of dmy_conv_fwd_partial_rows, or one row per wave of the persistent halo kernel
 * (3x3 stride-1 64 -> 64-channel layers, csrc/conv.hip conv3_halo64) */
/* BN partial rows: an upper bound for any route of a training forward with these M / K (allocate this many rows of
 * psum / psq), and the rows the last training forward launched on this host thread actually wrote (pass that count
 * to dmy_colsum2 / dmy_bn_finalize).  Replaces the host-side prediction dmy_conv_fwd_bn_rows for allocation: the
 * count comes from the routing that launched.  BatchNorm2d.forward's batch statistics,
 * torch/nn/modules/batchnorm.py via models/common.py:72 */
long dmy_conv_fwd_bound_rows(long M, int K);
long dmy_conv_fwd_last_rows(void);
int dmy_conv_fwd_bn_rows(int dtype, const void* x, const void* w_ohwi, const float* bias, const void* y, int N,
                                int H, int W, int C, long xps, int K, int KH, int KW, int S, int P, int OH, int OW,
                                long yps);
int dmy_conv_fwd(int dtype, const void* x, const void* w_ohwi, const float* bias, void* y, float* psum, float* psq,
                 int N, int H, int W, int C, long xps, int K, int KH, int KW, int S, int P, int OH, int OW, long yps,
                 void* stream);
/* Inference form (eval BN / fused-model Conv), in one launch:
 * y = act(T(conv(x) + bias) * scale + shift) (+ res), the value dmy_conv_fwd + dmy_bn_act_fwd produce, in one
 * launch (models/common.py:69-77 forward / forward_fuse with BN in eval mode).  scale/shift may be NULL. */
int dmy_conv_fwd_act(int dtype, const void* x, const void* w_ohwi, const float* bias, void* y, int N, int H, int W,
                     int C, long xps, int K, int KH, int KW, int S, int P, int OH, int OW, long yps, const float* scale,
                     const float* shift, int act, const void* res, long rps, void* stream);
/* inference forward with a split-K workspace for small M (batch-1 detect, csrc conv_fwd_split + splitk_epi):
 * dmy_conv_fwd_act semantics; ws of dmy_conv_fwd_splitk_elems floats (0 = no split for these arguments). */
long dmy_conv_fwd_splitk_elems(int dtype, const void* x, const void* w_ohwi, const void* y, int N, int H, int W, int C,
                               long xps, int K, int KH, int KW, int S, int P, int OH, int OW, long yps);
int dmy_conv_fwd_act_ws(int dtype, const void* x, const void* w_ohwi, const float* bias, void* y, int N, int H, int W,
                        int C, long xps, int K, int KH, int KW, int S, int P, int OH, int OW, long yps, const float* scale,
                        const float* shift, int act, const void* res, long rps, float* ws, long ws_elems, void* stream);
int dmy_conv_dgrad(int dtype, const void* dy, const void* w_ihwo, void* dx, int accumulate, int N, int H, int W, int C,
                   long xps, int K, int KH, int KW, int S, int P, int OH, int OW, long yps, void* stream);
int dmy_conv_wgrad(int dtype, const void* x, const void* dy, float* dw_ohwi, int N, int H, int W, int C, long xps,
                   int K, int KH, int KW, int S, int P, int OH, int OW, long yps, void* stream);
/* bwd1x1.hip: fused backward of a train-mode 1x1 stride-1 Conv -> BatchNorm -> act (models/common.py:67-73, k = 1),
 * bf16: dz = dmy_bn_bwd_apply's value on (dy, z) in registers (never stored), then dx (+)= dz Wt and dw += dz^T x in
 * one persistent launch.  Replaces dmy_bn_bwd_apply + dmy_conv_dgrad + dmy_conv_wgrad_ex(OIHW) of such a layer; the
 * reduce / finalize that produce ca, cb, cc run before it as before.  x / dx / dy: [M][C] / [M][C] / [M][K] rows of
 * pixel stride xps / bps / dps; z dense [M][K]; wt = the IHWO copy [C][K]; dw fp32 [K][C], ACCUMULATED (the caller
 * zeroes it).  _ok: 1 when this shape / alignment is supported (else the call returns -1 and launches nothing).
 * ws (nullable): deterministic mode -- the per-block weight-grad partials go to ws (ws_elems >= _ws_elems) and are
 * summed in block order (run-to-run bit-identical dw), instead of fp32 atomics. */
int dmy_conv1x1_bwd_bn_ok(long M, int K, int C, long dps, long xps, long bps, const void* dy, const void* z,
                          const void* x, const void* dx);
int dmy_conv1x1_bwd_bn(const void* dy, long dps, const void* z, const void* x, long xps, const void* wt,
                       const float* scale, const float* shift, const float* mean, const float* invstd, int act,
                       const float* ca, const float* cb, const float* cc, void* dx, long bps, int accumulate,
                       float* dw, float* ws, long ws_elems, long M, int K, int C, void* stream);
long dmy_conv1x1_bwd_bn_ws_elems(long M, int K, int C);
/* flags: 1 = write dw in torch OIHW order (the parameter's .grad layout, no wgrad_to_oihw pass; needs Cp == C),
 *        2 = dw is already zero (a per-step gradient arena cleared once), skip the memset.  Same sums as above. */
int dmy_conv_wgrad_ex(int dtype, const void* x, const void* dy, float* dw, int N, int H, int W, int C, long xps, int K,
                      int KH, int KW, int S, int P, int OH, int OW, long yps, int flags, void* stream);
/* Deterministic weight-grad (same sums, run-to-run bit-identical): the split-K partials go to the fp32 workspace
 * ws (no atomics) and are reduced in split order.  dmy_conv_wgrad_ws_elems: workspace elements the same call needs
 * (0 = one split, ws may be NULL). */
long dmy_conv_wgrad_ws_elems(int dtype, const void* x, const void* dy, int N, int H, int W, int C, long xps, int K,
                             int KH, int KW, int S, int P, int OH, int OW, long yps, int flags);
int dmy_conv_wgrad_det(int dtype, const void* x, const void* dy, float* dw, int N, int H, int W, int C, long xps,
                       int K, int KH, int KW, int S, int P, int OH, int OW, long yps, int flags, float* ws,
                       long ws_elems, void* stream);
/* Route query: the kernel the dispatch takes for these arguments, from the plan the launch itself executes (csrc/conv.hip
 * plan_fwd / plan_dgrad / plan_wgrad).  Launches nothing and never dereferences a, b, c (only their 16-byte alignment
 * counts).  pass 0 = training forward without bias (a = x, b = w_ohwi, c = y), 1 = data-grad (a = dy, b = w_ihwo,
 * c = dx; acc = accumulate), 2 = weight-grad (a = x, b = dy, c unused).  Returns a DMY_KERN_* code, or -1 for an
 * unknown pass or a stride the data-grad does not support.  Several rules count blocks per CU, so the route of a
 * shape depends on the device's CU count. */
int dmy_conv_route(int pass, int dtype, const void* a, const void* b, const void* c, int N, int H, int W, int C,
                   long xps, int K, int KH, int KW, int S, int P, int OH, int OW, long yps, int acc);
enum {
  /* forward, and stride-1 data-grads (a forward over dy) */
  DMY_KERN_HALO = 0,     /* persistent 3x3 64 -> 64 halo kernel (conv3_halo64) */
  DMY_KERN_SPLITK = 1,   /* small-M split-K forward (conv_fwd_split + splitk_epi; dmy_conv_fwd_act_ws only) */
  DMY_KERN_P1S = 2,      /* 1x1 streaming GEMM (conv_p1s) */
  DMY_KERN_STEM = 3,     /* 16-channel 3x3 stem view on the streaming GEMM's gather */
  DMY_KERN_P1P = 4,      /* persistent 1x1 GEMM with the register epilogue (conv_p1p) */
  DMY_KERN_PIPE8 = 5,    /* 1x1 256 x 256 half-tile pipeline (conv_fwd_8p) */
  DMY_KERN_WIDE = 6,     /* 256 x 256 wide tile (conv_fwd_w) */
  DMY_KERN_WIDE288 = 7,  /* 288 x 256 wide tile */
  DMY_KERN_TALL = 8,     /* 512 x 128 tall tile */
  DMY_KERN_V3 = 9,       /* LDS-DMA 256 x 128 / 256 x 64 tiles (conv_fwd_v3) */
  DMY_KERN_V2 = 10,      /* register-staged tiles (forward: either size; data-grad: 64 x 64) */
  /* data-grad only */
  DMY_KERN_V2_BIG = 11,     /* register-staged 128 x 128 tile */
  DMY_KERN_S2_Q2S = 12,     /* stride 2 as one GEMM over dy pixels, 32 channels (conv_dgrad_q2s) */
  DMY_KERN_S2_Q2 = 13,      /* the same for 64 / 128 channels (conv_dgrad_q2) */
  DMY_KERN_S2_MERGED = 14,  /* stride 2, the four parity classes in one launch (conv_dgrad_s2_v3) */
  DMY_KERN_S2_CLASS = 15,   /* stride 2, one launch a class: 256 / 288 x 256 wide tile or 256 x 128 */
  /* weight-grad */
  DMY_KERN_W_TAP128 = 16,   /* tap-fused 3x3, 128-row tile (conv_wgrad_tap) */
  DMY_KERN_W_TAP64 = 17,    /* tap-fused, 64-row tile */
  DMY_KERN_W_TAP64X2 = 18,  /* tap-fused, 64-row tile over two halo planes */
  DMY_KERN_W_V4 = 19,       /* 256 x 128 tile (conv_wgrad_v4) */
  DMY_KERN_W_V3 = 20,       /* 128 x 128 tile (conv_wgrad_v3) */
  DMY_KERN_W_V3N128 = 21,   /* narrow tile, 32 / 64 rows x 128 columns (conv_wgrad_v3n) */
  DMY_KERN_W_V3N256 = 22,   /* narrow tile, 32 / 64 rows x 256 columns */
  DMY_KERN_W_V2_128 = 23,   /* register-staged 128 x 128 tile */
  DMY_KERN_W_V2_64 = 24     /* register-staged 64 x 64 tile */
};
/* Cp >= C: input channels zero-padded to a full 16-byte vector (the 3-channel stem, yaml:15) */
int dmy_conv_wprep(int dtype, const float* w_oihw, void* w_ohwi, void* w_ihwo, int K, int C, int Cp, int KH, int KW,
                   void* stream);
/* All conv weights of a model in one launch: descs is a DEVICE array of n records
 * { const float* w_oihw; void* w_ohwi; void* w_ihwo (nullable); int K, C, KH, KW; } (40 bytes, 8-byte aligned),
 * each as dmy_conv_wprep with Cp == C. */
int dmy_conv_wprep_multi(int dtype, const void* descs, int n, void* stream);
/* Stem as space-to-depth (yolov5*.yaml / DMA-YOLO yaml layer 0: Conv(3, c2, 6, 2, 2), models/common.py:50-77):
 * the k6 s2 p2 conv over x == a k3 s1 p1 conv over dmy_image_s2d(x) with these weights (Cs >= 4C channels). */
int dmy_conv_wprep_s2d(int dtype, const float* w_oihw, void* w_s2d, int K, int C, int Cs, void* stream);
int dmy_conv_wgrad_s2d_to_oihw(const float* dw_s2d, float* dw_oihw, int K, int C, int Cs, void* stream);
int dmy_conv_wgrad_to_oihw(const float* dw_ohwi, float* dw_oihw, int K, int C, int Cp, int KH, int KW, void* stream);

/* ---- depthwise convolution (csrc/dwconv.hip): replaces nn.Conv2d(c, c, k, s, k // 2, groups=c) in DWConv
 *      (models/common.py:79-82) and GhostConv.cv2 (:666-699).  One k x k filter per channel, no reduction over
 *      channels: streaming kernels over NHWC, fp32 accumulation, no atomics (run-to-run bit-identical).
 *      w is the filter tap-major, channel-minor [KH][KW][C] in the activation dtype: exactly the IHWO copy
 *      dmy_conv_wprep / dmy_conv_wprep_multi write for a (C, 1, k, k) OIHW weight (K = C, C = 1).
 *      Also nn.Conv2d(dim, dim, 7, padding=3, bias=True, groups=dim) of get_dwconv in GnConv (:1329, 1361-1362).
 *      dmy_dwconv_ok (models/common.py:79-82): 1 when the layer is supported -- groups == C == K, square k in
 *      {3, 5} with stride 1 or 2 or k in {7, 9} with stride 1, padding k / 2, OH / OW the conv's output size, C a whole number of 16-byte vectors
 *      (C % 8 bf16, C % 4 fp32), pixel strides >= C and whole vectors, 16-byte aligned bases.  Every other entry
 *      returns -1 and launches nothing when its arguments fail that test. */
int dmy_dwconv_ok(int dtype, const void* x, const void* w, const void* z, int N, int H, int W, int C, int K, int groups,
                  long xps, int KH, int KW, int S, int P, int OH, int OW, long zps);
/* models/common.py:79-82 in training: z = T(conv + bias) (bias nullable).  psum / psq (nullable together): per-block
 * partial sums and sums of squares of the values as stored, dmy_dwconv_fwd_rows(M = N * OH * OW, C) rows of C floats,
 * every row written; they feed dmy_colsum2 / dmy_bn_finalize like dmy_conv_fwd's. */
int dmy_dwconv_fwd_rows(long M, int C);
int dmy_dwconv_fwd(int dtype, const void* x, const void* w, const float* bias, void* z, float* psum, float* psq, int N,
                   int H, int W, int C, long xps, int KH, int KW, int S, int P, int OH, int OW, long zps, void* stream);
/* models/common.py:79-82 in inference (eval BN / fused DWConv), one launch with dmy_conv_fwd_act's semantics:
 * y = act(T(conv + bias) * scale + shift) (+ res); scale / shift nullable together. */
int dmy_dwconv_fwd_act(int dtype, const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int C,
                       long xps, int KH, int KW, int S, int P, int OH, int OW, long yps, const float* scale,
                       const float* shift, int act, const void* res, long rps, void* stream);
/* backward of models/common.py:79-82 w.r.t. its input, as a gather: each dx element sums the taps (i, j) whose
 * (h + P - i) and (w + P - j) are divisible by S.  accumulate as in dmy_conv_dgrad (dx += for GradSink targets). */
int dmy_dwconv_dgrad(int dtype, const void* dz, const void* w, void* dx, int accumulate, int N, int H, int W, int C,
                     long xps, int KH, int KW, int S, int P, int OH, int OW, long zps, void* stream);
/* backward of models/common.py:79-82 w.r.t. its weight: dmy_dwconv_wgrad writes dmy_dwconv_wgrad_rows(M, C) partial
 * rows [KH * KW * C] (tap-major), dmy_dwconv_wgrad_finalize sums them in row order into the (C, 1, KH, KW) OIHW fp32
 * gradient: dw = (accumulate ? dw : 0) + sum. */
int dmy_dwconv_wgrad_rows(long M, int C);
int dmy_dwconv_wgrad(int dtype, const void* x, const void* dz, float* part, int N, int H, int W, int C, long xps, int KH,
                     int KW, int S, int P, int OH, int OW, long zps, void* stream);
int dmy_dwconv_wgrad_finalize(const float* part, int rows, int C, int KH, int KW, float* dw, int accumulate,
                              void* stream);
/* backward of get_dwconv(dim, 7, True) (models/common.py:1361-1362) w.r.t. weight and bias in one launch, k = 7 only
 * (-1 otherwise): the same dmy_dwconv_wgrad_rows(M, C) partial rows, each [(KH * KW + 1) * C], whose last C floats are
 * the row's share of the bias gradient sum_pixels dz.  dmy_dwconv_wgrad_bias_finalize sums them in row order into dw
 * as above and into dbias = (bias_accumulate ? dbias : 0) + sum.  No atomics: both are run-to-run bit-identical. */
int dmy_dwconv_wgrad_bias(int dtype, const void* x, const void* dz, float* part, int N, int H, int W, int C, long xps,
                          int KH, int KW, int S, int P, int OH, int OW, long zps, void* stream);
int dmy_dwconv_wgrad_bias_finalize(const float* part, int rows, int C, int KH, int KW, float* dw, int accumulate,
                                   float* dbias, int bias_accumulate, void* stream);
/* nn.Conv2d(dim, dim, 9, groups=dim, padding='same') of ConvMix.Resnet (models/cspcm.py:29): dmy_dwconv_ok also admits
 * k = 9 with stride 1 and padding 4, and dmy_dwconv_fwd / _fwd_act / _dgrad / _wgrad / _wgrad_finalize take it (kernels
 * of their own, the filter loaded per column; dmy_dwconv_wgrad_bias stays k = 7 only).
 * dmy_dwconv_fwd_actbn is the one-launch inference form of x + BN(GELU(dw(x))) (models/cspcm.py:28-32, 39):
 * y = act(T(conv + bias)) * scale + shift (+ res); scale / shift nullable together.  k = 9 only, -1 otherwise. */
int dmy_dwconv_fwd_actbn(int dtype, const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int C,
                         long xps, int KH, int KW, int S, int P, int OH, int OW, long yps, const float* scale,
                         const float* shift, int act, const void* res, long rps, void* stream);

/* ---- activation before BatchNorm (csrc/convmix.hip): conv(+bias) -> GELU -> BatchNorm2d, both halves of ConvMix
 *      (models/cspcm.py:28-37).  a = act(z) is recomputed from the stored pre-activation z [M][C] (pixel stride zps)
 *      and never written.  16-byte vectors only: C a whole number of vectors, pixel strides >= C and whole vectors,
 *      16-byte aligned bases; otherwise -1 and nothing is launched.  Every partial array is
 *      [dmy_bn_partial_rows(M)][C], every row written, no atomics (run-to-run bit-identical).
 * dmy_actbn_stats (models/cspcm.py:30-31, 35-36, train): per-block sums of a and a * a, for dmy_bn_finalize. */
int dmy_actbn_stats(int dtype, const void* z, long zps, int act, long M, int C, float* psum, float* psq, void* stream);
/* models/cspcm.py:30-31 / 35-36 and the residual of :39: y = act(z) * scale + shift (+ res); y may be a channel
 * slice of a concat buffer (yps > C). */
int dmy_actbn_fwd(int dtype, const void* z, long zps, int act, const float* scale, const float* shift, const void* res,
                  long rps, void* y, long yps, long M, int C, void* stream);
/* backward of models/cspcm.py:30-31 / 35-36, first pass: per-block sums of dy and dy * ahat, ahat = (a - mean) * invstd,
 * for dmy_bn_bwd_finalize (-> dgamma, dbeta and the coefficients ca, cb, cc below). */
int dmy_actbn_bwd_reduce(int dtype, const void* z, long zps, const void* dy, long dps, const float* mean,
                         const float* invstd, int act, long M, int C, float* pdb, float* pdg, void* stream);
/* backward of models/cspcm.py:30-31 / 35-36, second pass: dz = act'(z) * (ca * dy + cb + cc * ahat) -- train-mode BN
 * with dmy_bn_bwd_finalize's coefficients, i.e. act'(z) * scale * (dy - mean(dy) - ahat * mean(dy * ahat)); eval mode:
 * ca = scale, cb = cc = 0.  pdz (nullable): per-block sums of dz for dmy_reduce_rows, the gradient of the conv bias
 * (models/cspcm.py:29, 34), which is not zero behind an activation. */
int dmy_actbn_bwd_apply(int dtype, const void* z, long zps, const void* dy, long dps, const float* mean,
                        const float* invstd, int act, const float* ca, const float* cb, const float* cc, void* dz,
                        long dzps, long M, int C, float* pdz, void* stream);

/* ---- adaptive-fusion necks (csrc/adapt.hip): AdaptConcat (models/common.py:953-992) and Adapt_Add2 / Adapt_Add3
 *      (models/common.py:1028-1061).  Streaming NHWC kernels, fp32 arithmetic, no atomics (run-to-run bit-identical).
 *      Every tensor has its own pixel stride.  Supported: bf16 with every channel count and stride a multiple of 8,
 *      fp32 a multiple of 4, 16-byte aligned bases; anything else returns -1 and launches nothing.
 *      Gate (models/common.py:979-990), L = 2 or 3 levels (x2 / C2 ignored for L = 2): wm [M][16 L] are the level maps
 *      the three add_conv blocks (:1063-1081) wrote side by side, W [L][16 L] / b [L] the weight_levels conv (:966) in
 *      fp32.  Per pixel: a = softmax(W wm + b) in fp32 with the maximum subtracted, y[:, off_l : off_l + C_l] =
 *      x_l * a_l rounded once to storage; a [M][L] fp32 is kept for the backward. */
int dmy_adapt_gate_blocks(int dtype, long M, int Ct, int L);
int dmy_adapt_gate_fwd(int dtype, int L, const void* x0, long x0ps, int C0, const void* x1, long x1ps, int C1,
                       const void* x2, long x2ps, int C2, const void* wm, long wmps, const float* W, const float* b,
                       void* y, long yps, float* a, long M, void* stream);
/* backward of models/common.py:979-990.  Per pixel da_l = sum_c dy_{l,c} x_{l,c}, dlogit = a * (da - sum a da);
 * dx_l = dy_l * a_l (bit l of accumulate: dx_l += for a GradSink target), dwm = W^T dlogit, and one partial row per
 * block, dmy_adapt_gate_blocks(dtype, M, Ct = sum C_l, L) rows, every row written: pdw [rows][L * 16 L] of
 * sum_m dlogit (x) wm and pdb [rows][L] of sum_m dlogit, for dmy_reduce_rows. */
int dmy_adapt_gate_bwd(int dtype, int L, const void* dy, long dps, const void* x0, long x0ps, int C0, const void* x1,
                       long x1ps, int C1, const void* x2, long x2ps, int C2, const float* a, const void* wm, long wmps,
                       const float* W, void* dx0, long dx0ps, void* dx1, long dx1ps, void* dx2, long dx2ps,
                       int accumulate, void* dwm, long dwmps, float* pdw, float* pdb, long M, void* stream);
/* models/common.py:1040-1044 (n = 2) and :1057-1061 (n = 3, after the shared 1x1 conv): y = silu(sum_i wn_i x_i) with
 * wn = w / (sum w + eps) computed on the device; the n inputs have C channels each (x2 ignored for n = 2). */
int dmy_adapt_add_fwd(int dtype, int n, const void* x0, long x0ps, const void* x1, long x1ps, const void* x2, long x2ps,
                      const float* w, float eps, void* y, long yps, long M, int C, void* stream);
/* backward of the above: s is recomputed from the inputs, dx_i = wn_i dy silu'(s) (bit i of accumulate: dx_i +=), and
 * part [n][dmy_dot_partial_blocks(M, C)] holds the per-block shares of sum dy silu'(s) x_i, which dmy_bifpn_wgrad
 * turns into dw (the normalisation is AdConcat's). */
int dmy_adapt_add_bwd(int dtype, int n, const void* dy, long dps, const void* x0, long x0ps, const void* x1, long x1ps,
                      const void* x2, long x2ps, const float* w, float eps, void* dx0, long dx0ps, void* dx1, long dx1ps,
                      void* dx2, long dx2ps, int accumulate, float* part, long M, int C, void* stream);

/* ---- fp8 (OCP e4m3fn) forward conv for config 5 (BASELINE configs[4], "fp8 MFMA conv"): replaces the forward of
 *      Conv.conv (models/common.py:61-74) when enabled; backward stays bf16.  Activations are quantised per
 *      tensor with the current amax (x ~ x8 * amax / 448), weights per output channel (w ~ w8 * wscale[k]);
 *      the MX-scaled 16x16x128 MFMA runs with unit block scales and the accumulator is dequantised in the
 *      epilogue.  Requirements: C % 128 == 0, K % 8 == 0, x8 dense [N*H*W][C]. */
long dmy_fp8_quant_ws_elems(void);  /* float workspace of dmy_fp8_quant; ws[0] = the amax used */
int dmy_fp8_quant(const void* x_bf16, long rows, int C, long xps, void* x8, float* ws, void* stream);
int dmy_conv_wprep_fp8(const float* w_oihw, void* w8_ohwi, float* wscale, int K, int C, int KH, int KW, void* stream);
int dmy_conv_fwd_fp8_partial_rows(long M, int K); /* BN partial rows of dmy_conv_fwd_fp8's epilogue */
int dmy_conv_fwd_fp8(const void* x8, const void* w8_ohwi, const float* xamax, const float* wscale, const float* bias,
                     void* y, float* psum, float* psq, int N, int H, int W, int C, int K, int KH, int KW, int S, int P,
                     int OH, int OW, long yps, const float* scale, const float* shift, int act, const void* res,
                     long rps, void* stream);

/* ---- BatchNorm2d + activation: replaces nn.BatchNorm2d/nn.SiLU/nn.Hardswish in models/common.py:68-73,
 *      1176-1180, 1284-1306 with utils/torch_utils.py:161-170 eps/momentum. act: 0 none 1 silu 2 hardswish
 *      3 sigmoid 4 gelu(erf). */
int dmy_bn_partial_rows(long M);
int dmy_bn_stats(int dtype, const void* z, long zps, long M, int C, float* psum, float* psq, void* stream);
int dmy_bn_finalize(const float* psum, const float* psq, int P, int C, double count, const float* gamma,
                    const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked,
                    float momentum, float eps, int update, float* mean, float* invstd, float* scale, float* shift,
                    void* stream);
int dmy_bn_eval_coef(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                     float eps, int C, float* scale, float* shift, void* stream);
int dmy_bn_act_fwd(int dtype, const void* z, long zps, const float* scale, const float* shift, int act,
                   const void* res, long rps, void* y, long yps, long M, int C, void* stream);
/* config-5 fp8 with delayed scaling: dmy_bn_act_fwd (bf16) that also writes the e4m3 copy y8 [M][C] (dense) of its
 * output for an e4m3 conv consumer (dmy_conv_fwd_fp8), quantised with the PREVIOUS step's amax -- the max over the
 * dmy_bn_act_f8_blocks() floats pmax that the previous call left in its nmax; used[0] receives that amax (the conv's
 * xamax) -- and leaves this step's block maxima in nmax (same size).  Replaces dmy_fp8_quant's two passes.
 * headroom (>= 1) multiplies that amax (Transformer-Engine-style margin against a growing range); nsat (nullable, same
 * size as nmax) receives per block the count of elements that saturated at +-448. */
int dmy_bn_act_f8_blocks(void);
int dmy_bn_act_fwd_f8(const void* z, long zps, const float* scale, const float* shift, int act, const void* res,
                      long rps, void* y, long yps, long M, int C, void* y8, const float* pmax, float* nmax, float* used,
                      float headroom, float* nsat, void* stream);
int dmy_bn_bwd_reduce(int dtype, const void* z, long zps, const void* dy, long dps, const float* scale,
                      const float* shift, const float* mean, const float* invstd, int act, long M, int C, float* pdb,
                      float* pdg, void* stream);
int dmy_bn_bwd_finalize(const float* pdb, const float* pdg, int P, int C, double count, const float* gamma,
                        const float* invstd, float* dgamma, float* dbeta, float* ca, float* cb, float* cc,
                        void* stream);
int dmy_bn_bwd_apply(int dtype, const void* z, long zps, const void* dy, long dps, const float* scale,
                     const float* shift, const float* mean, const float* invstd, int act, const float* ca,
                     const float* cb, const float* cc, void* dz, long dzps, long M, int C, void* stream);
int dmy_reduce_rows(const float* part, int P, int C, float* out, int accumulate, void* stream);
int dmy_bn_reduce_rows(int dtype, const void* z, long zps, const void* dy, long dps, long M, int C);
int dmy_colsum2_rows(long P);
int dmy_colsum2(const float* a, const float* b, long P, int C, float* oa, float* ob, void* stream);
/* SyncBatchNorm (torch.nn.SyncBatchNorm, train.py:272-275).  One layer's per-rank sums travel in a slab [R][2C + 1]
 * of doubles, R = world size: slot r = (sum a[C], sum b[C], n) of rank r, (sum x, sum x^2, pixels) in the forward and
 * (sum dy, sum dy * xhat, pixels) in the backward.  Every rank packs its own slot and zeros the others, the caller
 * all-reduces (SUM) the slab -- adding zeros is exact, so the result is an all-gather whatever the collective's order --
 * and finalizes.  No atomics: bit-identical on every rank and from run to run.  A bad slab / R / rank / C returns
 * hipErrorInvalidValue and launches nothing.
 * dmy_bn_sync_pack: column sums of P partial rows of pa / pb [P][C] in double, in dmy_bn_finalize's order, and `count`
 * into slot `rank`; zeros in every other slot, same launch. */
int dmy_bn_sync_pack(const float* pa, const float* pb, int P, int C, double count, double* slab, int R, int rank,
                     void* stream);
/* What dmy_bn_finalize writes (running statistics with the unbiased variance, num_batches_tracked += 1 when `update`),
 * from the R slots added in rank order; the global count is read from the slab on the device.  R = 1 equals
 * dmy_bn_finalize over the same rows bit for bit. */
int dmy_bn_sync_finalize(const double* slab, int R, int C, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, long long* num_batches_tracked, float momentum, float eps, int update,
                         float* mean, float* invstd, float* scale, float* shift, void* stream);
/* dmy_bn_bwd_finalize over the slab: dgamma / dbeta (nullable) from slot `rank` alone -- parameter gradients stay local
 * and the DDP reducer averages them, torch's SyncBatchNorm rule -- ca / cb / cc from all slots in rank order over the
 * global count. */
int dmy_bn_sync_bwd_finalize(const double* slab, int R, int rank, int C, const float* gamma, const float* invstd,
                             float* dgamma, float* dbeta, float* ca, float* cb, float* cc, void* stream);

/* ---- SPD-mix downsamplers (csrc/spd.hip): DMConv / DMMConv / DMMConv2 with SM and MP (models/common.py:1460-1475,
 *      1508-1547).  Streaming NHWC kernels, fp32 arithmetic, no atomics.  Supported: bf16 with every channel count and
 *      pixel stride a multiple of 8, fp32 a multiple of 4, at most 256 vectors per row, 16-byte aligned bases; anything
 *      else returns hipErrorInvalidValue and launches nothing.
 *      SM layout (models/common.py:1467): the full-resolution pixel (n, h, w) with K channels is the K-channel block
 *      q = (h & 1) + 2 * (w & 1) of the half-resolution pixel (n, h / 2, w / 2); H and W even. */
/* Conv.bn + Conv.act + SM of DMConv / DMMConv.cv2 (models/common.py:1533-1534, 1544-1545): y_sm = act(z * scale +
 * shift), z [N][H][W][K] with pixel stride zps, y_sm [N][H/2][W/2][4K] with pixel stride yps >= 4K.  dmy_bn_act_fwd's
 * per-element math (no residual, no fp8 emit) stored through the SM mapping. */
int dmy_bn_act_s2d_fwd(int dtype, const void* z, long zps, const float* scale, const float* shift, int act, void* y,
                       long yps, int N, int H, int W, int K, void* stream);
/* the backward of the same lines: dmy_bn_bwd_reduce / dmy_bn_bwd_apply with dy [N][H/2][W/2][4K] (pixel stride dps)
 * read through the SM mapping and z / dz in plain row order.  The reduce writes dmy_bn_bwd_reduce_s2d_rows(dtype, M =
 * N * H * W, K) partial rows of K floats to pdb and pdg, every row written, rows visited in a fixed order; they feed
 * dmy_colsum2 / dmy_bn_bwd_finalize like dmy_bn_bwd_reduce's. */
int dmy_bn_bwd_reduce_s2d_rows(int dtype, long M, int K);
int dmy_bn_bwd_reduce_s2d(int dtype, const void* z, long zps, const void* dy, long dps, const float* scale,
                          const float* shift, const float* mean, const float* invstd, int act, int N, int H, int W,
                          int K, float* pdb, float* pdg, void* stream);
int dmy_bn_bwd_apply_s2d(int dtype, const void* z, long zps, const void* dy, long dps, const float* scale,
                         const float* shift, const float* mean, const float* invstd, int act, const float* ca,
                         const float* cb, const float* cc, void* dz, long dzps, int N, int H, int W, int K,
                         void* stream);
/* nn.MaxPool2d(2, 2) of MP (models/common.py:1469-1475): y [N][H/2][W/2][C] (floor), argmax [N * (H/2) * (W/2)][C]
 * the window offset dh * 2 + dw of the maximum under ATen's rule (first maximum in (row, column) scan order, a NaN
 * wins).  The backward is a gather over dx [N][H][W][C]: every input pixel belongs to at most one window; accumulate
 * as in dmy_maxpool_bwd (dx += for GradSink targets). */
int dmy_maxpool2_fwd(int dtype, const void* x, long xps, void* y, long yps, unsigned char* argmax, int N, int H, int W,
                     int C, void* stream);
int dmy_maxpool2_bwd(int dtype, const void* dy, long dps, const unsigned char* argmax, void* dx, long dxps,
                     int accumulate, int N, int H, int W, int C, void* stream);
/* DMMConv2's front end (models/common.py:1516, 1519): x is read once; sm [N][H/2][W/2][4C] (pixel stride smps) takes
 * SM(x), mp [N][H/2][W/2][C] and argmax take MP(x) as dmy_maxpool2_fwd writes them.  The backward writes dx =
 * SM^-1(dsm) + the pool's gather of dmp, summed in fp32 and rounded once, one write per element.  H and W even. */
int dmy_spd_split_fwd(int dtype, const void* x, long xps, void* sm, long smps, void* mp, long mpps,
                      unsigned char* argmax, int N, int H, int W, int C, void* stream);
int dmy_spd_split_bwd(int dtype, const void* dsm, long dsmps, const void* dmp, long dmpps, const unsigned char* argmax,
                      void* dx, long dxps, int N, int H, int W, int C, void* stream);

/* ---- GnConv / HorBlock (csrc/hor.hip): the recursive gate product and the layer-scaled residual
 *      (models/common.py:1343-1359, 1382-1400).  Streaming NHWC kernels over M pixels of C channels, fp32 arithmetic,
 *      one rounding per stored element, no atomics.  Supported: C and every pixel stride a whole number of 16-byte
 *      vectors (8 channels bf16, 4 fp32), pixel strides >= C, 16-byte aligned bases, so an operand may be a channel
 *      slice of a wider buffer at a vector offset; anything else returns hipErrorInvalidValue and launches nothing. */
/* models/common.py:1349-1355: `pwa * dw_list[0]` and `self.pws[i](x) * dw_list[i + 1]` with the `* self.scale` of
 * dw_abc folded in: y = a * b * scale.  a, b, y each with their own pixel stride. */
int dmy_gate_fwd(int dtype, const void* a, long aps, const void* b, long bps, void* y, long yps, long M, int C,
                 float scale, void* stream);
/* the backward of the same lines in one launch: da = dy * b * scale, db = dy * a * scale, each written (not
 * accumulated) through its own pixel stride (torch.split's backward :1347, :1351 is the slice addressing). */
int dmy_gate_bwd(int dtype, const void* dy, long dps, const void* a, long aps, const void* b, long bps, void* da,
                 long daps, void* db, long dbps, long M, int C, float scale, void* stream);
/* models/common.py:1388 and :1395-1398 without DropPath: out = x + gamma[c] * y.  x and out strided, y dense [M][C],
 * gamma fp32 [C]. */
int dmy_layerscale_fwd(int dtype, const void* x, long xps, const void* y, const float* gamma, void* out, long ops,
                       long M, int C, void* stream);
/* its backward in one launch: dy = gamma[c] * dout (dense [M][C]) and one partial row per block of sum_m dout * y,
 * part [dmy_layerscale_bwd_rows(M)][C], every row written, for dmy_reduce_rows (-> dgamma, rows summed in row order:
 * bit-identical run to run).  dx is dout itself.  At most 256 vectors per row. */
int dmy_layerscale_bwd_rows(long M);
int dmy_layerscale_bwd(int dtype, const void* dout, long dps, const void* y, const float* gamma, void* dy, long M,
                       int C, float* part, void* stream);

/* ---- memory-bound NHWC ops */
/* nn.MaxPool2d(k, 1, k//2): SPPF common.py:250-258, SPPFCSPC :1266-1274 */
int dmy_maxpool_fwd(int dtype, const void* x, long xps, void* y, long yps, unsigned char* argmax, int N, int H, int W,
                    int C, int k, void* stream);
int dmy_maxpool_bwd(int dtype, const void* dy, long dps, const unsigned char* argmax, void* dx, long dxps,
                    int accumulate, int N, int H, int W, int C, int k, void* stream);
/* inference SPPF / SPPFCSPC pyramid (common.py:250-258, :1266-1274 under no_grad): y1 = pool(x), y2 = pool(y1),
   y3 = pool(y2) in one launch, bit-identical to three dmy_maxpool_fwd calls; k 3 or 5, 16-B vectors, no argmax */
int dmy_maxpool_chain3_fwd(int dtype, const void* x, long xps, void* y1, void* y2, void* y3, long yps, int N, int H,
                           int W, int C, int k, void* stream);
/* nn.AvgPool2d(r, r): SCConv.k2[0] common.py:1282 */
int dmy_avgpool_fwd(int dtype, const void* x, long xps, void* y, int N, int H, int W, int C, int r, void* stream);
int dmy_avgpool_bwd(int dtype, const void* dy, void* dx, long dxps, int accumulate, int N, int H, int W, int C, int r,
                    void* stream);
/* nearest resize: nn.Upsample (yaml head), F.interpolate in SCConv common.py:1311 */
int dmy_resize_fwd(int dtype, const void* x, long xps, void* y, long yps, float yscale, int N, int IH, int IW, int OH,
                   int OW, int C, void* stream);
int dmy_resize_bwd(int dtype, const void* dy, long dps, void* dx, long dxps, int N, int IH, int IW, int OH, int OW,
                   int C, void* stream);
/* torch.cat / AdConcat2/3 fast-normalised weights: common.py:656-664, 994-1026 */
int dmy_slice_copy(int dtype, const void* src, long sps, void* dst, long dps, long M, int C, const float* w, int idx,
                   int nw, float eps, int accumulate, void* stream);
int dmy_dot_partial_blocks(long M, int C);
int dmy_dot_partial(int dtype, const void* a, long aps, const void* b, long bps, long M, int C, float* part,
                    void* stream);
/* BiFPN weighted-concat backward of one input in one pass: dmy_slice_copy(dy -> g, scale, accumulate) and
   dmy_dot_partial(dy, x -> part) reading dy once (16-B vectors; else hipErrorInvalidValue) */
int dmy_slice_copy_dot(int dtype, const void* dy, long dps, void* g, long gps, const void* x, long xps, long M, int C,
                       const float* wv, int idx, int nw, float eps, int accumulate, float* part, void* stream);
int dmy_bifpn_wgrad(const float* part, int nblk, int nw, const float* w, float eps, float* dw, void* stream);
/* SCConv gate k3(x) * sigmoid(x + up(k2(x))): common.py:1311-1314 */
int dmy_scgate_fwd(int dtype, const void* x, long xps, const void* u3, const void* g, void* out, int N, int H, int W,
                   int C, int GH, int GW, void* stream);
int dmy_scgate_bwd(int dtype, const void* x, long xps, const void* u3, const void* g, const void* dout, void* du3,
                   void* dpre, long dpps, int accumulate, int N, int H, int W, int C, int GH, int GW, void* stream);
/* the same gate with k3's BatchNorm (common.py:1296-1300) folded in (bf16): the forward reads k3's pre-BN conv output z
   and applies scale / shift; the backward also writes k3's BN backward-reduce partials, one row per block
   (dmy_scgate_bn_rows rows of C floats each) */
int dmy_scgate_bn_rows(int N, int H, int W, int C);
int dmy_scgate_bn_fwd(const void* x, long xps, const void* z, const float* scale, const float* shift, const void* g,
                      void* out, int N, int H, int W, int C, int GH, int GW, void* stream);
int dmy_scgate_bn_bwd(const void* x, long xps, const void* z, const float* scale, const float* shift,
                      const float* mean, const float* invstd, const void* g, const void* dout, void* du3, void* dpre,
                      int N, int H, int W, int C, int GH, int GW, float* pdb, float* pdg, void* stream);
/* CoorAttention pooling + re-weighting: common.py:1183-1207 */
int dmy_ca_pool_fwd(int dtype, const void* x, long xps, void* y, int N, int H, int W, int C, void* stream);
int dmy_ca_pool_bwd(int dtype, const void* dy, void* dx, long dxps, int accumulate, int N, int H, int W, int C,
                    void* stream);
int dmy_ca_apply_fwd(int dtype, const void* x, long xps, const void* lh, const void* lw, void* out, long ops, int N,
                     int H, int W, int C, void* stream);
int dmy_ca_apply_bwd(int dtype, const void* x, long xps, const void* lh, const void* lw, const void* dout, long dps,
                     void* dx, long dxps, void* dlh, void* dlw, int N, int H, int W, int C, void* stream);
/* input normalisation imgs.float()/255 (train.py:402) + layout changes */
/* NCHW image (uint8 / fp32, even H, W) -> space-to-depth NHWC [N][H/2][W/2][Cs], channel (dy*2+dx)*C+c,
 * times scale (train.py:402 `/255`); the stem conv's input in its k3 s1 form */
int dmy_image_s2d(int dtype, int src_kind, const void* x, void* y, int N, int C, int H, int W, int Cs, float scale,
                  void* stream);
/* NCHW image -> NHWC [N][H][W][Cp] times scale, channels [C, Cp) zero; Cp a whole number of 16-byte vectors of the
 * storage type (8 bf16 / 4 fp32), Cp >= C and y 16-byte aligned, hipErrorInvalidValue otherwise */
int dmy_nchw_to_nhwc(int dtype, int src_kind, const void* x, void* y, int N, int C, int H, int W, int Cp, float scale,
                     void* stream);
/* one test-time-augmentation input (models/yolo.py:199-201 with utils/torch_utils.py:264-274 scale_img): the NCHW
 * image (src_kind / scale as dmy_image_s2d) flipped (0 none, 2 up-down, 3 left-right), resized to OH x OW
 * (F.interpolate bilinear, align_corners=False), padded right / bottom with pad_value to OHp x OWp, in the stem's
 * layout: s2d = 1 [N][OHp/2][OWp/2][Cs] as dmy_image_s2d (OHp, OWp even), s2d = 0 [N][OHp][OWp][Cs] as
 * dmy_nchw_to_nhwc; channels past the image's are zero */
int dmy_tta_image(int dtype, int src_kind, const void* x, void* y, int N, int C, int H, int W, int s2d, int Cs,
                  float scale, int flip, int OH, int OW, int OHp, int OWp, float pad_value, void* stream);
int dmy_nhwc_to_nchw_f32(int dtype, const void* x, long xps, float* y, int N, int C, int H, int W, void* stream);
int dmy_pointwise(int dtype, int op, int act, const void* a, const void* b, void* y, long n, float alpha,
                  void* stream);
int dmy_cast(int src_kind, int dst_kind, const void* x, void* y, long n, float scale, void* stream);

/* ---- Detect decode (models/yolo.py:78-101) and ComputeLoss (utils/loss.py:167-276, metrics.py:192-235) */
int dmy_detect_decode(int dtype, const void* y, long sb, long sh, long sw, int N, int H, int W, int na, int no,
                      float stride, const float* anchors, float* z, long zoff, long ztotal, void* stream);
/* every level of one Detect forward in one launch (yolo.py:63-76 under eval): level l's NHWC head output ys[l] with
   element strides strides[3l .. 3l+2] = (batch, row, col), hw[2l], hw[2l+1] = its H, W, lvl_stride[l] its stride,
   anchors [nl][na][2] (device); z rows of level l start at the sum of the earlier levels' na*H*W.  The bits of one
   dmy_detect_decode per level */
int dmy_detect_decode_levels(int dtype, int nl, const void* const* ys, const long* strides, const int* hw,
                             const float* lvl_stride, int N, int na, int no, const float* anchors, float* z, long ztotal,
                             void* stream);
/* one test-time-augmentation pass written into its slice of the combined [N][ztotal][no] buffer
   (models/yolo.py:194-275: _forward_augment, _descale_pred, _clip_augmented): dmy_detect_decode_levels' arguments and
   arithmetic, then xywh / scale (IEEE division) and x = img_w - x (flip 3) or y = img_h - y (flip 2).  Levels whose
   level_mask bit is clear are neither read nor written; a kept level's rows start at zoff plus the kept earlier
   levels' na*H*W */
int dmy_detect_decode_tta(int dtype, int nl, const void* const* ys, const long* strides, const int* hw,
                          const float* lvl_stride, int N, int na, int no, const float* anchors, float* z, long ztotal,
                          float scale, int flip, float img_h, float img_w, int level_mask, long zoff, void* stream);
int dmy_build_targets(const float* targets, int nt, const float* anchors, int na, int H, int W, float anchor_t,
                      int* b, int* a, int* gj, int* gi, int* tcls, float* tbox, float* anch, int* count,
                      void* stream);
/* per level: part = dmy_yolo_loss_part_rows() fp32 block partials (caller-zeroed), G / tobj caller-zeroed;
 * workspaces tgrad [cap][4 + nc] fp32 and links [N*na*H*W + cap] int32 (no float atomics: deterministic) */
int dmy_yolo_loss_part_rows(void);
int dmy_yolo_loss_level(int dtype, const void* p, long sb, long sa, long sh, long sw, int N, int na, int H, int W,
                        int no, int nc, float box_gain, float obj_gain, float cls_gain, float cls_pw, float obj_pw,
                        float cp, float cn, float balance, float bs, const int* b, const int* a, const int* gj,
                        const int* gi, const int* tcls, const float* tbox, const float* anch, const int* count,
                        int cap, float* grad, float* tobj, float* part, float* tgrad, int* links, void* stream);
int dmy_yolo_loss_finalize(const float* part, int nl, float box, float obj, float cls, float bs, float* loss,
                           float* items, void* stream);
/* Focal loss and autobalance.  dmy_yolo_loss_level_focal is dmy_yolo_loss_level with the FocalLoss wrapper of
 * utils/loss.py:35-62 around both BCE terms (alpha 0.25, mean; fl_gamma 0 = plain BCE; 1, 1.5 and 2 by multiplies /
 * sqrtf, any other gamma by powf) and with the level's objectness balance read from balance[level] (device, double)
 * instead of passed by value.  Its objectness partials are left unbalanced and belong to
 * dmy_yolo_loss_finalize_balance, which applies balance[] as it stood before the call and then, when autobalance
 * is set, updates it in place as utils/loss.py:207-212 does (balance[i] = balance[i] * 0.9999 + 0.0001 / obji, all
 * divided by balance[ssi]; a level whose obji is 0 or not finite keeps its value).  nl <= 8; no host read. */
int dmy_yolo_loss_level_focal(int dtype, const void* p, long sb, long sa, long sh, long sw, int N, int na, int H, int W,
                              int no, int nc, float box_gain, float obj_gain, float cls_gain, float cls_pw,
                              float obj_pw, float cp, float cn, const double* balance, int level, float fl_gamma,
                              float bs, const int* b, const int* a, const int* gj, const int* gi, const int* tcls,
                              const float* tbox, const float* anch, const int* count, int cap, float* grad,
                              float* tobj, float* part, float* tgrad, int* links, void* stream);
int dmy_yolo_loss_finalize_balance(const float* part, int nl, float box, float obj, float cls, float bs,
                                   double* balance, int autobalance, int ssi, float* loss, float* items,
                                   void* stream);
int dmy_loss_grad(int dtype, const float* grad, const float* upstream, void* dp, long n, void* stream);
/* SIoU (utils/metrics.py:192-235, bbox_iou(..., x1y1x2y2=False, SIoU=True)) of n xywh pairs through the
 * loss kernel's device function: iou [n] and d iou / d b1 [n][4] (forward-mode duals). */
int dmy_siou_eval(const float* b1, const float* b2, float* iou, float* grad_b1, int n, void* stream);
/* The box criterion of the loss: the keyword of the reference's bbox_iou call at utils/loss.py:185
 * (utils/metrics.py:192-252).  Append only, never renumber. */
#define DMY_IOU_SIOU 0  /* SIoU=True, metrics.py:219-235: what the reference's ComputeLoss passes */
#define DMY_IOU_CIOU 1  /* CIoU=True, metrics.py:238-247: alpha = v / (v - iou + (1 + eps)) is a constant (no_grad) */
#define DMY_IOU_DIOU 2  /* DIoU=True, metrics.py:238-242: iou - rho2 / c2 */
#define DMY_IOU_GIOU 3  /* GIoU=True, metrics.py:248-250: iou - (c_area - union) / c_area */
#define DMY_IOU_PLAIN 4 /* no keyword, metrics.py:215, 252: inter / union */
/* dmy_yolo_loss_level / dmy_yolo_loss_level_focal (utils/loss.py:167-218) with the box term's criterion chosen by
 * iou_kind, the last argument; every other argument, buffer and workspace as there.  DMY_IOU_SIOU runs the very
 * kernels of those entries; the other kinds are further instances of the same target kernel, so tobj =
 * max(clamp(iou, 0)), the per-cell ordered gradient sums and the block partials are unchanged (no float atomics, no
 * host read).  An unknown iou_kind returns hipErrorInvalidValue and launches nothing. */
int dmy_yolo_loss_level_iou(int dtype, const void* p, long sb, long sa, long sh, long sw, int N, int na, int H, int W,
                            int no, int nc, float box_gain, float obj_gain, float cls_gain, float cls_pw, float obj_pw,
                            float cp, float cn, float balance, float bs, const int* b, const int* a, const int* gj,
                            const int* gi, const int* tcls, const float* tbox, const float* anch, const int* count,
                            int cap, float* grad, float* tobj, float* part, float* tgrad, int* links, void* stream,
                            int iou_kind);
int dmy_yolo_loss_level_focal_iou(int dtype, const void* p, long sb, long sa, long sh, long sw, int N, int na, int H,
                                  int W, int no, int nc, float box_gain, float obj_gain, float cls_gain, float cls_pw,
                                  float obj_pw, float cp, float cn, const double* balance, int level, float fl_gamma,
                                  float bs, const int* b, const int* a, const int* gj, const int* gi, const int* tcls,
                                  const float* tbox, const float* anch, const int* count, int cap, float* grad,
                                  float* tobj, float* part, float* tgrad, int* links, void* stream, int iou_kind);
/* bbox_iou (utils/metrics.py:192-252, eps = 1e-7) of n box pairs through the loss kernel's device functions:
 * iou [n] and d iou / d b1 [n][4] by forward-mode duals, box 2 constant.  xyxy = 0: both boxes are (x, y, w, h)
 * (x1y1x2y2=False, metrics.py:200-204) and the gradient is with respect to those; xyxy != 0: (x1, y1, x2, y2) used as
 * given (metrics.py:197-199), gradient with respect to the corners.  torch.min / torch.max ties split the gradient,
 * clamp(0) passes it at 0.  n <= 0 launches nothing; an unknown iou_kind returns hipErrorInvalidValue. */
int dmy_bbox_iou_eval(int iou_kind, int xyxy, const float* b1, const float* b2, float* iou, float* grad_b1, int n,
                      void* stream);

/* ---- non_max_suppression (utils/general.py:633-725 -> torchvision.ops.nms at :708) */
int dmy_nms_candidates(const float* pred, int nimg, int A, int no, float conf, int multi_label,
                       const unsigned char* class_ok, unsigned long long* keys, long cap, int* counts, void* stream);
int dmy_nms_sort(unsigned long long* keys, long cap, const int* counts, int nimg, void* stream);
/* ncand (nullable): the greedy launch also writes each image's candidate count there and re-zeroes counts[b], so a
   persistent counts buffer is zero for the next dmy_nms_candidates without a fill launch */
int dmy_nms_greedy(const float* pred, int nimg, int A, int no, float iou, int agnostic, int max_det, int max_nms,
                   const unsigned long long* keys, long cap, int* counts, float* boxes, float* out, int* nkeep,
                   int* ncand, void* stream);
/* the same greedy keep set / order through an IoU bitmask (cap <= dmy_nms_mask_rows(); mask: nimg * cap * cap / 64 words;
   boxes is not used: the mask kernel makes each box from its key) */
int dmy_nms_mask_rows(void);
int dmy_nms_greedy_mask(const float* pred, int nimg, int A, int no, float iou, int agnostic, int max_det, int max_nms,
                        const unsigned long long* keys, long cap, int* counts, float* boxes,
                        unsigned long long* mask, float* out, int* nkeep, int* ncand, void* stream);
/* ---- the modes of non_max_suppression beyond its default call; the entries above run that one, unchanged.
 * Apriori label rows (utils/general.py:663-670, the autolabel / --save-hybrid input of val.py:228-231): labels
 * [sum n_i, 5] = (cls, x, y, w, h) in pixels, packed image after image, label_off [nimg + 1] their offsets.  Label k of
 * an image is row A + k of that image in every key: box = the label's xywh, obj = 1, one-hot class (score 1.0 * 1.0),
 * after the prediction rows in the index order.  A label whose class is outside [0, nc) is dropped.  The later
 * entries of a call read such rows from the same table (nullable there, both pointers or neither). */
int dmy_nms_candidates_labels(const float* pred, const float* labels, const int* label_off, int nimg, int A, int no,
                              float conf, int multi_label, const unsigned char* class_ok, unsigned long long* keys,
                              long cap, int* counts, void* stream);
/* Criterion NMS (NMS() of utils/general.py:727-761 over bbox_iou, utils/general.py:764-824): dmy_nms_greedy /
 * dmy_nms_greedy_mask with the suppression test chosen by iou_kind, a DMY_IOU_* code.  DMY_IOU_PLAIN is the default
 * path's torchvision test (IoU > thr); DMY_IOU_GIOU / _DIOU / _CIOU evaluate bbox_iou(box1 = the kept, earlier
 * candidate, box2 = the later one, x1y1x2y2=True, ...) in fp32 with one rounding per operation and suppress iff
 * !(value <= thr), so a NaN suppresses.  DMY_IOU_SIOU (which NMS() never reaches) and unknown codes return
 * hipErrorInvalidValue.  The mask form takes no boxes scratch. */
int dmy_nms_greedy_kind(int iou_kind, const float* pred, const float* labels, const int* label_off, int nimg, int A,
                        int no, float iou, int agnostic, int max_det, int max_nms, const unsigned long long* keys,
                        long cap, int* counts, float* boxes, float* out, int* nkeep, int* ncand, void* stream);
int dmy_nms_greedy_mask_kind(int iou_kind, const float* pred, const float* labels, const int* label_off, int nimg,
                             int A, int no, float iou, int agnostic, int max_det, int max_nms,
                             const unsigned long long* keys, long cap, int* counts, unsigned long long* mask,
                             float* out, int* nkeep, int* ncand, void* stream);
/* Merge-NMS (utils/general.py:712-718), after a greedy launch that was given ncand = NULL (counts still holds the
 * candidate counts) and wrote its keep counts to nk, a device vector.  For an image with 1 < n < 3000 candidates every
 * kept row becomes sum_j w[j] xyxy[j] / sum_j w[j] over all n candidates, w[j] = (box_iou(offset box i, offset box j)
 * > iou) * score[j] (utils/metrics.py:254-276), the sums in fp64, one division and rounding to fp32; with redundant,
 * rows with no more than one hit are dropped and the rest move up.  Other images keep their rows.  merged [nimg,
 * max_det, 6] and hits [nimg, max_det] are scratch.  nkeep gets the final keep counts; ncand as in dmy_nms_greedy. */
int dmy_nms_merge(const float* pred, const float* labels, const int* label_off, int nimg, int A, int no, float iou,
                  int agnostic, int max_det, int redundant, const unsigned long long* keys, long cap, int* counts,
                  const int* nk, float* merged, int* hits, float* out, int* nkeep, int* ncand, void* stream);

/* ---- Swin / C3STR (models/common.py:452-654): LayerNorm, shifted-window attention core with the
 *      reference's mask semantics, per-sample DropPath scale (common.py:386-403) */
int dmy_layernorm_fwd(int dtype, const void* x, long xps, const float* w, const float* b, void* y, float* mean,
                      float* rstd, long M, int C, float eps, void* stream);
int dmy_layernorm_bwd_blocks(long M);
int dmy_layernorm_bwd(int dtype, const void* x, long xps, const void* dy, long dps, const float* w, const float* mean,
                      const float* rstd, void* dx, long dxps, int accumulate, long M, int C, float* pdw, float* pdb,
                      void* stream);
int dmy_winattn_fwd(int dtype, const void* qkv, const float* table, void* out, int B, int H, int W, int C, int nh,
                    int shift, float scale, void* stream);
int dmy_winattn_bwd_groups(int B, int H, int W, int nh);
int dmy_winattn_bwd(int dtype, const void* qkv, const void* dout, const float* table, void* dqkv, float* dtab_part,
                    float* dtab, int B, int H, int W, int C, int nh, int shift, float scale, void* stream);
int dmy_sample_scale(int dtype, const void* x, const float* scale, void* y, long per, long n, void* stream);
/* DropPath fused with the residual add of an active SwinTransformerLayer drop_path (common.py:386-403, 621-627): y = x +
 * f * s[b], s[b] = floor(keep + u[b]) / keep on torch's drawn uniforms u [N] (samples = contiguous blocks of `per`
 * elements); _grad: df = dy * s[b]. */
int dmy_droppath_add(int dtype, const void* x, const void* f, const float* u, float keep, void* y, long per, long n,
                     void* stream);
int dmy_droppath_grad(int dtype, const void* dy, const float* u, float keep, void* df, long per, long n, void* stream);

/* ---- optimizer step / EMA (train.py:216-222, 449-454; utils/torch_utils.py:329-339) and the GradScaler
 *      (train.py:354, 445-450).  scale / found: device [1] fp32 loss scale and non-finite flag, or both NULL
 *      (scaler disabled); the update is skipped on the device when *found != 0 (scaler.step). */
int dmy_chunk_size(void);
int dmy_sgd(float* const* p, const float* const* g, float* const* m, const long* n, const int* tid, const long* off,
            int nchunks, float lr, float momentum, float weight_decay, int nesterov, const float* scale,
            const float* found, void* stream);
/* dstep: NULL (bias corrections from the two floats) or the group's device step count before this step: the kernel
 * derives the bias corrections from it and advances it unless the GradScaler skipped the step (as torch's Adam t). */
int dmy_adam(float* const* p, const float* const* g, float* const* m, float* const* v, const long* n, const int* tid,
             const long* off, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay,
             float bias_corr1, float bias_corr2_sqrt, const float* scale, const float* found, int* dstep,
             void* stream);
/* scaler.unscale_ check: *found = 1 if any g * (1 / *scale) is non-finite (found is not cleared here) */
int dmy_amp_check(const float* const* g, const long* n, const int* tid, const long* off, int nchunks,
                  const float* scale, float* found, void* stream);
/* scaler.update(): backoff / growth of *scale, *gup = *scale * world (the loss's upstream gradient), re-arms found */
int dmy_amp_update(float* scale, float* gup, int* tracker, float* found, float world, float growth, float backoff,
                   int interval, void* stream);
int dmy_ema(float* const* ema, const float* const* src, const long* n, const int* tid, const long* off, int nchunks,
            float decay, void* stream);


/* ---- anchor-free TAL path: replaces models/detect_t.py:38-101 (TDetect outputs, DFL decode),
 *      utils/tal.py:81-221 (ComputeLoss_TAL, BboxLoss, bbox2dist) and utils/tal_assign.py:54-189
 *      (TaskAlignedAssigner); models/common.py:1451-1458 (space_to_depth).  H, W, stride are HOST
 *      arrays of nl entries; box / cls are read through (batch, channel, anchor) element strides. */
long dmy_tal_workspace_bytes(int B, int A, int cap);
int dmy_tal_loss(int dtype, const void* box, long sbb, long sbc, long sba, const void* cls, long scb, long scc, long sca,
                 int B, int nc, int nl, const int* H, const int* W, const float* stride, const float* targets, int nt,
                 float alpha, float beta, float pos_weight, void* workspace, float* G, float* loss, float* items,
                 void* stream);
int dmy_tal_flatten(int dtype, const void* x, long xps, int B, int H, int W, int A, int a0, int no, void* F, int backward,
                    void* stream);
int dmy_tal_detect_out(int dtype, const void* F, int B, int nc, int nl, const int* H, const int* W, const float* stride,
                       float* y, void* stream);
int dmy_space_to_depth(int dtype, const void* x, long xps, void* y, long yps, int N, int H, int W, int C, int backward,
                       void* stream);


/* ---- config-5 modules: CBAM (models/common.py:260-310) channel / spatial attention pieces; SPP
 *      (common.py:212-227) reuses dmy_maxpool_* with k = 3..13. */
/* global avg + max pool (CBAM ChannelAttentionModule avg_pool / max_pool, common.py:266-267):
 * out [2N][C] = (means; maxima), arg [N][C] = first argmax pixel.  ws: dmy_gpool_ws_bytes() of fp32 scratch. */
long dmy_gpool_ws_bytes(int dtype, int N, int HW, int C);
int dmy_gpool_fwd(int dtype, const void* x, long xps, int N, int HW, int C, void* out, int* arg, float* ws,
                  void* stream);
int dmy_gpool_bwd(int dtype, const void* dz, const int* arg, void* dx, long dxps, int accumulate, int N, int HW, int C,
                  void* stream);
int dmy_halves_sigmoid(int dtype, const void* z, int N, int C, void* ca, const void* dca, void* dz, void* stream);
int dmy_cbam_in_fwd(int dtype, const void* x, long xps, const void* ca, int N, int HW, int C, void* out1, void* s2,
                    int* am, void* stream);
long dmy_cbam_in_bwd_ws_elems(int N, int HW, int C);
int dmy_cbam_in_bwd(int dtype, const void* x, long xps, const void* ca, const void* dout1, long dps, const void* ds2,
                    const int* am, int N, int HW, int C, void* dx, long dxps, int accumulate, float* dca, float* ws,
                    void* stream);
int dmy_pixscale(int dtype, const void* out1, const void* sa, long sps, int N, int HW, int C, void* out, long ops,
                 const void* dout, long dps, void* dout1, void* dsa, void* stream);

/* ---- config-5 C3TR (models/common.py:184-189, 312-355): the attention core of the
 *      nn.MultiheadAttention (common.py:323; torch multi_head_attention_forward: softmax(q k^T / sqrt(d)) v
 *      per head, after the in-projection) over the H*W tokens of each image, and the TransformerLayer
 *      nn.Dropout(0.1) (common.py:328).  q/k/v/o are NHWC token rows [B*L][ps], head h = columns
 *      [h d, h d + d); lse2 = fp32 [B][nh][L] (log2-domain log-sum-exp, saved for the backward);
 *      Dq = fp32 workspace [B][nh][L]; dq/dk/dv use the token stride `ops`.  d <= 128; bf16 with
 *      d in {32, 64, 128} runs on MFMA, everything else on the fp32-math generic kernels.
 *      dmy_mha_fwd_ref always runs the generic kernel (test reference for the MFMA path). */
int dmy_mha_fwd(int dtype, const void* q, long qps, const void* k, long kps, const void* v, long vps, void* o, long ops,
                float* lse2, int B, int L, int nh, int d, float scale, void* stream);
int dmy_mha_fwd_ref(int dtype, const void* q, long qps, const void* k, long kps, const void* v, long vps, void* o,
                    long ops, float* lse2, int B, int L, int nh, int d, float scale, void* stream);
int dmy_mha_bwd(int dtype, const void* q, long qps, const void* k, long kps, const void* v, long vps, const void* o,
                const void* dout, long ops, const float* lse2, float* Dq, void* dq, void* dk, void* dv, int B, int L,
                int nh, int d, float scale, void* stream);
/* y[m][c] = x[m][c] * (u(*seed, m * C + c) >= p) / (1 - p); the same call with the same seed on dy is the backward.
 * seed is device memory (graph-replay safe); dmy_dropout_seed advances a device generator state and writes a
 * fresh seed (nn.Dropout's per-call RNG draw, common.py:328). */
int dmy_dropout_seed(unsigned long long* state, unsigned long long* seed, void* stream);
int dmy_dropout(int dtype, const void* x, long xps, void* y, long yps, long M, int C, float p,
                const unsigned long long* seed, void* stream);

/* ---- validation matching: replaces process_batch (val.py:62-83) with box_iou (utils/metrics.py:254-276) for
 *      a batch of images in one launch.  det [ND][6] (x1 y1 x2 y2 conf cls), lab [NL][5] (cls x1 y1 x2 y2),
 *      det_off / lab_off [B + 1] per-image row offsets, iouv [T]; workspaces ws_* of ND entries;
 *      correct [ND][T] (0/1).  Matching rules: csrc/metrics.hip header. */
int dmy_process_batch(const float* det, const int* det_off, const float* lab, const int* lab_off, int B,
                      const float* iouv, int T, int* ws_lab, float* ws_iou, int* ws_win, unsigned char* correct,
                      void* stream);

/* ---- confusion matrix: replaces ConfusionMatrix.process_batch (utils/metrics.py:122-160) for a batch of images
 *      in one launch, over the packed layout of dmy_process_batch.  Only detections with conf > `conf` take
 *      part; a (label, detection) pair is a candidate when iou > iou_thres (both strict, classes not compared).
 *      ws_lab / ws_iou / ws_win: ND entries, ws_lab_win: NL entries.  matrix [(nc + 1)][(nc + 1)] 64-bit
 *      counters, row = predicted class, column = true class, index nc = background; the entry ADDS into it and
 *      never clears it.  A class outside [0, nc) is not stored.  Matching rules: csrc/metrics.hip header. */
int dmy_confusion_matrix(const float* det, const int* det_off, const float* lab, const int* lab_off, int B, int nc,
                         float conf, float iou_thres, int* ws_lab, float* ws_iou, int* ws_win, int* ws_lab_win,
                         unsigned long long* matrix, void* stream);

/* ---- training augmentation tail (augment.hip): utils/datasets.py:552-622 after the random draws -- warp
 *      (cv2.warpAffine / warpPerspective INTER_LINEAR, border 114), mixup, augment_hsv, flips, BGR->RGB, HWC->CHW --
 *      for n host-built descriptors (984-byte AugDesc: canvas pointers, inverse maps, mixup ratio, HSV LUTs,
 *      flips; layout in dmayolo/augment.py AUG_DESC) into uint8 out [n, 3, OH, OW]. */
long dmy_aug_desc_bytes(void);
int dmy_augment_batch(const void* descs, int n, void* out, int OH, int OW, void* stream);
/* mosaic canvas composition (utils/datasets.py:680-724 with load_image :659-675's INTER_LINEAR resize): n MosaicDesc
 * (4 decoded images, their host-built resize tables and canvas rectangles; layout in dmayolo/augment.py MOSAIC_DESC,
 * sizeof = dmy_mosaic_desc_bytes) -> each desc's uint8 HWC BGR canvas of S2 x S2 (114 outside the four images). */
long dmy_mosaic_desc_bytes(void);
int dmy_mosaic_compose(const void* descs, int n, int S2, void* stream);

/* ---- AutoShape (autoshape.hip).
 *      dmy_letterbox_batch replaces AutoShape.forward's host pre-processing (models/common.py:775-778:
 *      letterbox(im, new_shape=shape1, auto=False) per image, stack, BHWC -> BCHW, / 255, cast) and the Model.to_input
 *      that follows: n device-resident 56-byte LetterboxDesc (source uint8 HWC pointer and size, unpadded size, the
 *      two [4, dst] int32 INTER_LINEAR tables, top / left pad, channel-swap flag; layout in dmayolo/models/common.py
 *      LETTERBOX_DESC, sizeof = dmy_letterbox_desc_bytes) -> y, the stem input of the batch in dtype (0 fp32, 1 bf16):
 *      s2d = 1 [n][OH/2][OW/2][Cs] as dmy_image_s2d, s2d = 0 [n][OH][OW][Cs] as dmy_nchw_to_nhwc; the value is the
 *      letterboxed uint8 level (114 in the border) times scale.  host_descs is the host copy of descs, read for the
 *      geometry checks: odd OH / OW with s2d, a rectangle outside the canvas, Cs not a whole number of 16-byte vectors
 *      or y unaligned return hipErrorInvalidValue before any launch.
 *      dmy_scale_boxes replaces scale_coords (utils/general.py:605-617) per image and the Detections conversions
 *      (models/common.py:805-808) for the padded NMS output det [nimg][max_det][6] and its int32 keep counts: per
 *      image geom = (gain, pad_x, pad_y, w0, h0) fp32; det's xyxy is rewritten in place ((x - pad) / gain clamped to
 *      the image), xywh / xyxyn / xywhn receive xyxy2xywh and the divisions by (w0, h0, w0, h0); rows at or past an
 *      image's count are not touched.  fp32, IEEE divisions, the reference's operation order. */
long dmy_letterbox_desc_bytes(void);
int dmy_letterbox_batch(int dtype, const void* descs, const void* host_descs, int n, void* y, int OH, int OW, int s2d,
                        int Cs, float scale, void* stream);
int dmy_scale_boxes(void* det, const void* counts, const void* geom, void* xywh, void* xyxyn, void* xywhn, int nimg,
                    int max_det, void* stream);

/* ---- weighted boxes fusion (wbf.hip): ensemble_boxes.weighted_boxes_fusion, conf_type 'avg', allows_overflow False,
 *      as the reference's multi-model evaluation calls it (wbf.py:67), for every image of a batch at once. */
/* wbf.py:67 -- the most records (M * R) per image dmy_wbf takes */
int dmy_wbf_max_rows(void);
/* wbf.py:67 -- bytes of the workspace dmy_wbf needs for nimg images of rows = M * R records */
long dmy_wbf_workspace_bytes(int nimg, int rows);
/* wbf.py:67 -- det [M][nimg][R][6] fp32 (xyxy in pixels, conf, cls: the padded NMS layout stacked over M models),
 * counts [M][nimg] int32 valid rows, wh [nimg][2] fp32 image (width, height), weights [M] fp64 -> out [nimg][M * R][6]
 * fp32 fused rows (xyxy in pixels, score, label) in descending score order and nout [nimg] int32 row counts.  fp64
 * arithmetic, one rounding per operation.  M * R above dmy_wbf_max_rows, nimg above 65535 or a null / misaligned
 * pointer return hipErrorInvalidValue before any launch. */
int dmy_wbf(const float* det, const int* counts, const float* wh, const double* weights, int M, int nimg, int R,
            double iou_thr, double skip_box_thr, void* ws, float* out, int* nout, void* stream);

#ifdef __cplusplus
}
#endif
#endif

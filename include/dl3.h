/*
 * dl3.h — C ABI of libdl3.so: the MI355X (gfx950) native operator set behind
 * Deeplabv3() (reference: deeplabv3p.py:209-466, subpixel.py:41-103, utils.py:127-130,169-214).
 *
 * The reference has no FFI of its own: every FLOP of its hot path runs inside
 * Keras/TensorFlow layer objects (Conv2D, DepthwiseConv2D, BatchNormalization, ...,
 * imported at deeplabv3p.py:29-40).  Each entry point below replaces the device-side
 * work of one of those layer types (forward and gradients); the Python host layer in
 * keras-segmentation-deeplab-v3.1_amd/ re-exposes the reference's Deeplabv3()/Subpixel/
 * SegModel surface on top of them.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - every op returns int: 0 OK, -1 bad argument, -2 HIP error, -3 workspace too small,
 *    -4 unsupported configuration; dl3_last_error() gives a thread-local message.
 *  - all tensor pointers are caller-owned DEVICE pointers (fp32 unless noted), NHWC,
 *    weights in Keras layouts (pointwise [K][N]; depthwise [3][3][C]; dense [3][3][Cin][Cout]).
 *  - no allocation, no synchronisation, no global mutable state inside ops; the last
 *    argument is the hipStream_t to enqueue on.  Ops are hipGraph-capturable.
 *    Two documented exceptions, both opt-in and off by default: dl3_set_gemm_math() is a
 *    process-wide switch (by design: it selects the arithmetic of every later launch), and in
 *    split math (DL3_MATH_SPLIT) the dl3_pwconv_fwd / _bwd_data launches keep ONE device
 *    scratch per device for the launch's pre-split weights, grown with hipMalloc on first use —
 *    so the first split-math launch of a process must not be issued inside a stream capture
 *    (it returns -1 with a message; the engine's eager warm-up step takes care of it).  The
 *    f32 path — the default, and the only one any benchmark headline uses — keeps the rule.
 *  - "input transform": a tensor is handed over as (raw, scale[C], shift[C], act) and is
 *    read as act(scale*raw+shift) — BatchNorm + ReLU/ReLU6 of the PRODUCER are applied on
 *    load by the consumer, so an activation is written once and read once.  scale==NULL
 *    means identity affine.
 *  - "gradient operand": dY is handed over as (g, yraw, cA[C], cB[C], cC[C]) and read as
 *    cA*g + cB*yraw + cC — the BatchNorm backward of the producer applied on load
 *    (cA==NULL means dY = g).
 *  - "partials": per-channel reductions (BN batch statistics, BN backward sums, weight
 *    gradients) are written as P deterministic partial rows; dl3_*_partials() returns P
 *    for a shape, dl3_bn_finalize()/dl3_bn_bwd_finalize()/dl3_reduce_partials() fold them
 *    in a fixed order.  No float atomics anywhere: results are run-to-run bit-identical.
 */
#ifndef DL3_H
#define DL3_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DL3_OK 0
#define DL3_EINVAL (-1)
#define DL3_EHIP (-2)
#define DL3_EWORKSPACE (-3)
#define DL3_EUNSUPPORTED (-4)

#define DL3_ACT_NONE 0
#define DL3_ACT_RELU 1  /* Activation('relu')            deeplabv3p.py:72,77,82,287,380,387,409 */
#define DL3_ACT_RELU6 2 /* relu(x, max_value=6.)         deeplabv3p.py:181,192,325 */

#define DL3_IMPL_AUTO 0
#define DL3_IMPL_GATHER 1 /* generic 9-tap gather kernel (any stride / rate / pad) */
#define DL3_IMPL_MARCH 2  /* stride-1 row-marching kernel (each input row read once) */

int dl3_version(void);
const char *dl3_last_error(void);

/* ---- DepthwiseConv2D 3x3 (deeplabv3p.py:73-74, :186-188) ------------------------------ */
/* number of partial rows P written by dwconv fwd (stat_partial [P][C][2]) and bwd
 * (dstat_partial [P][C][2], dw_partial [P][9][C]) for this shape/impl.  The pads are not an argument: DL3_IMPL_AUTO counts
 * the rows of the march kernels for every stride-1 geometry with Ho == H and Wo == W.  Where such a geometry's pads are not
 * its rate the launches need the gather kernels and more rows: they return DL3_EUNSUPPORTED under DL3_IMPL_AUTO; size and
 * launch it with DL3_IMPL_GATHER. */
int dl3_dwconv3x3_partials(int N, int H, int W, int C, int stride, int rate, int Ho, int Wo, int impl);
/* y[n,oy,ox,c] = sum_{i,j} T(x)[n, oy*stride-pad_t+i*rate, ox*stride-pad_l+j*rate, c] * w[i][j][c];
 * stat_partial (nullable): per-channel sum(y), sum(y^2) partials */
int dl3_dwconv3x3_fwd(const float *x, const float *in_scale, const float *in_shift, int in_act,
                      const float *w, float *y, int N, int H, int W, int C, int stride, int rate,
                      int pad_t, int pad_l, int Ho, int Wo, float *stat_partial, int impl, void *stream);
/* fused bwd-data + bwd-weight.
 *   dY = cA*g + cB*yraw + cC                                   [N,Ho,Wo,C]
 *   dw_partial[p][i][j][c] = partial sum_{n,oy,ox} T(x)[...tap...] * dY
 *   dx = mask_{in_act}(conv^T(dY, w)) + dx_add                 [N,H,W,C]   (dx nullable)
 *   dstat_partial (nullable): sum(dx), sum(dx * (x-x_mean)*x_invstd) partials */
int dl3_dwconv3x3_bwd(const float *g, const float *yraw, const float *cA, const float *cB, const float *cC,
                      const float *x, const float *in_scale, const float *in_shift, int in_act,
                      const float *w, float *dx, const float *dx_add, const float *x_mean,
                      const float *x_invstd, float *dstat_partial, float *dw_partial, int N, int H, int W,
                      int C, int stride, int rate, int pad_t, int pad_l, int Ho, int Wo, int impl, void *stream);

/* the same launch with the BatchNorm-backward sums of dx taken against ANOTHER tensor: dstat_partial = sum(dx),
 * sum(dx * (stat_x - x_mean) * x_invstd), stat_x [N,H,W,C] — the other input of the residual Add whose output gradient
 * this launch completes (Xception's `sum` shortcuts, deeplabv3p.py:147-149: the gradient reaches the block's last
 * pointwise BatchNorm unchanged, so its sums need no pass of their own; round 4).  March kernel only (stride 1, SAME). */
int dl3_dwconv3x3_bwd_sx(const float *g, const float *yraw, const float *cA, const float *cB, const float *cC,
                         const float *x, const float *in_scale, const float *in_shift, int in_act, const float *w,
                         float *dx, const float *dx_add, const float *stat_x, const float *x_mean,
                         const float *x_invstd, float *dstat_partial, float *dw_partial, int N, int H, int W, int C,
                         int stride, int rate, int pad_t, int pad_l, int Ho, int Wo, int impl, void *stream);

/* ---- Conv2D 1x1 = GEMM on fp32 MFMA (deeplabv3p.py:78-79,:175,:194,:377,:385,:406,:420,:438) -- */
#define DL3_MATH_ENV (-1)  /* follow the environment (DL3_GEMM_MATH=split selects split math); the default */
#define DL3_MATH_F32 0     /* v_mfma_f32_32x32x2_f32 */
#define DL3_MATH_SPLIT 1   /* fp32 operands cut exactly into three bf16 pieces, six of the nine piece products on
                              v_mfma_f32_32x32x16_bf16, fp32 accumulate (same error class as the f32 MFMA) */
/* matrix math of the dl3_pwconv_* launches issued after the call (process-wide; launches already captured in a
 * hipGraph keep what they were captured with); dl3_get_gemm_math returns the mode in effect (0 or 1) */
int dl3_set_gemm_math(int mode);
int dl3_get_gemm_math(void);
/* The four queries below and dl3_pwconv_bwd_weight_splits are answers of the launch planner (csrc/pwplan.h) that every
 * dl3_pwconv_* launch goes through: they describe the dispatch itself, not a restatement of it.
 * P for the [M,K]x[K,N] GEMM's per-output-channel partials: the most rows any launch of that shape writes, over forward and
 * bwd-data, one- and two-tensor operands, with and without mask / addend, aligned and unaligned operands, f32 and split
 * math (plus the floors listed beside query_partials).  A launch that would write more rows than that returns DL3_EINVAL
 * before anything runs. */
int dl3_pwconv_partials(int M, int K, int N);
/* which kernel a dl3_pwconv_fwd launch of this shape takes (dl3_pwconv_route dir 0: 16-byte aligned operands, rows back to
 * back, no addend): 0 the tiled MFMA GEMM, 1 the weight-stationary streaming kernel of the HBM-bound layers (round 5: the
 * whole K x N matrix in LDS, every wave walks 32-row tiles on its own, 16-byte stores; deeplabv3p.py:175-198 at
 * 16..192 channels, M >= 32768), 2 the weight-stationary kernel of the MFMA-bound short reductions (round 6: K = 160 / 96 /
 * 64 into an output at least twice as wide, M >= 98304 forward / 65536 bwd-data, 131072 for K = 64; DL3_WS2=0 disables it — and its packed-output variant for the
 * logits layer, K = 256, N <= 32, ldy == N, M >= 8192; DL3_NARROW=0).  Diagnostic only. */
int dl3_pwconv_fwd_impl(int M, int K, int N);
/* ... and the route of a launch by name, for plans that want to assert what they benchmark (tests/test_host.py): the route
 * of the planner's plan for the canonical operand form of each dir (16-byte aligned operands, rows back to back) —
 * dir 0 = forward (as dl3_pwconv_fwd_impl), 1 = bwd-data with the single-tensor dY, a mask operand and no addend, 2 = the
 * weight gradient (two-tensor operand), 3 = bwd-data with the single-tensor dY (rows back to back) and neither mask, addend
 * nor BatchNorm sums (the logits layer), 4 = the weight gradient with a single-tensor dY, folded by the launch (dw given),
 * bias gradient optional (2, 4: 16-byte aligned operands, leading dimensions multiples of 4).
 * Returns DL3_ROUTE_*.  Diagnostic only. */
#define DL3_ROUTE_TILED 0      /* pw_gemm_stream_kernel / pw_gemm_kernel / pw_wgrad_kernel */
#define DL3_ROUTE_WS_HBM 1     /* pw_fwd_ws_kernel */
#define DL3_ROUTE_WS_MFMA 2    /* pw_ws2_kernel */
#define DL3_ROUTE_KSPLIT 3     /* pw_ksplit32_kernel (1 024 - 16 384 rows) */
#define DL3_ROUTE_WGRAD_ROW 4  /* pw_wgrad_row_kernel (one tile row over K) */
#define DL3_ROUTE_NARROW 5     /* the logits layer, N = classes <= 32 off a 256-wide input: pw_ws2_kernel FLAT (dir 0),
                                  pw_narrowk_kernel (dir 3), pw_wgrad_narrow_kernel (dir 4) */
int dl3_pwconv_route(int dir, int M, int K, int N);
/* y[M,N](ldy) = T(x)[M,K](ldx) . w[K,N] (+bias[N]); stat_partial (nullable) [P][N][2] = sum(y), sum(y^2) */
int dl3_pwconv_fwd(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act,
                   const float *w, const float *bias, float *y, int ldy, int M, int K, int N,
                   float *stat_partial, void *stream);
/* the same with an addend: y[m,:] += add[(m / add_div) * ldadd + :] — add_div = 1: a residual tensor; add_div = H*W: one
 * row per image, i.e. the contribution of channels that are constant over the image (the ASPP image-pooling branch,
 * deeplabv3p.py:375-382,:402-406: the broadcast 1x1 feature never has to be materialised or multiplied per pixel) */
int dl3_pwconv_fwd_add(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act,
                       const float *w, const float *bias, float *y, int ldy, int M, int K, int N,
                       float *stat_partial, const float *add, int ldadd, int add_div, void *stream);
/* the same product for a FEW rows — one per image: the ASPP image-pooling branch (deeplabv3p.py:375-382) and its share of
 * concat_projection (:402-406) — accumulated in DOUBLE and rounded once (round 5).  The result is a per-image constant the
 * network adds to every pixel of the map: its rounding error does not average out over pixels, and a reduction of 2 048 on
 * the f32 MFMA was where the path's distance to float64 left torch-fp32's (tools/r5/xception_layer_distance.py).  add
 * (nullable): y[m,:] += add[(m / add_div) * ldadd + :].  No BatchNorm partial sums (few rows: dl3_bn_finalize_direct). */
int dl3_pwconv_fwd_rows(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act,
                        const float *w, const float *bias, float *y, int ldy, int M, int K, int N, const float *add,
                        int ldadd, int add_div, void *stream);
/* dx[M,K](lddx) = mask_{in_act}(dY[M,N] . wT[N,K]) + add_scale*dx_add ; dY = cA*g + cB*yraw + cC.
 * x/in_scale/in_shift/in_act describe the FORWARD input (needed for the mask and x_hat);
 * dx_add row address = dx_add + (m / add_div)*ldadd (add_div = H*W broadcasts a per-image vector);
 * dstat_partial (nullable) [P'][K][2] = sum(dx), sum(dx*(x-x_mean)*x_invstd), P' = dl3_pwconv_partials(M,N,K) */
int dl3_pwconv_bwd_data(const float *g, int ldg, const float *yraw, int ldyraw, const float *cA,
                        const float *cB, const float *cC, const float *wT, float *dx, int lddx,
                        const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act,
                        const float *dx_add, int ldadd, int add_div, float add_scale, const float *x_mean,
                        const float *x_invstd, float *dstat_partial, int M, int K, int N, void *stream);
/* bytes of workspace a dl3_pwconv_bwd_weight* launch of this shape needs: the slabs and bias column-sum rows of the largest of
 * the planner's plans over the launch's operand forms (two-tensor dY; single-tensor dY folded by the launch; single-tensor
 * dY with the slabs left to the caller) */
size_t dl3_pwconv_bwd_weight_workspace(int M, int K, int N);
/* dw[K,N] = T(x)^T . dY ; dbias[N] (nullable) = colsum(dY).  The launch reduces over M in S =
 * dl3_pwconv_bwd_weight_splits(M, K, N, cA != NULL) deterministic slabs [S][K][N] at the head of the workspace and folds
 * them into dw.  dw == NULL (then dbias must be NULL too) leaves the slabs where they are: the caller folds them later —
 * dl3_reduce_partials(workspace, S, K*N, dw), or together with every other weight gradient of the step in ONE
 * dl3_reduce_partials_batched launch (the workspace must then be the launch's own until that fold has run). */
int dl3_pwconv_bwd_weight_splits(int M, int K, int N, int two_tensor_dy);
int dl3_pwconv_bwd_weight(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act,
                          const float *g, int ldg, const float *yraw, int ldyraw, const float *cA,
                          const float *cB, const float *cC, float *dw, float *dbias, int M, int K, int N,
                          void *workspace, size_t workspace_bytes, void *stream);
/* the same launch, which also writes the gradient operand it assembles anyway, dy_out[M][N](lddy) = cA*g + cB*yraw + cC
 * (round 4): dl3_pwconv_bwd_data of the same layer can then be handed (g = dy_out, cA = NULL) — ONE operand tensor, no
 * operand transform, and with it the room for a straight-line masked epilogue.  Costs one write of dY; the bwd-data GEMM
 * reads one tensor less.  dy_out 16-byte aligned, lddy >= N and a multiple of 4.  Replaces the BatchNormalization
 * backward TF runs as a separate op in front of both Conv2D gradients (deeplabv3p.py:175-201 expand / project convs). */
int dl3_pwconv_bwd_weight_dy(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act,
                             const float *g, int ldg, const float *yraw, int ldyraw, const float *cA,
                             const float *cB, const float *cC, float *dw, float *dbias, int M, int K, int N,
                             void *workspace, size_t workspace_bytes, float *dy_out, int lddy, void *stream);
/* Both gradients of a 1x1 convolution in ONE pass over (g, yraw, x) — for the HBM-bound layers with a small weight matrix
 * (round 4: the expand / project convolutions of the first inverted-residual blocks, deeplabv3p.py:175-201, 16..144
 * channels on 256x256 / 128x128 maps, where _bwd_weight and _bwd_data each read the wide gradient operand once):
 *   dw[K,N] = T(x)^T . dY                                  (dw == NULL: the [S][K][N] slabs stay in the workspace)
 *   dx[M,K](lddx) = mask_{in_act}(dY . wT[N,K]) + dx_add   dY = cA*g + cB*yraw + cC
 *   dstat_partial (nullable) [S][K][2] = sum(dx), sum(dx * (stat_x - x_mean) * x_invstd) — stat_x is the forward input
 *   itself or, when the gradient reaches another BatchNorm'ed tensor unchanged through a residual Add, that tensor.
 * S = dl3_pwconv_bwd_fused_splits(M, K, N) workgroups / slabs / partial rows; workspace >= _workspace(M, K, N) bytes.
 * _supported: 0 unless K, N are multiples of 4 with ceil(K/32) * ceil(N/32) <= 6; 2: any epilogue; 1 (K > 64): without
 * dx_add and with stat_x == x only (-4 otherwise).  All operands 16-byte aligned, leading dimensions multiples of 4. */
int dl3_pwconv_bwd_fused_supported(int M, int K, int N);
int dl3_pwconv_bwd_fused_splits(int M, int K, int N);
size_t dl3_pwconv_bwd_fused_workspace(int M, int K, int N);
int dl3_pwconv_bwd_fused(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act,
                         const float *g, int ldg, const float *yraw, int ldyraw, const float *cA, const float *cB,
                         const float *cC, const float *wT, float *dw, float *dx, int lddx, const float *dx_add,
                         int ldadd, const float *stat_x, int ldstatx, const float *x_mean, const float *x_invstd,
                         float *dstat_partial, int M, int K, int N, void *workspace, size_t workspace_bytes,
                         void *stream);
/* out[cols][rows] = in[rows][cols]^T  (W[K,N] -> WT[N,K] for bwd_data) */
int dl3_transpose(const float *in, float *out, int rows, int cols, void *stream);
/* n transposes in one launch (all W -> WT of a backward pass).  desc (device, int64 [n][6]): in pointer, out pointer,
 * rows, cols, index of the matrix's first 32x32 tile, tiles per tile-row (= ceil(cols/32)); matrices in ascending
 * first-tile order; total_tiles = sum of ceil(rows/32)*ceil(cols/32). */
int dl3_transpose_batched(const long long *desc, int n, int total_tiles, void *stream);

/* ---- dense Conv2D 3x3 (stem convs: deeplabv3p.py:283,:289,:318) ----------------------- */
int dl3_conv3x3_partials(int N, int Ho, int Wo, int Cout);
int dl3_conv3x3_fwd(const float *x, const float *in_scale, const float *in_shift, int in_act, const float *w,
                    float *y, int N, int H, int W, int Cin, int Cout, int stride, int pad_t, int pad_l,
                    int Ho, int Wo, float *stat_partial, void *stream);
/* dw_partial [P][3][3][Cin][Cout] */
int dl3_conv3x3_bwd_weight(const float *x, const float *in_scale, const float *in_shift, int in_act,
                           const float *g, const float *yraw, const float *cA, const float *cB,
                           const float *cC, float *dw_partial, int N, int H, int W, int Cin, int Cout,
                           int stride, int pad_t, int pad_l, int Ho, int Wo, void *stream);
/* dx = mask(conv^T(dY,w)) + dx_add, optional dstat partials ([P'][Cin][2], P' = dl3_conv3x3_partials(N,H,W,Cin)) */
int dl3_conv3x3_bwd_data(const float *g, const float *yraw, const float *cA, const float *cB, const float *cC,
                         const float *w, float *dx, const float *x, const float *in_scale,
                         const float *in_shift, int in_act, const float *dx_add, const float *x_mean,
                         const float *x_invstd, float *dstat_partial, int N, int H, int W, int Cin, int Cout,
                         int stride, int pad_t, int pad_l, int Ho, int Wo, void *stream);

/* Matrix-pipe route for a dense 3x3 conv between 32- or 64-channel tensors (xception entry_flow_conv1_2 32 -> 64,
 * deeplabv3p.py:289), im2col-free: the taps are gathered straight into the MFMA A operand, the weight slice of one tap
 * is the LDS-staged B operand.  Same semantics as the three ops above except: the stat partial buffers have
 * P = dl3_conv3x3_mfma_partials(N, Ho, Wo) (forward) / (N, H, W) (bwd-data) rows; bwd_weight writes the finished
 * dw [3][3][Cin][Cout] (its per-workgroup slabs live in the caller's workspace); bwd_data takes
 * wT [Cout][9*Cin] (dl3_transpose of w). */
int dl3_conv3x3_mfma_supported(int Cin, int Cout);
int dl3_conv3x3_mfma_partials(int N, int Hc, int Wc);
int dl3_conv3x3_mfma_fwd(const float *x, const float *in_scale, const float *in_shift, int in_act, const float *w,
                         float *y, int N, int H, int W, int Cin, int Cout, int stride, int pad_t, int pad_l, int Ho,
                         int Wo, float *stat_partial, void *stream);
size_t dl3_conv3x3_mfma_bwd_weight_workspace(int N, int H, int W, int Cin, int Cout, int stride, int Ho, int Wo);
int dl3_conv3x3_mfma_bwd_weight(const float *x, const float *in_scale, const float *in_shift, int in_act,
                                const float *g, const float *yraw, const float *cA, const float *cB, const float *cC,
                                float *dw, int N, int H, int W, int Cin, int Cout, int stride, int pad_t, int pad_l,
                                int Ho, int Wo, void *workspace, size_t workspace_bytes, void *stream);
int dl3_conv3x3_mfma_bwd_data(const float *g, const float *yraw, const float *cA, const float *cB, const float *cC,
                              const float *wT, float *dx, const float *x, const float *in_scale,
                              const float *in_shift, int in_act, const float *dx_add, const float *x_mean,
                              const float *x_invstd, float *dstat_partial, int N, int H, int W, int Cin, int Cout,
                              int stride, int pad_t, int pad_l, int Ho, int Wo, void *stream);

/* ---- BatchNormalization (54 layers mnv2 / 146 xception; eps 1e-3 or 1e-5) -------------- */
/* training mode: fold stat partials [P][ldc][2] (channels c0..c0+C-1 at partial + 2*c0) into
 * scale = gamma*invstd, shift = beta - mean*scale, mean, invstd (biased batch variance) and
 * update the moving statistics: moving_mean = m*moving_mean + (1-m)*mean,
 * moving_var = m*moving_var + (1-m)*var_unbias*biased_var.  count = n = N*H*W.  var_unbias is the framework's
 * sample-variance factor, chosen by the host: Keras 2.2.4 on TF 1.13 (the reference's environment) multiplies
 * FusedBatchNorm's already Bessel-corrected batch variance by n/(n-(1+eps)) once more (keras/layers/normalization.py
 * `variance *= sample_size / (sample_size - (1.0 + self.epsilon))`), i.e. var_unbias = n/(n-1) * n/(n-(1+eps));
 * tf.keras uses n/(n-1).  moving_mean/moving_var NULL (together): a non-trainable layer, whose moving statistics
 * Keras 2.2.x leaves untouched. */
int dl3_bn_finalize(const float *stat_partial, int P, int ldc, int C, double count, const float *gamma,
                    const float *beta, float eps, float momentum, double var_unbias, float *scale, float *shift,
                    float *mean, float *invstd, float *moving_mean, float *moving_var, void *stream);
/* the same outputs for a SMALL tensor y[M][ldy] (channels 0..C-1), statistics taken straight from its values in two
 * double-precision passes (mean, then squared deviations).  The partial-sum form computes sum(y^2)/n - mean^2, which
 * cancels catastrophically when |mean| >> spread: the image-pooling BatchNorm (deeplabv3p.py:375-379) sees ONE value per
 * image.  The host uses it for M <= 4096 rows. */
int dl3_bn_finalize_direct(const float *y, int ldy, int M, int C, const float *gamma, const float *beta, float eps,
                           float momentum, double var_unbias, float *scale, float *shift, float *mean, float *invstd,
                           float *moving_mean, float *moving_var, void *stream);
/* inference / frozen mode: scale, shift, mean, invstd from the moving statistics */
int dl3_bn_frozen(const float *gamma, const float *beta, const float *moving_mean, const float *moving_var,
                  float eps, int C, float *scale, float *shift, float *mean, float *invstd, void *stream);
/* the same for a tensor whose PRODUCER subtracts the mean: neg_mean[C] = -moving_mean is handed to the producing
 * convolution as its bias (a BatchNorm'ed Conv2D has none of its own, deeplabv3p.py:78-79), the tensor holds y - mean,
 * and consumers read scale*(y - mean) + beta with scale = gamma*invstd, shift = beta, mean = 0.  scale*y + (beta -
 * mean*scale) rounds the large product mean*scale into the shift once and for all — half an ulp of |mean*scale| on
 * every element, the size of the tensor's own rounding noise when |mean| >> sigma; (y - mean) is exact there.  This is
 * the form the reference's BatchNormalization evaluates in inference, gamma*(x - mean)/sqrt(var + eps) + beta. */
int dl3_bn_frozen_centered(const float *gamma, const float *beta, const float *moving_mean, const float *moving_var,
                           float eps, int C, float *scale, float *shift, float *mean, float *invstd, float *neg_mean,
                           void *stream);
/* fold backward partials (sum g, sum g*x_hat) into dgamma, dbeta and the on-load coefficients
 * dY = cA*g + cB*yraw + cC.  batch_mode=1: full BN backward; 0: frozen statistics (cB=cC=0). */
int dl3_bn_bwd_finalize(const float *dstat_partial, int P, int ldc, int C, double count, const float *gamma,
                        const float *mean, const float *invstd, int batch_mode, float *cA, float *cB,
                        float *cC, float *dgamma, float *dbeta, void *stream);

/* ---- element-wise / reductions ------------------------------------------------------- */
int dl3_rows_partials(int M); /* P for row-wise reducing kernels over M rows */
/* out = act_a(sa*a+ta) + act_b(sb*b+tb)  (b nullable): Add (deeplabv3p.py:147-149,:201) and
 * materialisation of a BN(+act) output.  Optional Dropout (deeplabv3p.py:410): if drop_rate>0,
 * out *= keep_mask(seed, step, element index)/(1-drop_rate). */
int dl3_affine_add(const float *a, int lda, const float *sa, const float *ta, int act_a, const float *b,
                   int ldb, const float *sb, const float *tb, int act_b, float *out, int ldo, int M, int C,
                   float drop_rate, unsigned long long drop_seed, const unsigned long long *drop_step, void *stream);
/* *counter += inc (device memory).  The dropout step number: launch arguments are frozen inside a captured hipGraph,
 * so kernels read the step from *drop_step (nullable) and use the seed drop_seed + step * 0xD1B54A32D192ED03. */
int dl3_counter_add(unsigned long long *counter, unsigned long long inc, void *stream);
/* gout = mask_{act}(gin_scale * gin[m / gin_div] * dropmask/(1-rate)) + add ; gin_div = H*W broadcasts a
 * per-image gradient vector (backward of the global average pool); dstat partials [P][C][2] (nullable),
 * P = dl3_rows_partials(M).  gout may alias gin (gin_div == 1) and/or add. */
int dl3_grad_finish(const float *gin, int ldgin, int gin_div, float gin_scale, float *gout, int ldgout,
                    const float *add, int ldadd, const float *xraw, int ldx, const float *scale,
                    const float *shift, int act, const float *mean, const float *invstd, float *dstat_partial,
                    int M, int C, float drop_rate, unsigned long long drop_seed, const unsigned long long *drop_step,
                    void *stream);
/* strided 1x1 convolutions (Xception shortcuts, _conv2d_same(kernel_size=1, stride=2), deeplabv3p.py:143-145) sample
 * rows/cols 0, s, 2s, ...: y[n,oy,ox,c] = T(x)[n, oy*s, ox*s, c] compacts the sampled pixels for the GEMM;
 * the backward scatters the compact gradient back (zeros elsewhere). */
int dl3_subsample_fwd(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act, float *y,
                      int N, int H, int W, int C, int stride, int Ho, int Wo, void *stream);
int dl3_subsample_bwd(const float *g, float *dx, int N, int H, int W, int C, int stride, int Ho, int Wo, void *stream);
/* AveragePooling2D over the whole map (deeplabv3p.py:375): out[n][c] = out_scale * sum_hw T(x)[n,hw,c] */
int dl3_gap_fwd(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act, float *out,
                int N, int HW, int C, float out_scale, void *stream);
/* tf.image.resize_bilinear, TF1 legacy (align_corners=False, no half-pixel): deeplabv3p.py:382,:418,:439 */
int dl3_resize_bilinear_fwd(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act,
                            float *y, int ldy, int N, int Hi, int Wi, int Ho, int Wo, int C, void *stream);
/* dx[N,Hi,Wi,C] (+= if accumulate) = resize^T(dy) — deterministic gather form.  With a workspace of
 * dl3_resize_bilinear_bwd_workspace() bytes the transpose runs separably (columns, then rows: each dy element is
 * read once); workspace == NULL selects the single-pass 2-D gather. */
size_t dl3_resize_bilinear_bwd_workspace(int N, int Hi, int Wi, int Ho, int Wo, int C);
int dl3_resize_bilinear_bwd(const float *dy, int lddy, float *dx, int lddx, int N, int Hi, int Wi, int Ho,
                            int Wo, int C, int accumulate, void *workspace, size_t workspace_bytes, void *stream);
/* Subpixel._phase_shift (subpixel.py:77-88): out[n,ia*r+q,ib*r+p,ch] = in[n,ia,ib,ch*r*r+p*r+q];
 * inverse!=0 applies the inverse permutation (the backward pass) */
int dl3_phase_shift(const float *in, float *out, int N, int H, int W, int Cout, int r, int inverse, void *stream);
/* Subpixel head, training tail (utils.py:195-198 + the loss): softmax cross-entropy evaluated on the UNshuffled output u
 * [N,H,W,C*r*r] of the Subpixel convolution — labels / weights live at the shuffled resolution [N, H*r, W*r] — writing
 * du in u's own layout, so that neither the shuffled logits nor the shuffled gradient nor the two phase-shift passes
 * exist.  loss_partial [P], P = dl3_shuffle_xent_partials(...) (0: shape not supported, fall back to dl3_phase_shift +
 * dl3_softmax_xent).  C <= 32. */
int dl3_shuffle_xent_partials(int N, int H, int W, int C, int r);
int dl3_shuffle_softmax_xent(const float *u, const float *labels, const float *weights, const float *nnz, float *du,
                             float *loss_partial, int N, int H, int W, int C, int r, void *stream);
/* Subpixel with kernel_size > 1 (subpixel.py:42-58: Subpixel IS a Conv2D with any kernel_size; icnr_weights' default
 * shape is 3x3, subpixel.py:9): the k x k taps of T(x) = act(scale*x+shift), zero outside the image, gathered next to
 * each other — cols[(n,oy,ox)][(i*k+j)*C + c] = T(x)[n, oy-pad_t+i, ox-pad_l+j, c] (stride 1) — so that the Keras
 * kernel [k][k][C][F] read as a [k*k*C][F] matrix drives the ordinary 1x1 GEMM entry points.  _bwd is the transpose:
 * dx[n,iy,ix,c] = sum over taps of dcols (deterministic gather, no atomics). */
int dl3_conv_taps_fwd(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act, float *cols,
                      int N, int H, int W, int C, int k, int pad_t, int pad_l, int Ho, int Wo, void *stream);
int dl3_conv_taps_bwd(const float *dcols, float *dx, int N, int H, int W, int C, int k, int pad_t, int pad_l, int Ho,
                      int Wo, void *stream);
/* softmax over the last axis (deeplabv3p.py:441,:444) */
int dl3_softmax_fwd(const float *logits, float *probs, int M, int C, void *stream);
/* argmax over the last axis -> int32 (first maximum wins, like np.argmax) */
int dl3_argmax(const float *x, int *out, int M, int C, void *stream);
/* count of non-zero sample weights -> *out (float) ; sparse_crossentropy_ignoring_last_label
 * (utils.py:127-130) with Keras temporal sample weights:
 *   loss = sum_m w[m]*(-log clip(p[m,label]))/nnz ; dlogits = (p - onehot)*w/nnz ; label==C (void): onehot=0.
 * loss_partial [P] (P = dl3_rows_partials(M)) holds per-block shares of the loss (already divided by nnz);
 * probs nullable. */
int dl3_count_nonzero(const float *w, int M, float *out, void *stream);
int dl3_softmax_xent(const float *logits, const float *labels, const float *weights, const float *nnz,
                     float *probs, float *dlogits, float *loss_partial, int M, int C, void *stream);
/* the same loss with the final resize_bilinear (deeplabv3p.py:439, utils.py:190) fused in: logits_lo is the
 * [N,Hi,Wi,C] output of the logits conv, labels / weights / dlogits live at [N,Ho,Wo]; the full-resolution logits
 * are interpolated in registers and never touch HBM.  C <= 32. */
int dl3_upsample_softmax_xent(const float *logits_lo, const float *labels, const float *weights, const float *nnz,
                              float *probs, float *dlogits, float *loss_partial, int N, int Hi, int Wi, int Ho, int Wo,
                              int C, void *stream);
/* the training tail without the full-resolution gradient: loss as above, and the x half of the transposed resize
 * applied on chip — dlogits_xfold [N,Ho,Wi,C] = sum over the output columns of each output row (fixed order);
 * dl3_resize_bilinear_bwd_rows folds the rows (the y half) into dx [N,Hi,Wi,C].  loss_partial has
 * P = dl3_xent_fold_partials(N, Ho) entries.  C <= 32 and (Wo + 2*Wi)*C*4 <= 64 KB (an output row and its two
 * source rows live in LDS). */
int dl3_xent_fold_partials(int N, int Ho);
int dl3_upsample_softmax_xent_fold(const float *logits_lo, const float *labels, const float *weights, const float *nnz,
                                   float *dlogits_xfold, float *loss_partial, int N, int Hi, int Wi, int Ho, int Wo,
                                   int C, void *stream);
int dl3_resize_bilinear_bwd_rows(const float *xfold, float *dx, int lddx, int N, int Hi, int Wi, int Ho, int C,
                                 int accumulate, void *stream);
/* ---- hard-example mining in front of the loss kernels above (csrc/mine.hip; DeepLab's top_k_percent_pixels, restated
 * from memory of deeplab/utils/train_utils.py): the step trains on the k largest per-pixel losses.
 * v[m] = w[m] * -log clip(p[m,label], 1e-7, 1-1e-7) in fp32, +0 where the label is void or the product is not > 0;
 * weights nullable (w = 1).  One source per training form: materialised logits [M,C] (any C), the low-resolution
 * logits in front of the final resize (TF's stated weight, as dl3_upsample_softmax_xent's loss; C <= 32), the
 * UNshuffled Subpixel output u [N,H,W,C*r*r] (labels / weights / v at [N,H*r,W*r]; C <= 32). */
int dl3_pixel_xent_plain(const float *logits, const float *labels, const float *weights, float *v, int M, int C,
                         void *stream);
int dl3_pixel_xent_bilinear(const float *logits_lo, const float *labels, const float *weights, float *v, int N, int Hi,
                            int Wi, int Ho, int Wo, int C, void *stream);
int dl3_pixel_xent_shuffle(const float *u, const float *labels, const float *weights, float *v, int N, int H, int W,
                           int C, int r, void *stream);
/* *k = min(N, trunc(pct * N)), pct = p if S == 0 else ratio*p + (1 - ratio), ratio = min(1, s/S), s = *step (nullable:
 * 0) — every operation one rounded float32 operation; *tau = the k-th largest of v[N] (v >= 0: a radix select over the
 * bit patterns, +inf and denormals are ordinary values; k == 0: +inf, and dl3_mine_weights selects nothing).
 * ws: dl3_topk_workspace_bytes(N) bytes, zeroed by the call itself; deterministic (integer atomics only). */
size_t dl3_topk_workspace_bytes(int N);
int dl3_topk_threshold(const float *v, int N, float p, int S, const unsigned long long *step, void *ws, size_t ws_bytes,
                       int *k, float *tau, void *stream);
/* w_out[m] = weights[m] (nullable: 1) where v[m] >= *tau and v[m] > 0 (and *k > 0), else 0: ties at tau are all kept;
 * *nnz_out = their number, counted in integers and converted once.  ws is the workspace the dl3_topk_threshold call in
 * front of it used (it holds the counter, zeroed there). */
int dl3_mine_weights(const float *v, const float *weights, const float *tau, const int *k, float *w_out, float *nnz_out,
                     void *ws, int N, void *stream);
/* ---- soft-Jaccard term next to the training cross-entropy (csrc/jaccard.hip): CE + lambda * L_J ------
 * Our own definition, mirroring utils.Jaccard (utils.py:139-157).  B images of HW pixels, C <= 32 classes (-4 above):
 *   u = (w != 0 and label < C; weights NULL: w = 1), p = softmax(z) in fp32 (no renormalise, no clip), y the one-hot label;
 *   I = sum u p y, S = sum u p, Y = sum u y, U = S + Y - I per (image, class); present = Y > 0, J = I / U;
 *   n_c = #images that hold class c, n_legal = #classes with n_c > 0;
 *   L_J = 1 - (1 / n_legal) sum_c (1 / n_c) sum_b J  (0, with a zero gradient, when n_legal = 0: an all-void batch).
 * dl3_jaccard_sums_*: partials [B][P][3][C] (double; I, S, Y), P = dl3_jaccard_partials(B, HW); a workgroup never mixes
 *   two images, a lane accumulates in double, the waves meet in a fixed order.  plain: materialised logits [B*HW][C];
 *   bilinear: the low-resolution logits in front of the final resize, interpolated in registers with TF's stated weight —
 *   the logits dl3_upsample_softmax_xent sees (HW = Ho * Wo).
 * dl3_jaccard_coef: folds the partials in ascending order in double into sums [B][C][3] (I, S, Y), then
 *   kappa = present / (n_c n_legal), coef [B][C][2] = (A, Bc) = (-kappa / U, kappa I / U^2) rounded to float once,
 *   stats [4] (double) = (L_J, n_legal, lambda * L_J, -) and *loss_row (nullable) = (float)(lambda * L_J): an extra row of
 *   the loss partials, so that dl3_reduce_partials returns CE + lambda * L_J.  lambda is the only value frozen in the
 *   launch: everything else is read from device memory, so the launch replays in a captured graph.
 * dl3_softmax_xent_jaccard / dl3_upsample_softmax_xent_jaccard: loss_partial and the cross-entropy gradient exactly as
 *   dl3_softmax_xent / dl3_upsample_softmax_xent (operation for operation: with an all-zero coef the gradient is theirs
 *   bit for bit), plus lambda u p_k (G_k - sum_c p_c G_c), G_c = A[b,c] where c is the pixel's label, else Bc[b,c].
 *   loss_partial has dl3_jaccard_loss_partials(B, HW) entries and carries the cross-entropy alone.
 * No atomics: two runs are bit-identical.  At most 65535 images of at most 2^30 pixels, 2^31 - 1 pixels in all (-1). */
int dl3_jaccard_partials(int B, int HW);
int dl3_jaccard_loss_partials(int B, int HW);
int dl3_jaccard_sums_plain(const float *logits, const float *labels, const float *weights, double *partials, int B, int HW,
                           int C, void *stream);
int dl3_jaccard_sums_bilinear(const float *logits_lo, const float *labels, const float *weights, double *partials, int N,
                              int Hi, int Wi, int Ho, int Wo, int C, void *stream);
int dl3_jaccard_coef(const double *partials, int P, int B, int C, float lambda, double *sums, float *coef, double *stats,
                     float *loss_row, void *stream);
int dl3_softmax_xent_jaccard(const float *logits, const float *labels, const float *weights, const float *nnz,
                             const float *coef, float lambda, float *dlogits, float *loss_partial, int B, int HW, int C,
                             void *stream);
int dl3_upsample_softmax_xent_jaccard(const float *logits_lo, const float *labels, const float *weights, const float *nnz,
                                      const float *coef, float lambda, float *dlogits, float *loss_partial, int N, int Hi,
                                      int Wi, int Ho, int Wo, int C, void *stream);
/* ---- focal loss in every form of the training loss tail (csrc/losstail.hip; Lin et al. 2017 eq. 5 in softmax
 * form, our own statement).  Inputs as the four loss kernels above take them (label outside 0..C-1: void; weights
 * nullable: w = 1, forced to 0 on void pixels; *nnz floored as there), plus
 *   alpha  device pointer to C floats >= 0, or NULL (every class 1); read once per workgroup into LDS
 *   gamma  >= 0 and finite, a launch argument (-1 otherwise, nothing is written)
 * With p = softmax(z), q = clip(p_t / sum_c p_c, 1e-7f, 1 - 1e-7f) and inside = (the unclipped quotient lies in that
 * interval), per pixel
 *   l = alpha[t] (1 - q)^gamma (-log q);   loss = sum_m w l / nnz
 *   dlogits[m,k] = (w / nnz) inside alpha[t] mu (p_k - [k = t]),  mu = (1 - q)^gamma + gamma q (1 - q)^(gamma-1) (-log q)
 * 1 - q is formed without cancellation (above one half: the renormalised sum of the other classes' probabilities) and
 * clipped to [1 - (1 - 1e-7f), 1 - 1e-7f], the interval 1 - q has while q is in its own.  gamma = 0 with alpha NULL (or all ones) is the cross-entropy: the gradient of each
 * entry point is then its counterpart's bit for bit.  Each entry point keeps its counterpart's grid, loss partials
 * (dl3_rows_partials, dl3_xent_fold_partials, dl3_shuffle_xent_partials), layouts and summation order; none writes probs.
 * C <= 32 (-4 above).  The fold form needs (Wo + 2*Wi)*C*4 + 8*Wo + 128 <= 64 KB of LDS (the row, its source rows, the
 * lerp table and alpha).  No atomics: two runs are bit-identical. */
int dl3_focal_xent(const float *logits, const float *labels, const float *weights, const float *nnz, const float *alpha,
                   float gamma, float *dlogits, float *loss_partial, int M, int C, void *stream);
int dl3_upsample_focal_xent(const float *logits_lo, const float *labels, const float *weights, const float *nnz,
                            const float *alpha, float gamma, float *dlogits, float *loss_partial, int N, int Hi, int Wi,
                            int Ho, int Wo, int C, void *stream);
int dl3_upsample_focal_xent_fold(const float *logits_lo, const float *labels, const float *weights, const float *nnz,
                                 const float *alpha, float gamma, float *dlogits_xfold, float *loss_partial, int N, int Hi,
                                 int Wi, int Ho, int Wo, int C, void *stream);
int dl3_shuffle_focal_xent(const float *u, const float *labels, const float *weights, const float *nnz, const float *alpha,
                           float gamma, float *du, float *loss_partial, int N, int H, int W, int C, int r, void *stream);
/* out[i] = sum_p partial[p][i]  (fixed order) */
int dl3_reduce_partials(const float *partial, int P, int n, float *out, void *stream);
/* m folds in one launch, each bit-identical to its own dl3_reduce_partials call.  desc (device, int64 [m][5]): partial
 * pointer, out pointer, P, n, index of the fold's first workgroup; folds in ascending first-workgroup order; a fold takes
 * dl3_reduce_partials_blocks(P, n) workgroups and total_blocks is their sum.  (All weight-gradient slab folds of a
 * backward pass: 55 launches less per step for MobileNetV2.) */
int dl3_reduce_partials_blocks(int P, int n);
int dl3_reduce_partials_batched(const long long *desc, int m, int total_blocks, void *stream);
int dl3_fill(float *p, float value, size_t n, void *stream);
/* p[i] *= value (the data-parallel loss normaliser: count_all(w != 0) summed over ranks on the stream, then / world) */
int dl3_scale(float *p, float value, size_t n, void *stream);
/* Keras Adam with decay (notebook cell 2): lr_t is computed on the host;
 * g is first multiplied by grad_scale (1/world_size after the RCCL sum) */
int dl3_adam_step(float *p, const float *g, float *m, float *v, size_t n, float lr_t, float beta1, float beta2,
                  float eps, float grad_scale, void *stream);
/* the same with the scale finished on the device: g is multiplied by grad_scale / max(denom[0], 1e-20).  Data-parallel
 * step without a host round trip (round 5; utils.py:209-211 merges the towers and evaluates ONE loss over the global
 * batch): every rank differentiates sum_shard(l*w) / c0 with a FIXED c0, its count(w != 0) and loss sum ride behind the
 * gradients in the same all-reduce, denom = the summed count, grad_scale = c0. */
int dl3_adam_step_norm(float *p, const float *g, float *m, float *v, size_t n, float lr_t, float beta1, float beta2,
                       float eps, float grad_scale, const float *denom, void *stream);

/* ---- the optimizer step beyond plain Adam --------------------------------------------------------------
 * [TF-semantics: Keras 2.2.4 keras/optimizers.py, restated from memory.]
 * dl3_grad_sumsq: out[0] (double, device) = sum of g[i]^2 over [0, n).  Two launches: per-workgroup partial sums
 * accumulated in double into `workspace` (dl3_grad_sumsq_workspace_bytes(n), 8-byte aligned), then ONE workgroup folds
 * them in a fixed order — no float atomics, bit-reproducible from run to run.  16-byte loads where g is 16-byte aligned.
 * -3 (DL3_EWORKSPACE) on a short workspace. */
size_t dl3_grad_sumsq_workspace_bytes(size_t n);
int dl3_grad_sumsq(const float *g, size_t n, double *out, void *workspace, size_t workspace_bytes, void *stream);
/* dl3_opt_step: ONE launch over [0, n).  The effective gradient (Optimizer.get_gradients), built on the device:
 *   sc = grad_scale / max(denom[0], 1e-20) when denom is given (dl3_adam_step_norm's semantics), else grad_scale
 *   clipnorm > 0: norm = sc * sqrt(sumsq[0]) (sumsq: the result of dl3_grad_sumsq over the SAME g — the GLOBAL norm);
 *                 g' = g * sc * (clipnorm / norm) when norm >= clipnorm, else g * sc
 *   clipvalue > 0: g' clamped to [-clipvalue, clipvalue]
 * and the rule (lr_t from the host: lr / (1 + decay * iterations), for Adam times the bias correction):
 *   DL3_OPT_SGD     c0 = momentum: v = c0*s0 - lr_t*g'; s0 <- v; p += v, or with nesterov p += c0*v - lr_t*g'
 *   DL3_OPT_RMSPROP c0 = rho:      s0 <- c0*s0 + (1-c0)*g'^2; p -= lr_t*g' / (sqrt(s0) + eps)
 *   DL3_OPT_ADAM    c0, c1 = beta_1, beta_2; s0 = m, s1 = v: dl3_adam_step's arithmetic on g'
 * s1 may be NULL for the one-slot rules.  fp32 throughout; nothing is read back to the host. */
#define DL3_OPT_SGD 0
#define DL3_OPT_RMSPROP 1
#define DL3_OPT_ADAM 2
typedef struct {
  float lr_t, c0, c1, eps, grad_scale, clipnorm, clipvalue; /* clipnorm / clipvalue: 0 = off */
  int nesterov;
} dl3_opt_hyper;
int dl3_opt_step(float *p, const float *g, float *s0, float *s1, size_t n, int rule, const dl3_opt_hyper *hyper,
                 const float *denom, const double *sumsq, void *stream);

/* ---- L2 weight regularisers: Keras kernel_regularizer=l2(l) over a flat arena ---------------------------
 * [TF-semantics: Keras 2.2.4 keras/regularizers.py and the total loss of keras/engine/training.py, restated from memory:
 * l2(l) on a weight w adds l * sum(w^2) to the loss, gradient 2*l*w.]
 * The regularised part of the arena p is a table of S runs, built on the host and resident on the device (trusted here;
 * the host builder validates it — dl3_reduce_partials_batched's desc is the precedent):
 *   runs (int64 [S][3]): first element, length (>= 1), first tile — runs ascend and are disjoint; a TILE is up to 1024
 *        consecutive elements of ONE run, a run of `length` has ceil(length / 1024) of them, `first tile` is the prefix
 *        sum of the tile counts in front of the run and `tiles` the total
 *   coef (float [S]): l >= 0, finite
 * out (double [2], device): out[0] = sum_s coef[s] * sum_{i in run s} p[i]^2 — squares and sums in double ((double)w *
 *   (double)w is exact); every workgroup writes ONE double partial into `workspace` (dl3_l2_penalty_workspace_bytes(tiles),
 *   8-byte aligned) and ONE workgroup folds them in ascending order: no float atomics, two runs give the same 64 bits;
 *   which element goes to which lane depends on the table and the grid rule (workgroup b: tiles b, b + grid, ...) only.
 *   out[1] = out[0] rounded once to float, stored as double: a float reader and a double reader agree.
 * g (nullable): g[i] += ((2 * coef[s]) * p[i]) / sc on the runs, sc = grad_scale, or grad_scale / max(denom[0], 1e-20)
 *   when denom is given — dl3_opt_step's sc, so the step's later multiplication by sc returns 2*l*w (sc == 1 divides
 *   exactly).  grad_scale must then be positive and finite.  Elements outside the runs are neither read nor written; p is
 *   never written.  16-byte loads and stores on the runs that start 16-byte aligned in 16-byte aligned p and g, element by
 *   element otherwise.
 * S == 0 (tiles == 0): out = {0, 0}; coef and the workspace are not looked at and may be NULL.  Refused before any launch,
 * nothing written: S < 0, a NULL p / out / runs, with S > 0 a NULL coef, tiles < S, out or workspace not 8-byte aligned (-1);
 * with S > 0 a short workspace (-3, DL3_EWORKSPACE). */
size_t dl3_l2_penalty_workspace_bytes(long long tiles);
int dl3_l2_penalty(const float *p, float *g, const long long *runs, const float *coef, int S, long long tiles,
                   float grad_scale, const float *denom, double *out, void *workspace, size_t workspace_bytes,
                   void *stream);

/* ---- either side of the network: targets in, metric counts out -------------------------- */
#define DL3_LABEL_U8 0  /* cv2.imread(path, 0) label maps (utils.py:314) */
#define DL3_LABEL_I32 1 /* label.astype('int32') (utils.py:371) */
/* Tensor contract of SegmentationGenerator.__getitem__ (utils.py:375-402) from raw label maps labels[B][HW]:
 *   y = label, values > C-1 (and negative ones) -> C ("void")            utils.py:377
 *   Y[B][HW]  (nullable) = y as float (the [B,HW,1] target of train_on_batch)   utils.py:379
 *   SW[B][HW] (nullable) = per-image 'balanced' class weight n_valid / (n_present * count[y]) evaluated in double and
 *                          rounded to float; 0 on void pixels                  utils.py:391-400
 *   hist[B][C+1] (required, int32) = per-image label histogram (bin C = void), also the scratch of the op.
 * C <= 255.  Integer counting with int atomics: results are exact and run-to-run identical. */
int dl3_prepare_targets(const void *labels, int label_dtype, int B, int HW, int C, float *Y, float *SW, int *hist,
                        void *stream);
/* Pixel counts behind Jaccard / sparse_accuracy_ignoring_last_label (utils.py:132-157), per image b and class c:
 *   counts[b][0][c] = #(y_true == c), counts[b][1][c] = #(pred == c), counts[b][2][c] = #(y_true == c && pred == c)
 * pred = dl3_argmax output (int32), y_true as fed to the loss (float, void = C).  The ratios stay on the host
 * (utils.Jaccard_from_counts): union = true + pred - inter, exactly the reference's inter/union sums. */
int dl3_seg_counts(const int *pred, const float *y_true, int B, int HW, int C, int *counts, void *stream);

/* ---- evaluation tail (Model.evaluate / validation): loss sums, metric counts, confusion matrix and the
 * argmax mask from the LOW-resolution logits and the labels in one pass — neither full-resolution logits nor
 * probabilities are written.  Three input forms:
 *   bilinear  logits_lo [N][Hi][Wi][C], labels / weights [N][Ho][Wo]: the TF1 legacy bilinear resize applied in registers,
 *             bit-identical to dl3_resize_bilinear_fwd (so the mask equals dl3_resize_bilinear_fwd + dl3_argmax); the loss
 *             interpolates with TF's stated weight fl(o * scale) - lo (the resize kernel fuses that into one fma);
 *   shuffle   u [N][H][W][C*r*r] (the Subpixel convolution's output), labels / weights [N][H*r][W*r]: dl3_phase_shift by index;
 *   plain     materialised logits [N*HW][C], C <= 255.
 * The fused forms need C <= 32; their *_partials query returns 0 for a shape they do not support (fall back to
 * dl3_resize_bilinear_fwd / dl3_phase_shift followed by the plain form).  labels: float, void = C (as fed to the loss);
 * weights nullable (w = 1).  Outputs, per call:
 *   loss_sum[N]   (double) per image sum_m w[m] * l[m], l the per-pixel expression of dl3_softmax_xent (softmax, Keras'
 *                 renormalise, clip to [1e-7, 1-1e-7], void -> 0), the fp32 terms added in double: per-workgroup partials[N][P] (double),
 *                 P = dl3_eval_tail_*_partials(...), folded per image in a fixed order in double by a second launch — no
 *                 float atomics, two runs are bit-identical;
 *   nnz[N]        (int32) count(w != 0) per image;
 *   counts[N][3][C] (int32) exactly dl3_seg_counts' contract;
 *   confusion[C][C] (int64, nullable) += #(label == row && prediction == column), void labels skipped: it ACCUMULATES
 *                 across calls (a whole validation pass needs no host trip); the caller zeroes it;
 *   mask[N][Ho][Wo] (int32, nullable) argmax, first maximum wins like dl3_argmax.
 * Integer outputs go through a per-workgroup LDS histogram and one global integer atomic per non-zero bin: exact and
 * independent of arrival order. */
int dl3_eval_tail_bilinear_partials(int N, int Hi, int Wi, int Ho, int Wo, int C);
int dl3_eval_tail_bilinear(const float *logits_lo, const float *labels, const float *weights, double *partials,
                           double *loss_sum, int *nnz, int *counts, long long *confusion, int *mask, int N, int Hi, int Wi,
                           int Ho, int Wo, int C, void *stream);
int dl3_eval_tail_shuffle_partials(int N, int H, int W, int C, int r);
int dl3_eval_tail_shuffle(const float *u, const float *labels, const float *weights, double *partials, double *loss_sum,
                          int *nnz, int *counts, long long *confusion, int *mask, int N, int H, int W, int C, int r,
                          void *stream);
int dl3_eval_tail_plain_partials(int N, int HW, int C);
int dl3_eval_tail_plain(const float *logits, const float *labels, const float *weights, double *partials, double *loss_sum,
                        int *nnz, int *counts, long long *confusion, int *mask, int N, int HW, int C, void *stream);

/* ---- training augmentation (SegmentationGenerator.__getitem__, utils.py:310-369) ------------------------------------
 * images[B][Hs][Ws][3] uint8 (BGR) and labels[B][Hs][Ws] (label_dtype) -> X[B][H][W][3] float32 (the engine's input) and
 * labels_out[B][H][W] (label_dtype; with DL3_AUG_WARP uint8, values the interpolation created set to C = void).
 * Per image, in the reference's order: [blur 5x5] -> crop at (x, y) -> [hflip] -> [vflip] -> gamma LUT -> [warpAffine]
 * -> [CLAHE on Y of YUV].  Every floating-point decision is taken on the host (augment.py) and arrives as tables:
 *   img_params[B][8] = {blur_on, crop_x, crop_y, hflip, vflip, 0, 0, 0};  lut[B][256] (identity without brightness)
 *   warp_tab[B][2W + 2H] = adelta[W], bdelta[W], X0[H], Y0[H] (cv2 fixed point, +16 rounding in X0 / Y0; identity
 *                          tables when only DL3_AUG_CLAHE is set)
 *   clahe_i[2W + 2H] = (tx1, tx2) per x then (ty1, ty2) per y;  clahe_f[2W + 2H] = (xa, 1-xa) per x, (ya, 1-ya) per y
 * Without DL3_AUG_WARP / DL3_AUG_CLAHE stage 1 writes X directly.  The warp takes uint8 labels only (-4 otherwise);
 * H >= 3, W >= 3, H <= Hs, W <= Ws, C <= 255 with the warp (-1 otherwise); CLAHE needs H, W >= 16 (-4).
 * Integer atomics only. */
#define DL3_AUG_WARP 1
#define DL3_AUG_CLAHE 2
size_t dl3_augment_workspace_bytes(int B, int H, int W, int flags);
int dl3_augment(const void *images, const void *labels, int label_dtype, int B, int Hs, int Ws, int H, int W, int flags,
                const int *img_params, const int *lut, const int *warp_tab, const int *clahe_i, const float *clahe_f,
                int C, float *X, void *labels_out, void *workspace, size_t workspace_bytes, void *stream);
/* dl3_augment with the label sets handed in: present[B][8], bit v of image b set when label value v occurs in its map
 * BEFORE any resize (dl3_cv_resize writes them from the source-size maps; the reference takes np.unique(label) there,
 * utils.py:317).  dl3_augment derives the same sets from its own `labels`.  Everything else is dl3_augment's contract. */
int dl3_augment_present(const void *images, const void *labels, int label_dtype, int B, int Hs, int Ws, int H, int W,
                        int flags, const int *img_params, const int *lut, const int *warp_tab, const int *clahe_i,
                        const float *clahe_f, int C, const int *present, float *X, void *labels_out, void *workspace,
                        size_t workspace_bytes, void *stream);

/* ---- cv2.resize in front of the augmentation (utils.py:322-324, :421-422): a ragged batch -> the uniform one -------------
 * B decoded images of DIFFERENT sizes lie back to back in image_pool (uint8, BGR, [Hs][Ws][3] each), their label maps in
 * label_pool (label_dtype, [Hs][Ws] each).  Per image, in the reference's order: [blur 5x5 at the source size, reflect-101
 * at the image's own borders] -> mode 0: cv2.resize to H x W (INTER_LINEAR for the image: 11-bit coefficients and cv2's
 * two-pass integer rounding; INTER_NEAREST for the label map) | mode 1: the H x W crop at (crop_x, crop_y).  Outputs:
 *   images_out[B][H][W][3] uint8, labels_out[B][H][W] (label_dtype): the input of dl3_augment / dl3_augment_present
 *   present[B][8] (nullable): the 256-bit set of label values of each SOURCE-size map (int32 values outside 0..255 set
 *                 nothing); zeroed here
 * Either pool may be NULL together with its output (images only, or maps only).  Tables, int32, in device memory:
 *   desc[B][12] = {image offset (bytes into image_pool), label offset (elements into label_pool), Hs, Ws, blur_on, mode,
 *                  crop_x, crop_y, table offset (ints into tab), 0, 0, 0}
 *   tab: per distinct source size 4W + 4H ints: xs[W], xa0[W], xa1[W], xn[W], ys[H], yb0[H], yb1[H], yn[H] — the first
 *        source column (clamped to 0..Ws-1) and its two coefficients (sum 2048), the nearest column; the first source row
 *        as floor() left it (the device clamps both taps) and its coefficients, the nearest row.  Mode-1 images read none.
 * The host takes every floating-point decision (augment.resize_tables); the device does integer arithmetic only.
 * THE DEVICE TRUSTS desc AND tab: the caller (augment.front_tables) checks that every image and map lies inside its pool,
 * every crop inside its image and every table index inside its source before the upload.  max_hs / max_ws: the largest
 * Hs / Ws of the batch (they size the grids of the blur and the label-set pass).  blur_any: some desc has blur_on — the
 * blurred copies go to `workspace` (dl3_cv_resize_workspace_bytes(image_pool_bytes, 1); nothing is needed without blur).
 * One launch per stage for the whole batch.  -1 for sizes below 1, a missing output or a short workspace; -4 for a label
 * dtype other than DL3_LABEL_U8 / DL3_LABEL_I32.  Integer atomics only. */
size_t dl3_cv_resize_workspace_bytes(size_t image_pool_bytes, int blur_any);
int dl3_cv_resize(const unsigned char *image_pool, size_t image_pool_bytes, const void *label_pool, int label_dtype, int B,
                  int max_hs, int max_ws, int H, int W, int blur_any, const int *desc, const int *tab, void *images_out,
                  void *labels_out, int *present, void *workspace, size_t workspace_bytes, void *stream);

/* ---- dense-CRF post-processing (do_crf, utils.py:74-91): exact mean-field inference, DESIGN.md §9 -----------------------
 * The model the reference configures in pydensecrf — unary from labels, a Gaussian position kernel and a bilateral
 * position + colour kernel, both with symmetric normalisation, Potts compatibility — evaluated over ALL pixel pairs
 * (no permutohedral lattice).  fp32, fixed summation order, no float atomics; L <= 32 labels (-4 above).
 * One workspace serves both launches: dl3_crf_workspace_bytes(B, H, W, L) (for dl3_crf_message: H * W >= N); 16-byte
 * aligned.
 * dl3_crf_message: one un-normalised pass out[b][i][l] = sum_j exp(-|f_i - f_j|^2 / 2) * Qin[b][j][l] (the j = i term
 *   included) over features feat[B][N][D], D <= 6 (-4 above); Qin and out are [B][N][L].
 * dl3_crf_inference: im[B][H][W][3] uint8, U[B][L][N] unary energies (N = H*W, pixel i = y*W + x),
 *   params = {sx, sy, w_gauss, sxy, srgb, w_bilateral}, six floats in HOST memory read before the call returns;  features g_i = (x/sx, y/sy), b_i = (x/sxy, y/sxy, c/srgb),
 *   k_ij = exp(-|f_i - f_j|^2 / 2), n_i = 1/sqrt(sum_j k_ij + 1e-20), M(Q)_i = n_i sum_j k_ij n_j Q_j;
 *   Q = softmax(-U); iters times Q = softmax(-U + w_gauss M_g(Q) + w_bilateral M_b(Q)).  Outputs, each nullable:
 *   Q[B][L][N], energy[B][L][N] (the last update's pre-softmax values), map[B][N] (int32 argmax, first maximum). */
size_t dl3_crf_workspace_bytes(int B, int H, int W, int L);
int dl3_crf_message(const float *feat, int D, const float *Qin, int B, int N, int L, float *out, void *ws,
                    size_t ws_bytes, void *stream);
int dl3_crf_inference(const unsigned char *im, const float *U, int B, int H, int W, int L, const float *params,
                      int iters, float *Q, float *energy, int *map, void *ws, size_t ws_bytes, void *stream);

/* ---- the dense CRF's unary energies from the network's class scores ("softmax unary") ----------------
 * pydensecrf.utils.unary_from_softmax(sm, scale=None, clip=1e-5) [pydensecrf-semantics] on the device, per pixel:
 *   p = softmax(scores) over the classes (plain form with is_prob = 1: p = x as given);
 *   scale > 0: p = scale * p + (1 - scale) / C   (scale <= 0 stands for None);
 *   clip  > 0: p = min(max(p, clip), 1)          (clip <= 0 stands for None);
 *   U = -log p, written as the planar U[B][C][N] that dl3_crf_inference reads (the MAP index is then the class id).
 * Three input forms, the ones of dl3_eval_tail_*:
 *   plain     x [B][N][C]: materialised logits, or probabilities (is_prob = 1);
 *   bilinear  logits_lo [B][Hi][Wi][C], N = Ho * Wo: the TF1 legacy bilinear resize applied in registers, the interpolated
 *             logits bit-identical to dl3_resize_bilinear_fwd;
 *   shuffle   u [B][H][W][C*r*r] (the Subpixel convolution's output), N = H*r * W*r: dl3_phase_shift by index.
 * scale and clip cross this boundary as floats: a value that float cannot hold exactly (0.3, 1e-5) is applied as its
 * float rounding, a relative difference of up to 6e-8 in the mixing weight or the clip level from the same number held
 * as a double.  scale > 1 (the uniform part would turn negative) and clip >= 1 (every energy would be 0) are refused (-1).
 * C <= 32, the limit of dl3_crf_inference (-4 above).  subtract-max, expf and the sum in fp32; quotient, scale, clip and
 * logarithm in double, rounded once.  No atomics: two runs are bit-identical.  The arg-min of U over the classes is the
 * first-maximum argmax of the scores (dl3_argmax) wherever it is unique. */
int dl3_crf_unary_plain(const float *x, int is_prob, float *U, int B, int N, int C, float scale, float clip, void *stream);
int dl3_crf_unary_bilinear(const float *logits_lo, float *U, int B, int Hi, int Wi, int Ho, int Wo, int C, float scale,
                           float clip, void *stream);
int dl3_crf_unary_shuffle(const float *u, float *U, int B, int H, int W, int C, int r, float scale, float clip,
                          void *stream);

/* ---- multi-scale and flip inference (Model.predict_multiscale) [deeplab-semantics] ---------------------
 * Both launches are the align_corners = True bilinear resize, every operation a separately rounded fp32 operation in this
 * order (no fused multiply-add), per axis with input extent `in` and output extent `out`:
 *   scale = fl((in - 1) / (out - 1)), 0 where out == 1;  f = fl(o * scale);  lo = min(int(f), in - 1);
 *   hi = min(lo + 1, in - 1);  w = fl(f - lo);
 *   top = tl + (tr - tl) * wx;  bot = bl + (br - bl) * wx;  value = top + (bot - top) * wy.
 * dl3_tta_resize_image: raw pixels src[B][Hi][Wi][3], float32 (DL3_TTA_F32) or uint8 (DL3_TTA_U8), -> float32
 *   dst[B][Ho][Wo][3], not rounded.  flip = 1: column ox receives the value computed for column Wo - 1 - ox.
 * dl3_tta_accumulate: one pass's probabilities probs[B][Hi][Wi][C] resized to [B][Ho][Wo][C] and folded into the fp32
 *   accumulator acc[B][Ho][Wo][C] (any 4-byte alignment; 16-byte accesses between its 16-byte boundaries).  flip = 1: the
 *   pass ran on a mirrored image, source column x is read at index Wi - 1 - x.  first = 1: acc = v, and acc is NOT read;
 *   otherwise acc = acc + v.  n_passes_if_last = n > 0: the stored value is (acc + v) / n (v / n when first), a correctly
 *   rounded fp32 division; 0: not the last pass.  Any C >= 1, any extents >= 1, up- and down-scaling.  No atomics: two runs
 *   are bit-identical. */
#define DL3_TTA_F32 0
#define DL3_TTA_U8 1
int dl3_tta_resize_image(const void *src, int src_dtype, float *dst, int B, int Hi, int Wi, int Ho, int Wo, int flip,
                         void *stream);
int dl3_tta_accumulate(const float *probs, float *acc, int B, int Hi, int Wi, int Ho, int Wo, int C, int flip, int first,
                       int n_passes_if_last, void *stream);

/* ---- sliding-window inference (Model.predict_sliding) -------------------------------------------------
 * An image [Hi][Wi][3] of ANY size is cut into overlapping windows of the model's size H x W; the class probabilities of
 * the windows are averaged where they overlap.  One image per launch; the window grid is arithmetic, per axis (extent
 * `size`, window `win`, stride 1 <= s <= win):
 *   P = max(size, win);  n = ceil((P - win) / s) + 1;  window k starts at min(k s, P - win)
 * (the last window is shifted back to end on the image's edge), window index k = ky * nx + kx.  A launch handles the
 * windows k0 .. k0 + nw - 1.
 * dl3_slide_gather: window pixel (r, c) of window k = image pixel (y0 + r, x0 + c) as float32 (src float32, DL3_TTA_F32,
 *   or uint8, DL3_TTA_U8) into dst[nw][H][W][3]; rows >= Hi and columns >= Wi — an image smaller than the window — hold
 *   pad_value.
 * dl3_slide_accumulate: probs[nw][H][W][C] folded into the canvas acc[Hi][Wi][C], which the caller zeroed in front of the
 *   image's first launch (any 4-byte alignment; 16-byte accesses between its 16-byte boundaries).  Per canvas element, over
 *   the launch's windows that cover its pixel in ascending k:  t = fl(w p);  acc = fl(acc + t), every operation a
 *   separately rounded fp32 operation (no fused multiply-add).  blend DL3_SLIDE_UNIFORM: w = 1; DL3_SLIDE_PYRAMID:
 *   w = fl(float(min(r + 1, H - r)) * float(min(c + 1, W - c))) at window pixel (r, c).  Probabilities at pad positions
 *   are not read.  Cutting one window sequence into launches differently gives the same bits.  A launch reads and writes
 *   only canvas pixels inside its own windows.  wsum (nullable) [Hi][Wi], zeroed like acc: ws = fl(ws + w) in the same
 *   order; NULL: dl3_slide_finalize recomputes it from the geometry, to the same bits.
 * dl3_slide_finalize: prob = fl(acc / ws), a correctly rounded fp32 division, into probs_out[Hi][Wi][C] (nullable; may
 *   be acc itself), and mask_out[Hi][Wi] (int32, nullable) = the first maximum of these prob values (dl3_argmax's rule).
 *   Not both NULL.  wsum NULL: ws is the weight sum of ALL the grid's windows over the pixel, in ascending k.
 * Any C >= 1, any extents >= 1.  No allocation, no synchronisation, no atomics: capturable, two runs are bit-identical.
 * -1 for: a stride outside [1, window], k0 + nw beyond the grid, nw < 1, an unknown blend or dtype, both outputs NULL, or
 * extents beyond the kernels' 32-bit pixel indices (Hi Wi, nw H W, Wi C < 2^31; C <= 65536). */
#define DL3_SLIDE_UNIFORM 0
#define DL3_SLIDE_PYRAMID 1
int dl3_slide_gather(const void *src, int src_dtype, int Hi, int Wi, int H, int W, int sh, int sw, int k0, int nw,
                     float pad_value, float *dst, void *stream);
int dl3_slide_accumulate(const float *probs, float *acc, float *wsum, int Hi, int Wi, int H, int W, int C, int sh, int sw,
                         int k0, int nw, int blend, void *stream);
int dl3_slide_finalize(const float *acc, const float *wsum, float *probs_out, int *mask_out, int Hi, int Wi, int H, int W,
                       int C, int sh, int sw, int blend, void *stream);

/* ---- trimap evaluation (Model.confusion_matrix_trimap): confusion matrices restricted to bands around the
 * object boundaries — the trimap experiment of the DeepLabV3+ paper, restated with a definition of its own.
 * labels[B][H][W]: float, 0..C-1 or void (C; every value outside 0..C-1 is read as void), as fed to the loss.
 * Seeds of an image (a bit mask): DL3_TRIMAP_SEED_VOID — the pixel is void; DL3_TRIMAP_SEED_EDGES — some 4-neighbour inside
 *   the same image has another label value (void counts as a value; both sides of an edge are seeds).  Images never see
 *   each other's pixels and nothing wraps at an image border.
 * dl3_trimap_rings: rings[b][y][x] (uint8, any alignment) = the smallest integer w >= 0 such that a seed of image b lies
 *   within distance w, clamped to wmax + 1 ("beyond"; an image without seeds is wmax + 1 everywhere).
 *   DL3_TRIMAP_CHEBYSHEV: distance max(|dy|, |dx|) — the (2w+1)^2 square dilation; DL3_TRIMAP_EUCLIDEAN: the smallest r
 *   with r^2 >= min(dy^2 + dx^2), decided in integers.  workspace: dl3_trimap_workspace_bytes(B, H, W) bytes (0 for sizes
 *   the kernels refuse), 4-byte aligned, fully overwritten.
 * dl3_trimap_confusion: band[K+1][C][C] (int64) += 1 at [bin][t][p] for every pixel with a legal label t and a prediction
 *   pred[b][y][x] = p in 0..C-1 (every other pixel is skipped, dl3_eval_tail_*'s confusion rule); bin = the first k with
 *   ring <= widths[k], else K.  The bins are disjoint; their running sum over k is the confusion matrix of the band of
 *   width widths[k], and the sum of all K + 1 the whole-image matrix.  band ACCUMULATES across calls; the caller zeroes it.
 *   widths: a HOST pointer to K strictly increasing widths >= 1, read during the call (they go by value into the launch);
 *   rings: dl3_trimap_rings' output for wmax >= widths[K-1].
 * Limits: 1 <= wmax <= 254, 1 <= K <= 8, widths <= 254, 1 <= C <= 255, B, H, W >= 1, B*H*W < 2^31.  -1, and nothing is
 * written, for a limit broken, widths not strictly increasing or < 1, an unknown metric, a seed mask outside 1..3, a null
 * pointer or a misaligned workspace.  No allocation, no synchronisation: capturable; the only atomics are integer ones, so
 * two runs are bit-identical. */
#define DL3_TRIMAP_CHEBYSHEV 0
#define DL3_TRIMAP_EUCLIDEAN 1
#define DL3_TRIMAP_SEED_VOID 1
#define DL3_TRIMAP_SEED_EDGES 2
size_t dl3_trimap_workspace_bytes(int B, int H, int W);
int dl3_trimap_rings(const float *labels, unsigned char *rings, void *workspace, int B, int H, int W, int C,
                     int wmax, int metric, int seeds, void *stream);
int dl3_trimap_confusion(const int *pred, const float *labels, const unsigned char *rings, long long *band,
                         int B, int H, int W, int C, const int *widths, int K, void *stream);

/* ---- data-parallel gradient exchange over RCCL / xGMI (replaces keras.utils.multi_gpu_model, utils.py:209-211) ----
 * One process per GPU.  Rank 0 draws a 128-byte id (dl3_comm_unique_id) and hands it to the other ranks over any host
 * channel; every rank then calls dl3_comm_init with its HIP device current.  The collectives are enqueued on the
 * caller's stream (no sync): ONE all-reduce(sum) of the flat fp32 gradient arena per step, the 1/world factor goes
 * into dl3_adam_step(grad_scale).  RCCL is bound with dlopen at the first call: -4 (DL3_EUNSUPPORTED) if absent. */
#define DL3_COMM_ID_BYTES 128
int dl3_comm_unique_id(void *id128);
int dl3_comm_init(void **comm, const void *id128, int rank, int world);
int dl3_comm_allreduce_f32(void *comm, const float *send, float *recv, size_t n, void *stream);
int dl3_comm_broadcast_f32(void *comm, float *buf, size_t n, int root, void *stream);
/* number of ranks RCCL itself reports for the communicator (ncclCommCount): lets a benchmark line state which data
 * plane produced it */
int dl3_comm_count(void *comm, int *count);
int dl3_comm_destroy(void *comm);

#ifdef __cplusplus
}
#endif
#endif

/*
 * yolo3hip.h -- C ABI of libyolo3hip.so, the MI355X (gfx950) hot path of the
 * YOLOv3 train / inference pipeline of usnistgov/object-detection-yolov3.
 *
 * The reference has no FFI of its own: its hot path is TensorFlow ops called
 * from Python (model.py) plus NumPy post-processing (bbox_utils.py).  Each
 * entry point below names the reference call site (file:line under the
 * reference checkout) whose arithmetic it replaces.  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers + sizes; every pointer is DEVICE memory unless it says host
 *   - activations are NHWC fp32 with an explicit row pitch `ld` (floats per
 *     pixel, >= channels) so producers can write straight into concat buffers
 *   - conv kernels are Keras layout [kh][kw][Cin][Cout] (= [tap][Cin][Cout])
 *   - all work is enqueued on `stream` (a hipStream_t) and returns at once
 *   - return 0 on success, negative Y3_E* on error; y3_last_error() = message
 *   - no entry point allocates, frees or synchronises (graph-capture safe)
 */
#ifndef YOLO3HIP_H
#define YOLO3HIP_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y3_OK 0
#define Y3_EINVAL (-1)   /* bad argument / unsupported shape */
#define Y3_ELAUNCH (-2)  /* HIP launch error */

typedef void* y3_stream_t; /* hipStream_t */

const char* y3_last_error(void);
/* Diagnostics: x / d computed the way the kernels' index decode does it (multiply-high + shift, common.h y3_make_div),
 * on the host; 0 <= x < 2^31, d >= 1.  The CPU tests compare it with the integer division it replaces. */
int y3_debug_div(int x, int d);
int y3_version(void);

/* ---- epilogue flags of y3_conv2d_fwd / y3_conv2d_dgrad ------------------ */
#define Y3_EPI_LRELU 1u  /* v = v > 0 ? v : alpha*v   (tf.nn.leaky_relu, model.py:34) */
#define Y3_EPI_ACCUM 2u  /* dst += v instead of dst = v */
/* Arithmetic selector of y3_conv2d_fwd / y3_conv2d_dgrad / y3_conv2d_dgrad_bn (conv_x3.hip).  Without it the contraction runs on
 * v_mfma_f32_32x32x2_f32 (exact fp32 fmaf chain).  With it every operand element is cut into three bf16 pieces that sum to it
 * exactly (8 + 8 + 8 significant bits, round to nearest), the six piece pairs that carry more than 2^-26 of a product go through
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation: fp32-class results (not bit-identical to the fmaf chain; tests/test_gpu_kernels.py
 * bounds the error against fp64 by that of the fp32 instruction) at 2.67x fewer matrix-pipe cycles.  THE WEIGHT OPERAND CHANGES
 * with the flag: the kernel needs K contiguous per output column AND the weights already split, so `wt` / `wt_t` then point at the
 * THREE bf16 PLANES y3_x3_split_weights() makes of the copy with that layout -- y3_conv2d_fwd: of [tap][Cout][Cin] (what
 * y3_transpose_weights writes), y3_conv2d_dgrad*: of [tap][Cin][Cout] (the Keras kernel); each entry point the copy the OTHER one
 * takes without the flag.  (The activations are split inside the kernels.)  Shapes: y3_conv2d_x3_ok() / y3_conv2d_dgrad_x3_ok().
 * Everything else -- epilogue, statistics, split-K workspace contract -- is unchanged; ask the *_x queries for tile
 * counts and workspace sizes.  y3_conv2d_wgrad_x takes the same flag (both its operands are activations: no planes involved). */
#define Y3_CONV_X3 4u
/* The weight operand of the Y3_CONV_X3 forward / data-gradient kernels.  w: a kernel with K contiguous per row, [taps][rows][k_per_row]
 * fp32 (forward: rows = Cout, k_per_row = Cin, i.e. what y3_transpose_weights writes; data gradient: rows = Cin, k_per_row = Cout,
 * the Keras kernel); k_per_row a multiple of 16.  planes (bf16, 3 * taps * rows * k_per_row elements, 16-byte aligned):
 *     planes[(((tap * k_per_row/16 + c/16) * rows + row) * 3 + piece) * 16 + c % 16] = piece `piece` of w[tap][row][c],
 * w = piece 0 + piece 1 + piece 2 exactly (each the round-to-nearest bf16 of what the earlier ones leave): the block one K step of
 * the kernels reads -- rows x 3 pieces x 16 k -- is contiguous. */
int y3_x3_split_weights(const float* w, void* planes, int taps, int rows, int k_per_row, y3_stream_t stream);
/* The same for every kernel of a parameter arena in ONE launch.  table_dev: DEVICE int32 [nlayers][5] = {arena offset of the
 * layer's kernel (floats), taps, rows, k_per_row, index of the layer's first block}, blocks of 1024 elements; total_blocks = sum over
 * layers of ceil(taps * rows * k_per_row / 1024).  The planes of a layer are written at planes_arena + 3 * offset (bf16 elements). */
int y3_x3_split_weights_batched(const float* arena, void* planes_arena, const int* table_dev, int nlayers, int total_blocks, y3_stream_t stream);
/* y3_transpose_weights_batched and the two y3_x3_split_weights_batched launches of an optimiser step in ONE pass over the arena:
 * params_t <- the transposed kernels, planes <- piece planes of the Keras copy, planes_t <- piece planes of the transposed copy
 * (each for the layers whose K per row is a multiple of 16; layouts as above, a layer's planes at 3 x its arena offset).
 * table_dev / nlayers / total_tiles: as for y3_transpose_weights_batched.  Bit-identical to the three launches it replaces. */
int y3_x3_prepare_weights_batched(const float* params, float* params_t, void* planes, void* planes_t, const int* table_dev, int nlayers,
                                  int total_tiles, y3_stream_t stream);

/*
 * Tensor view: NHWC, `ld` floats between consecutive pixels.
 */
typedef struct y3_tensor {
    float* ptr;
    int n, h, w, c;
    int ld;
} y3_tensor;

/*
 * conv_layer forward (model.py:29-39 Conv2D part, :108-120 detection_layer).
 *   dst = epi( conv_SAME(src, wt) + bias )
 * epi: optional leaky-relu, then optional per-channel affine v*scale+shift
 * (inference-mode BatchNorm folded), then optional residual add (model.py:47).
 * If `stats` != NULL the kernel also writes per-row-tile partial sums of the
 * post-activation value: stats[tile][0][c] = sum, stats[tile][1][c] = sum of
 * squares (training-mode BatchNorm statistics, model.py:38); the number of
 * tiles is y3_conv2d_stats_tiles().
 * TF 'same' padding (pad_before = pad_total/2, extra at the end).
 */
int y3_conv2d_fwd(const y3_tensor* src, const float* wt, const float* bias, int ksize, int stride,
                  const y3_tensor* dst, unsigned flags, float alpha,
                  const float* scale, const float* shift, const y3_tensor* resid,
                  float* stats, void* workspace, size_t workspace_bytes, y3_stream_t stream);
/* m = output pixels (N*OH*OW).  Launches whose tile count does not fill the 256 CUs evenly are split along K (all
 * tiles, or only the remainder round); the slices park raw partial sums in `workspace` and the slice of a tile that
 * finishes last reduces them in slice order inside the same kernel (bit-reproducible; no second launch).
 * WORKSPACE CONTRACT (y3_conv2d_fwd / _dgrad / _wgrad): the first 256 KiB of a workspace are per-tile tickets.  Zero
 * the workspace once after allocating it (hipMemset, or y3_fill); every launch leaves the tickets at zero.  Launches
 * that share a workspace must be ordered on one stream.  Passing less than y3_conv2d_*_workspace() bytes disables
 * the split (forward / data gradient) or is an error (kernel gradient).  A header that is NOT zero makes the affected
 * tiles keep stale output without any error (no slice draws the last ticket); to find such a caller run with the
 * environment variable Y3_CHECK_TICKETS=1: every ticketed launch then synchronises its stream, reads the header back and
 * fails with Y3_EINVAL / y3_last_error() if a ticket is non-zero (debug aid: it serialises the stream; launches on a stream
 * under graph capture are not checked). */
int y3_conv2d_stats_tiles(int m, int cin, int ksize, int cout);
size_t y3_conv2d_fwd_workspace(int m, int cin, int ksize, int cout);
/* The same two queries for a launch with `flags` (Y3_CONV_X3 changes the tile and the split-K plan). */
int y3_conv2d_stats_tiles_x(int m, int cin, int ksize, int cout, unsigned flags);
size_t y3_conv2d_fwd_workspace_x(int m, int cin, int ksize, int cout, unsigned flags);
/* 1 if the Y3_CONV_X3 kernels take an implicit GEMM of m rows, `ntaps` taps of `c` contracted channels each and `nout` output
 * columns (forward: c = Cin, nout = Cout; stride-1 data gradient: c = Cout, nout = Cin): c a multiple of 16 (a power of two when
 * ntaps > 1), nout >= 32. */
int y3_conv2d_x3_ok(int m, int c, int ntaps, int nout);
/* 1 if y3_conv2d_dgrad / y3_conv2d_dgrad_bn take this data gradient with Y3_CONV_X3: stride 1 as y3_conv2d_x3_ok(m, Cout, ksize^2,
 * Cin); stride 2 (3x3: the merged launch of the four output-parity classes, each with its own K slices): Cin >= 64, Cout a power of
 * two >= 32.  (tape.gradient through the stride-2 convs of darknet-53, model.py:496 / :362-366.) */
int y3_conv2d_dgrad_x3_ok(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc);
/* Diagnostics (host only, no launch): the plan y3_conv2d_fwd and the stride-1 y3_conv2d_dgrad use for an implicit GEMM of
 * m x cout x (ksize^2 * cin).  out13 = {bm, bn, bk, tiles, f, s0, s1, chunk0, chunk1, grid, stats_tiles, fast, nk}: tiles
 * [0, f) are cut into s0 K slices of chunk0 K steps, tiles [f, tiles) into s1 of chunk1 (nk K steps in all); grid = work
 * items = workgroups; fast: bit 0 = the MFMA kernel with split-K takes the launch, bit 1 = x3 plan whose short last slices are
 * dealt to the blocks dispatched last (a few blocks more than workgroup slots).  Returns the workspace bytes (= y3_conv2d_fwd_workspace).  tests/planner_sweep.cpp replays the
 * kernel's item -> (tile, slice, slab, ticket) mapping from these numbers under AddressSanitizer. */
size_t y3_conv2d_plan(int m, int cin, int ksize, int cout, int* out13);
size_t y3_conv2d_plan_x(int m, int cin, int ksize, int cout, unsigned flags, int* out13);     /* the plan of a launch with `flags` (Y3_CONV_X3) */

/*
 * Gradient w.r.t. the conv input (tape.gradient, model.py:496):
 *   dsrc (+)= conv_transpose(ddst, wt)
 * wt_t is the kernel with the two channel axes swapped: [tap][Cout][Cin]
 * (y3_transpose_weights).  ddst is the gradient at the conv output (dst of
 * the forward), dsrc has the forward's src geometry.
 */
int y3_conv2d_dgrad(const y3_tensor* ddst, const float* wt_t, int ksize, int stride,
                    const y3_tensor* dsrc, unsigned flags, void* workspace, size_t workspace_bytes,
                    y3_stream_t stream);
size_t y3_conv2d_dgrad_workspace(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc);
size_t y3_conv2d_dgrad_workspace_x(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc, unsigned flags);
/*
 * y3_conv2d_dgrad whose epilogue also sums the six raw moments of (dsrc after this launch, bn_a) per output column and
 * row tile -- the statistics of the BatchNorm backward of the layer that PRODUCED dsrc's activation (bn_a = that layer's
 * lrelu(z), geometry of dsrc).  Use it for the launch that completes dsrc (the last accumulation).  Fast-path channel
 * counts only; stride 2 (3x3) only when the four parity classes go out as one merged launch: y3_conv2d_dgrad_bn_tiles()
 * returns the number of partial rows (row tiles, over all classes; partials: rows * 6 * dsrc->c floats, 16-byte aligned),
 * or 0 when the shape does not qualify.  Same workspace as y3_conv2d_dgrad.
 */
int y3_conv2d_dgrad_bn(const y3_tensor* ddst, const float* wt_t, int ksize, int stride, const y3_tensor* dsrc,
                       unsigned flags, const y3_tensor* bn_a, float* bn_partials,
                       void* workspace, size_t workspace_bytes, y3_stream_t stream);
int y3_conv2d_dgrad_bn_tiles(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc);
int y3_conv2d_dgrad_bn_tiles_x(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc, unsigned flags);
/* Diagnostics (host only, no launch; the tensors' geometry is read, their data pointers are not): how y3_conv2d_dgrad /
 * y3_conv2d_dgrad_bn send this data gradient out.  out51 = {how, classes, rows, then 12 numbers per class}:
 *   how      0 one launch (stride 1), 1 the parity classes merged into one f32 launch, 2 merged into one x3 launch, 3 one launch per
 *            parity class (stride 2 off the fast path); -1 (and 0 returned) if the geometry is refused;
 *   classes  1 (stride 1), else the parity classes that have pixels (up to 4);
 *   rows     rows of partial statistics y3_conv2d_dgrad_bn writes (= y3_conv2d_dgrad_bn_tiles_x);
 *   per class, longest contraction first as the launch orders them, at out51[3 + 12 * c]:
 *            {taps, m, bm, bn, tiles, f, s0, s1, chunk0, chunk1, nk, fast}: `taps` kernel taps reach the class, m its pixels, tiles of
 *            bm x bn; tiles [0, f) are cut into s0 K slices of chunk0 K steps, tiles [f, tiles) into s1 of chunk1, nk K steps in all
 *            (a merged launch gives one slice count to all tiles of a class: f = tiles, s1 = s0); fast as in y3_conv2d_plan_x.
 * Stride 1: class 0 carries what y3_conv2d_plan_x(m, Cout, ksize, Cin) answers.  Returns the workspace bytes the launches use at most
 * -- exact: a merged f32 launch needs none, where y3_conv2d_dgrad_workspace_x keeps answering a loose bound. */
size_t y3_conv2d_dgrad_plan_x(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc, unsigned flags, int* out51);

/*
 * Gradient w.r.t. the kernel:  dw[tap][ci][co] = sum_pixels src*ddst.
 * The pixel axis is split over workgroups.  With 2..8 splits the last split of a (k-tile, n-tile) to finish sums the
 * partial slabs in split order inside the kernel (tickets); with more splits (layers whose kernel matrix is small and
 * whose pixel count is large) every split writes a natural-layout slab and slab_reduce_kernel follows in the same call.
 * Either way the sum order is fixed (bit-reproducible).  workspace: y3_conv2d_wgrad_workspace() bytes, zeroed once
 * (contract above).
 */
int y3_conv2d_wgrad(const y3_tensor* src, const y3_tensor* ddst, int ksize, int stride,
                    float* dw, void* workspace, size_t workspace_bytes, y3_stream_t stream);
size_t y3_conv2d_wgrad_workspace(const y3_tensor* src, const y3_tensor* ddst, int ksize, int stride);
/* The same with `flags`: Y3_CONV_X3 runs the contraction over the pixels as three bf16 pieces per operand (conv_wgrad_x3_kernel:
 * both operands are activations, so both are split in the kernel; 128 x 128 tiles of the [K][Nout] gradient, fragments read with
 * ds_read_b64_tr_b16).  Same operands, layouts, workspace contract and reduction order rules as y3_conv2d_wgrad; shapes:
 * y3_conv2d_wgrad_x3_ok() (K = ksize^2 * Cin >= 128, Cout >= 128, Cin a power of two when ksize = 3). */
int y3_conv2d_wgrad_x(const y3_tensor* src, const y3_tensor* ddst, int ksize, int stride,
                      float* dw, unsigned flags, void* workspace, size_t workspace_bytes, y3_stream_t stream);
size_t y3_conv2d_wgrad_workspace_x(const y3_tensor* src, const y3_tensor* ddst, int ksize, int stride, unsigned flags);
int y3_conv2d_wgrad_x3_ok(int m, int cin, int ksize, int cout);
/* Diagnostics: the kernel-gradient plan for m output pixels.  out8 = {bkr, bn, splits, chunk, tiles, in_kernel, grid,
 * pixel_table}: the m pixels are cut into `splits` runs of `chunk`; in_kernel = 1 when the last split of a tile reduces
 * the slabs inside the kernel (splits <= 8), else slab_reduce_kernel follows.  Returns the workspace bytes. */
size_t y3_conv2d_wgrad_plan(int m, int cin, int ksize, int cout, int* out8);
size_t y3_conv2d_wgrad_plan_x(int m, int cin, int ksize, int cout, unsigned flags, int* out8);

/* wt_t[tap][co][ci] = wt[tap][ci][co] */
int y3_transpose_weights(const float* wt, float* wt_t, int taps, int cin, int cout, y3_stream_t stream);
/* The same for every layer of a parameter arena in ONE launch.  table_dev: DEVICE int32 [nlayers][5] =
 * {arena offset (floats), taps, cin, cout, index of the layer's first 32x32 tile}; total_tiles = sum over layers of
 * taps * ceil(cin/32) * ceil(cout/32). */
int y3_transpose_weights_batched(const float* params, float* params_t, const int* table_dev, int nlayers,
                                 int total_tiles, y3_stream_t stream);

/* ---- BatchNormalization(axis=1), eps 1e-3, momentum .99 (model.py:38) ---- */
/*
 * Training forward, step 1: reduce conv-epilogue partials to batch mean and
 * biased variance; write scale = gamma*rsqrt(var+eps), shift = beta-mean*scale;
 * save mean / rstd for backward; update moving stats
 * (moving = moving*mom + batch*(1-mom), variance Bessel-corrected).
 */
int y3_bn_stats_finalize(const float* stats, int tiles, int c, int count,
                         const float* gamma, const float* beta, float eps, float momentum,
                         float* moving_mean, float* moving_var,
                         float* save_mean, float* save_rstd, float* scale, float* shift,
                         y3_stream_t stream);
/* moving-stats (inference) affine: scale = gamma*rsqrt(var+eps), shift = beta-mean*scale */
int y3_bn_fold_inference(const float* gamma, const float* beta, const float* moving_mean,
                         const float* moving_var, float eps, int c, float* scale, float* shift,
                         y3_stream_t stream);
/* The same for every BatchNorm layer in ONE launch.  table_dev: DEVICE int32 [nlayers][7] = float offsets of
 * {gamma, beta} in `params`, {moving mean, moving var} in `moving`, {scale, shift} in `chan`, and the channel count. */
int y3_bn_fold_inference_batched(const float* params, const float* moving, float* chan, const int* table_dev,
                                 int nlayers, float eps, y3_stream_t stream);
/* y = a*scale + shift (+ resid)   (BN apply and the residual add of model.py:47) */
int y3_bn_apply(const y3_tensor* a, const float* scale, const float* shift, const y3_tensor* resid,
                const y3_tensor* y, y3_stream_t stream);
/*
 * Backward of conv_layer's tail  y = BN(lrelu(z)):  given dy and a = lrelu(z)
 *   step 1 (stats):  per-channel raw moments of (dy, a) in fp64 (workspace), then -- by the workgroup whose partial
 *                    arrives last, inside the same launch -- dgamma, dbeta, dbias (bias gradient of the conv) and the
 *                    per-channel coefficients k1,k2,k3 (coef[3][c]).  Optionally the residual fan-in of model.py:47
 *                    rides along while dy streams through: dres = dy (dres_accumulate == 0) or dres += dy.
 *                    Channels: 4 / 8 / 16, or a multiple of 32 up to 1024 (every layer of this network).
 *                    `workspace`: y3_bn_bwd_workspace(m, c) bytes, 16-byte aligned; its first 1 KiB (tickets) must be
 *                    zero before the FIRST call -- every call leaves it zero again.
 *   step 2 (apply):  dz = (k1*dy + k2*a + k3) * (a > 0 ? 1 : alpha)
 */
int y3_bn_bwd_stats(const y3_tensor* dy, const y3_tensor* a, const y3_tensor* dres, int dres_accumulate,
                    const float* gamma, const float* save_mean, const float* save_rstd, float alpha,
                    float* dgamma, float* dbeta, float* dbias, float* coef,
                    void* workspace, size_t workspace_bytes, y3_stream_t stream);
size_t y3_bn_bwd_workspace(int m, int c); /* 0 if the channel count is unsupported */
int y3_bn_bwd_apply(const y3_tensor* dy, const y3_tensor* a, const float* coef, float alpha,
                    const y3_tensor* dz, y3_stream_t stream);
/* step 2 with the residual fan-in of model.py:47 riding along: dres = dy (dres_accumulate == 0) or dres += dy */
int y3_bn_bwd_apply_fanin(const y3_tensor* dy, const y3_tensor* a, const float* coef, float alpha,
                          const y3_tensor* dz, const y3_tensor* dres, int dres_accumulate, y3_stream_t stream);
/*
 * Step 1 without a pass of its own: when the LAST contribution to dy is written by a stride-1 data gradient
 * (y3_conv2d_dgrad_bn above: its epilogue has dy in registers), that launch leaves per-row-tile partial moments
 * [tiles][6][c] (fp32) and this call turns them into dgamma / dbeta / dbias / coef (fp64 across tiles).
 */
int y3_bn_bwd_finalize_tiles(const float* partials, int tiles, int c, int count, const float* gamma,
                             const float* save_mean, const float* save_rstd, float alpha,
                             float* dgamma, float* dbeta, float* dbias, float* coef, y3_stream_t stream);
/*
 * The same backward with FROZEN statistics (no call site in the reference: fine-tuning).  Forward was
 * y = a*scale + shift with scale = gamma / sqrt(moving_var + eps) and shift folded from the moving statistics
 * (y3_bn_fold_inference*), so nothing of the batch enters the normalisation and ONE pass over dy and a does it all:
 *   dz   = (dy * scale_c) * (a > 0 ? 1 : alpha)        two fp32 roundings, in this order
 *   dres = dy (dres_accumulate == 0) or dres += dy      when dres is given: the residual fan-in of model.py:47
 *   S1 = sum dy, S2 = sum dy*a, S3 = sum dz (the stored fp32 values): every term converted to fp64, summed in fp64 in a fixed order
 *   dbeta = S1,  dgamma = (S2 - mean_c * S1) / sqrt(var_c + eps) in fp64,  dbias = S3,  each rounded to fp32 once.
 * The sums are reduced inside the launch as in y3_bn_bwd_stats: fp64 partials in `workspace`, combined by the workgroup that
 * arrives last, in an order that does not depend on which one that is -- no floating-point atomics, two launches give the same
 * bits.  `workspace`: y3_bn_frozen_bwd_workspace(m, c) bytes, 16-byte aligned; its first 1 KiB (tickets) must be zero before the
 * FIRST call and every call leaves it zero again.
 * dy, a, dz (and dres): NHWC views of one geometry, any ld >= c; channels 4 / 8 / 16 or a multiple of 32 up to 1024.  Views whose
 * ld is a multiple of 4 and whose base is 16-byte aligned are accessed 16 bytes at a time, otherwise element by element.  dz must
 * not overlap dy, a or dres.  scale: 16-byte aligned.  Y3_EINVAL before any launch for a null pointer, an unsupported channel
 * count, mismatched shapes, an overlapping dz, a too small or misaligned workspace, a non-finite eps.
 */
int y3_bn_frozen_bwd(const y3_tensor* dy, const y3_tensor* a, const y3_tensor* dres, int dres_accumulate,
                     const float* scale, const float* moving_mean, const float* moving_var, float eps, float alpha,
                     const y3_tensor* dz, float* dgamma, float* dbeta, float* dbias,
                     void* workspace, size_t workspace_bytes, y3_stream_t stream);
size_t y3_bn_frozen_bwd_workspace(int m, int c); /* 0 if the channel count is unsupported */

/* ---- upsample_2x: frozen all-ones Conv2DTranspose k2 s2 (model.py:94-105) ---- */
/* out[n,2i+a,2j+b,co] = sum_ci in[n,i,j,ci] for every co */
int y3_upsample_sum2x_fwd(const y3_tensor* in, const y3_tensor* out, y3_stream_t stream);
/* din[n,i,j,ci] = sum_{a,b,co} dout[n,2i+a,2j+b,co] for every ci */
int y3_upsample_sum2x_bwd(const y3_tensor* dout, const y3_tensor* din, y3_stream_t stream);

/* ---- spatial pyramid pooling of YOLOv3-SPP (no call site in the reference: an opt-in variant) ----
 * dst[n,i,j, b*C + c] = max of src[n,i',j',c] over the (2r+1)^2 window around (i,j) clipped to the image, r = 2, 4, 6 for the
 * channel blocks b = 0, 1, 2: [pool5 | pool9 | pool13], stride 1, padding SAME, padded positions never win.  One launch reads src
 * once and writes all three blocks.  src is N x H x W x C, dst N x H x W x 3C, both NHWC with any ld; C and both ld multiples of 4,
 * pointers 16-byte aligned (bf16: 8-byte).  src and dst may be disjoint channel ranges of ONE allocation (the model: slice 0 and
 * slice [C, 4C) of the concat buffer the next convolution reads).  Exact: max does not round; -0 / +0 may come out as either;
 * +-inf are ordinary values; a NaN in a window gives NaN for that window.
 * H * W <= Y3_SPP_MAX_PLANE (any H, W up to 64 x 64; every grid of the model is at most 19 x 19): the plane of a channel group is
 * staged in LDS, a larger one is refused with Y3_EINVAL.  Planes of more than 2048 pixels raise the kernel's dynamic LDS limit
 * (a host call on the current device) before the launch: keep those out of a stream capture. */
#define Y3_SPP_MAX_PLANE 4096
int y3_spp_fwd(const y3_tensor* src, const y3_tensor* dst, y3_stream_t stream);      /* fp32 */
int y3_spp_fwd_bf16(const y3_tensor* src, const y3_tensor* dst, y3_stream_t stream); /* bf16 storage, as y3_upsample_sum2x_fwd_bf16 */
/* dsrc[p] (+)= sum over the three pools k and the pixels q whose k x k window has its FIRST maximum in row-major order at p of
 * ddst[q, block k]: the subgradient torch.nn.functional.max_pool2d(x, k, 1, k // 2) takes.  src is the forward input, ddst the
 * gradient of dst (N x H x W x 3C), dsrc N x H x W x C, fp32, same layout rules and plane limit; ddst and dsrc may be disjoint
 * channel ranges of one allocation.  accumulate != 0 adds to what dsrc holds (the identity branch's gradient), 0 overwrites.  A
 * gather per input pixel in a fixed order, no atomics: two runs give the same bits.  NaN in src: some in-bounds pixel wins.
 * (Two instantiations by plane size, 512 pixels and below or above: the same arithmetic in the same order.) */
int y3_spp_bwd(const y3_tensor* src, const y3_tensor* ddst, const y3_tensor* dsrc, int accumulate, y3_stream_t stream);

/* ---- bf16 inference path (BASELINE config 5: tiled inference with a bf16 conv path) ----------------
 * Tensors are NHWC with `ld` counted in ELEMENTS; `ptr` addresses bf16 (2-byte) elements unless noted.
 * Replaces the same Conv2D -> LeakyReLU -> BatchNorm(training=False) chain as y3_conv2d_fwd
 * (model.py:71-91,108-137) when inference runs in reduced precision: bf16 operands, fp32 accumulate on
 * v_mfma_f32_32x32x16_bf16, fp32 epilogue (bias, lrelu, folded BN scale/shift, residual), one rounding on store.
 * wt_t_bf16 is the y3_transpose_weights layout [kh][kw][Cout][Cin] converted with y3_f32_to_bf16.
 * Requires Cin % 32 == 0 (the first RGB layer stays on y3_conv2d_fwd).  dst_is_f32 != 0 writes fp32
 * (used for the three head convs so that decode / NMS stay fp32).
 * Which kernel runs is the library's choice and does not change the contract: the 3x3 layers 32 -> 64 and 64 -> 128 with bf16
 * output and 16-byte aligned rows (the 608^2 -> 152^2 stages of the tiled path) take HBM-bound patch kernels (input patch once
 * through LDS, weights in registers), Cin % 64 == 0 with Cout >= 256 and >= 96 tiles of 256 x 256 the ping-pong kernel, the rest
 * the LDS-DMA ring kernel.  All of them accumulate in fp32 and round once.
 * Y3_BF16_NO_PATCH in `flags` keeps a launch off the patch kernels: they win where a layer streams from HBM (hundreds of MB:
 * batches of 25+ tiles of 608^2) and lose 2 % of a whole forward at batch 8, where the next layer finds the ring kernel's
 * output in its own XCD's L2 (the patch kernels write strip-wise).  The caller knows its batch: yolo3/model.py sets the flag for
 * layers that move less than 300 MB. */
#define Y3_BF16_NO_PATCH 8u
int y3_conv2d_fwd_bf16(const y3_tensor* src, const void* wt_t_bf16, const float* bias, int ksize, int stride,
                       const y3_tensor* dst, int dst_is_f32, unsigned flags, float alpha,
                       const float* scale, const float* shift, const y3_tensor* resid, y3_stream_t stream);
/* The same with a caller-owned workspace (y3_conv2d_fwd_bf16_workspace(m = N*OH*OW, cin, ksize, cout) bytes; zero it once, the
 * first 256 KiB are per-tile tickets (the same header as the fp32 entries, so one zeroed workspace can serve both) that every launch leaves at zero; one stream per workspace): the small-M layers
 * (<= 512 tiles of 64 x 64 and >= 32 K steps: the 13x13 / 26x26 / 19x19 grids at batch 8) are then split along K into up to 8
 * slices whose fp32 partial sums the last-arriving slice adds in slice order inside the kernel (bit-reproducible).  Without a
 * workspace (or with y3_conv2d_fwd_bf16) every tile walks its whole K. */
size_t y3_conv2d_fwd_bf16_workspace(int m, int cin, int ksize, int cout);
int y3_conv2d_fwd_bf16_ws(const y3_tensor* src, const void* wt_t_bf16, const float* bias, int ksize, int stride,
                          const y3_tensor* dst, int dst_is_f32, unsigned flags, float alpha,
                          const float* scale, const float* shift, const y3_tensor* resid,
                          void* workspace, size_t workspace_bytes, y3_stream_t stream);
/* Which kernel y3_conv2d_fwd_bf16_ws would run for exactly these arguments (without the stream), on which tile and grid: the
 * entry point's own description of the launch (the fields it dispatches on), host only -- nothing is launched and no pointer
 * is dereferenced (of src / dst / resid -> ptr, the weights, the bias and the workspace only alignment and null-ness are read;
 * scale / shift: null-ness).
 * Returns the workspace bytes the launch would use (0: no split-K) and fills out12 with
 *   {route, bm, bn, bk, grid, threads, splits, chunk, vec_ok, patch stride, patch residual, nk}
 * route: one of Y3_BF16_ROUTE_*; bm x bn the output tile (patch kernels: the 32 x 8 / 4 / 2 output pixels of one row group by
 * Cout), bk the K step; grid workgroups of `threads`; every tile cut into `splits` K slices of `chunk` steps, the last one
 * nk - (splits - 1) * chunk long (nk = K / bk steps in all; splits == 1: whole); vec_ok: 16-byte epilogue accesses (aligned
 * dst / resid rows), 0: element by element; patch stride / residual: the template instantiation of a patch kernel (stride 1 / 2;
 * residual 0 / 1, always 0 for the 64 -> 128 kernel, which tests it at run time), 0 / 0 elsewhere.  A launch the entry point
 * would refuse gives route 0 and returns 0; y3_last_error() has the reason.  y3_conv2d_fwd_bf16 is the same launch with a null
 * workspace. */
#define Y3_BF16_ROUTE_PP 1    /* the 256 x 256 ping-pong kernel */
#define Y3_BF16_ROUTE_C32 2   /* the 32 -> 64 3x3 patch kernel */
#define Y3_BF16_ROUTE_C64 3   /* the 64 -> 128 3x3 patch kernel */
#define Y3_BF16_ROUTE_RING 4  /* the LDS-DMA ring kernel (tiles 128x32, 128x64, 256x128, 128x128, 64x64; split-K on 64x64) */
size_t y3_conv2d_fwd_bf16_plan(const y3_tensor* src, const void* wt_t_bf16, const float* bias, int ksize, int stride,
                               const y3_tensor* dst, int dst_is_f32, unsigned flags, float alpha,
                               const float* scale, const float* shift, const y3_tensor* resid,
                               void* workspace, size_t workspace_bytes, int* out12);
/* The first (RGB) conv_layer straight to bf16: src fp32 NHWC with Cin padded to 4, wt the fp32 Keras kernel
 * [3][3][4][32], 3x3 stride 1 SAME, dst bf16 with 32 channels; same epilogue order as above.  fp32-accurate: input and
 * weights are split into three bf16 pieces each and multiplied on the matrix pipe (fp32 accumulation), one rounding on the
 * store.  Any image size; src rows 16-byte aligned. */
int y3_conv2d_first_bf16(const y3_tensor* src, const float* wt, const float* bias, const y3_tensor* dst,
                         unsigned flags, float alpha, const float* scale, const float* shift, y3_stream_t stream);
int y3_f32_to_bf16(const float* src, void* dst, size_t count, y3_stream_t stream); /* round-to-nearest-even */
int y3_upsample_sum2x_fwd_bf16(const y3_tensor* in, const y3_tensor* out, y3_stream_t stream); /* model.py:94-105 */

/* ---- small data movement -------------------------------------------------- */
int y3_copy(const y3_tensor* src, const y3_tensor* dst, y3_stream_t stream);        /* strided copy (tf.concat, model.py:368,375) */
int y3_add_inplace(const y3_tensor* src, const y3_tensor* dst, y3_stream_t stream); /* dst += src (gradient fan-in) */
int y3_fill(float* ptr, size_t count, float value, y3_stream_t stream);
/* model input [N,C,H,W] -> NHWC with channels zero-padded to dst->c (multiple of 4) */
int y3_nchw_to_nhwc(const float* src, int n, int c, int h, int w, const y3_tensor* dst, y3_stream_t stream);
/* NHWC view -> dense [N,C,H,W] (feature-map export, model.py:462) */
int y3_nhwc_to_nchw(const y3_tensor* src, float* dst, y3_stream_t stream);
/* column sums: out[c] = sum_pixels src  (bias gradient of the detection layers) */
int y3_colsum(const y3_tensor* src, float* out, y3_stream_t stream);

/* ---- anchor decode: reorg_layer + convert_feature_map_to_inference_detections
 *      (model.py:122-212).  fm[s]: NHWC [N,G,G,A*(5+K)]; out: [N,Nb,5+K] rows
 *      [x0,y0,x1,y1,obj,cls..], scales coarse->fine, then row, col, anchor.
 *      anchors: host [A][2] (w,h).  stride quirk Q6 reproduced:
 *      x uses img_h/grid_h, y uses img_w/grid_w. */
int y3_decode_fwd(const y3_tensor* fm, int nscales, const float* anchors_host, int num_anchors,
                  int num_classes, int img_h, int img_w, float* out, y3_stream_t stream);

/* ---- loss_layer forward + backward for one scale (model.py:230-354) --------
 * fm NHWC [N,G,G,A*(5+K)], gt dense [N,G,G,A,5+K].  Adds the four terms
 * (xy, wh, obj, class; each / local batch) into loss4[0..3] and writes
 * dfm = d(total/global_batch)/d(fm) with fm's layout.  loss4 is accumulated
 * (zero it before the first scale).  workspace: y3_loss_workspace_bytes().
 */
int y3_loss_fwd_bwd(const y3_tensor* fm, const float* gt, const float* anchors_host, int num_anchors,
                    int num_classes, int img_h, int img_w, float global_batch,
                    float* loss4, const y3_tensor* dfm, void* workspace, y3_stream_t stream);
size_t y3_loss_workspace_bytes(void);

/* ---- opt-in IoU box-regression losses (not in the reference) -----------------------------------------
 * y3_loss_fwd_bwd_ex: y3_loss_fwd_bwd with a choice of box term.  Y3_BOX_LOSS_MSE (box_weight must be 1) is exactly the
 * launch of y3_loss_fwd_bwd: the reference's xy term (model.py:313-333, :351) and wh term (model.py:337-345, :352).  The
 * other kinds depart from those lines only: objectness, class, ignore mask (Q7), the anchor-present flags, the 64-block partial
 * reduction and the finalize step are the same code, so dfm[..., 4:] and loss4[2], loss4[3] keep their bits.  Per (cell,
 * anchor) with label row g and gm = g[4], the predicted box as reorg_layer decodes it (Q6 included):
 *   bx = (sigmoid(t0) + gx) sx, by = (sigmoid(t1) + gy) sy, bw = exp(t2) aw, bh = exp(t3) ah; target centre (g0, g1), size
 *   (g2, g3); corners c -+ s/2.  inter = max(min(x1) - max(x0), 0) max(min(y1) - max(y0), 0), U = bw bh + g2 g3 - inter,
 *   IoU = inter / U; enclosing box cw x ch, C = cw ch, c2 = cw^2 + ch^2, rho2 = (bx - g0)^2 + (by - g1)^2.
 *   Y3_BOX_LOSS_GIOU (Rezatofighi et al. 2019): X = IoU - (C - U) / C.
 *   Y3_BOX_LOSS_DIOU (Zheng et al. 2020):       X = IoU - rho2 / c2.
 *   Y3_BOX_LOSS_CIOU (Zheng et al. 2020):       X = IoU - rho2 / c2 - alpha v, v = (4 / pi^2)(atan(g2 / g3) - atan(bw / bh))^2,
 *                                               alpha = v / ((1 - IoU) + v + 1e-7), a constant of the backward pass.
 * loss4[0] += sum(gm box_weight (1 - X)) / local batch, loss4[1] += 0, and dfm[..., 0:4] = gm box_weight d(1 - X)/dt /
 * (local batch * global_batch); min, max and the clamp at 0 pass the gradient to the selected operand.  Where gm == 0 the
 * term is skipped by a branch: dfm[..., 0:4] = +0 there whatever the logits are.  Finite for every logit in [-30, 30].
 * box_loss outside 0..3, box_weight not finite or <= 0, or box_weight != 1 with Y3_BOX_LOSS_MSE: Y3_EINVAL + message,
 * nothing launched.  workspace: y3_loss_workspace_bytes(), as for y3_loss_fwd_bwd. */
#define Y3_BOX_LOSS_MSE  0   /* the reference's xy + wh terms: what y3_loss_fwd_bwd computes */
#define Y3_BOX_LOSS_GIOU 1
#define Y3_BOX_LOSS_DIOU 2
#define Y3_BOX_LOSS_CIOU 3
int y3_loss_fwd_bwd_ex(const y3_tensor* fm, const float* gt, const float* anchors_host, int num_anchors,
                       int num_classes, int img_h, int img_w, float global_batch, int box_loss, float box_weight,
                       float* loss4, const y3_tensor* dfm, void* workspace, y3_stream_t stream);

/* ---- opt-in ignore mask against each image's ground-truth boxes (not in the reference) ---------------
 * The reference's mask is model.py:250-282.  It quotes the paper next to it (model.py:282: a prediction that is not the best but overlaps a ground-truth
 * object by more than 0.5 is ignored), but the code above that line (model.py:250-275, Q7) compares with origin-centred
 * anchor-sized boxes gathered over the whole replica batch.  y3_loss_fwd_bwd and y3_loss_fwd_bwd_ex reproduce that; the two
 * entry points below state the paper's rule.
 *
 * y3_truth_boxes: the per-image box lists of one dense label tensor gt [n][cells_anchors][d], d = 5 + K.  For image i the
 * rows with gt[..., 4] != 0 have their first four floats (centre x, centre y, w, h in pixels) copied to boxes[i][0..] in
 * index order (row, column, anchor); boxes is [n][cap][4].  counts[i] is the TRUE number of such rows, also when it exceeds
 * cap; rows from cap on are not written, and slots past min(count, cap) are left untouched (nothing needs zeroing).  One
 * workgroup per image, ordered append by ballot prefix: no atomics, the same bits on every run.
 *
 * y3_loss_fwd_bwd_truth: y3_loss_fwd_bwd_ex with the truth mask.  Per (cell, anchor) with gm = g[4] and the predicted box
 * (bx, by, bw, bh) as above (Q6 included): best = max over j < min(truth_counts[image], truth_cap) of the IoU with
 * truth_boxes[image][j], in fp32 from corners c -+ s/2, inter / (bw bh + tw th - inter), combined with fmaxf from -INFINITY
 * (an empty list leaves every negative valid, a NaN IoU is dropped); ignore = best < ignore_thresh ? 1 : 0 and
 * valid = gm + (1 - gm) ignore feed the objectness term, a constant of the backward pass.  Only the objectness term
 * departs from y3_loss_fwd_bwd_ex: dfm[..., 0:4] and dfm[..., 5:] keep their bits for every box_loss; loss4[0], loss4[1] and
 * loss4[3] are the same terms added up over another block partition.  *ignored (may be NULL) is increased by the number of predictions with gm == 0 and ignore == 0 of this call
 * (a float, exact at these counts), through the block partials and a fixed-order finalize like loss4: no atomics.
 * A workgroup works on one image, whose list it stages in LDS Y3_TRUTH_CHUNK boxes at a time.
 * ignore_thresh not finite or outside (0, 1], truth_cap < 1, truth_boxes or truth_counts NULL, or box_loss / box_weight
 * against the rules of y3_loss_fwd_bwd_ex: Y3_EINVAL + message, nothing launched.
 * workspace: y3_loss_truth_workspace_bytes(n) for a batch of n images (0 for n < 1). */
#define Y3_TRUTH_CHUNK 256   /* boxes staged in LDS at a time (16 bytes each) */
int y3_truth_boxes(const float* gt, int n, long long cells_anchors, int d, float* boxes, int* counts, int cap,
                   y3_stream_t stream);
size_t y3_loss_truth_workspace_bytes(int n);
int y3_loss_fwd_bwd_truth(const y3_tensor* fm, const float* gt, const float* anchors_host, int num_anchors,
                          int num_classes, int img_h, int img_w, float global_batch, int box_loss, float box_weight,
                          const float* truth_boxes, const int* truth_counts, int truth_cap, float ignore_thresh,
                          float* loss4, float* ignored, const y3_tensor* dfm, void* workspace, y3_stream_t stream);

/* ---- opt-in focal loss and class-label smoothing (not in the reference) ------------------------------
 * The reference's objectness term is model.py:286-287 and its class term model.py:293-294, both plain
 * tf.nn.sigmoid_cross_entropy_with_logits.  y3_loss_fwd_bwd_focal stands beside those lines only: decode, ignore mask
 * (reference, Q7, or truth), box terms, partial sums and the finalize step are y3_loss_fwd_bwd_ex's / _truth's, so
 * dfm[..., 0:4], loss4[0], loss4[1] and *ignored keep their bits.  For a label z in [0, 1], a logit x and p = sigmoid(x):
 *   ce = max(x, 0) - x z + log1p(exp(-|x|))
 *   m  = z sigmoid(-x) + (1 - z) sigmoid(x)            (1 - p_t of Lin et al. 2017, formed without that subtraction)
 *   w  = alpha z + (1 - alpha)(1 - z) for alpha != 0, else 1
 *   FL = w m^gamma ce,   dFL/dx = w [m^gamma (p - z) + gamma m^gamma r (1 - 2z) ce],   r = p (1 - p) / m, r = 0 where m = 0.
 * r <= 1, and m^(gamma - 1) is never formed: both are finite for every gamma >= 0 and every logit, saturated ones included.
 * Objectness: loss4[2] += sum(valid FL(gm, t4; gamma_obj, alpha_obj)) / local batch, with valid as in the entry points above.
 * Class: z' = g (1 - label_smoothing) + label_smoothing / 2 (Keras BinaryCrossentropy(label_smoothing)), and
 * loss4[3] += sum(gm FL(z', t; gamma_cls, alpha_cls)) / local batch.  dfm[..., 4:] holds the derivatives / (local batch *
 * global_batch).  A term is neutral when its gamma and alpha are 0 (and, for class, label_smoothing is 0): it takes the
 * plain expressions and keeps the bits of y3_loss_fwd_bwd_ex / _truth; with both terms neutral the launch is theirs.
 * truth_boxes == NULL and truth_counts == NULL select the reference mask: truth_cap, ignore_thresh and ignored are not
 * read and workspace is y3_loss_workspace_bytes().  Otherwise the arguments and the workspace of y3_loss_fwd_bwd_truth.
 * gamma not finite or < 0, alpha neither 0 nor in (0, 1), label_smoothing outside [0, 1), or any argument against the rules
 * of y3_loss_fwd_bwd_truth: Y3_EINVAL + message, nothing launched. */
int y3_loss_fwd_bwd_focal(const y3_tensor* fm, const float* gt, const float* anchors_host, int num_anchors,
                          int num_classes, int img_h, int img_w, float global_batch, int box_loss, float box_weight,
                          const float* truth_boxes, const int* truth_counts, int truth_cap, float ignore_thresh,
                          float* loss4, float* ignored, const y3_tensor* dfm, void* workspace, float gamma_obj,
                          float alpha_obj, float gamma_cls, float alpha_cls, float label_smoothing, y3_stream_t stream);

/* ---- tf.keras.optimizers.Adam.apply_gradients (model.py:451,500) ----------
 * m += (g-m)(1-b1); v += (g*g-v)(1-b2); p -= lr_t*m/(sqrt(v)+eps), with
 * lr_t read from DEVICE memory (*lr_t_dev, ONE float) so the launch is
 * graph-replayable.  This entry point and its _ema / _scaled forms below run
 * the kernel of y3_optim_step with everything that serves weight decay
 * compiled out; each states its form, so a NULL ema_param, omd_dev or
 * scale_dev is an error there (moving / ema_moving may be NULL with
 * moving_count == 0). */
int y3_adam_step(float* param, const float* grad, float* m, float* v, size_t count,
                 const float* lr_t_dev, float beta1, float beta2, float eps, y3_stream_t stream);

/* ---- y3_adam_step + an exponential moving average of the weights, one launch
 * (replaces a trainer's separate EMA pass after the optimiser step, e.g.
 * ultralytics' ModelEMA.update; no counterpart in the reference).  param, m, v
 * come out bit-identical to y3_adam_step; then, with omd = *omd_dev (1 - decay,
 * DEVICE memory like lr_t_dev):
 *   ema_param[i]  += (param_new[i] - ema_param[i]) * omd     i < count
 *   ema_moving[j] += (moving[j] - ema_moving[j]) * omd       j < moving_count
 * moving: the BatchNorm moving statistics of this step's forward pass.  Every
 * array 16-byte aligned; counts need not be multiples of 4. */
int y3_adam_step_ema(float* param, const float* grad, float* m, float* v, size_t count,
                     const float* lr_t_dev, float beta1, float beta2, float eps,
                     float* ema_param, const float* moving, float* ema_moving, size_t moving_count,
                     const float* omd_dev, y3_stream_t stream);

/* ---- gradient accumulation and global-norm gradient clipping (DESIGN 3.10;
 * Keras Adam(global_clipnorm=...) and the accumulation every YOLO trainer has;
 * no counterpart in the reference).  One optimiser step = k micro-steps:
 *   y3_grad_accumulate   acc = *first_dev ? grad : acc + grad  (plain fp32), and
 *                        the per-block fp64 sums of squares of the result
 *   y3_grad_sumsq        the same partial sums of grad alone (k = 1)
 *   y3_grad_clip_scale   S = the partials added in index order by one workgroup
 *                        (no atomics: the same bits on every run);
 *                        *norm_dev  = (float)(norm = sqrt(S) / k)
 *                        *scale_dev = (float)((1/k) * (clip / max(norm, clip))),
 *                        (float)(1/k) with clip_norm == Y3_GRAD_CLIP_OFF; fp64
 *   y3_adam_step_scaled / y3_adam_step_ema_scaled
 *                        y3_adam_step / y3_adam_step_ema on grad[i] * *scale_dev
 *                        (one fp32 multiply; the same bits when the scale is 1)
 * first_dev (int32), norm_dev, scale_dev are DEVICE memory, so a replayed graph
 * picks up each step's values.  workspace: y3_grad_norm_workspace_bytes(count),
 * 8-byte aligned, written whole by every accumulate / sumsq launch (no zeroing)
 * and read by the y3_grad_clip_scale that follows with the same count.  Arenas
 * 16-byte aligned; counts need not be multiples of 4. */
#define Y3_GRAD_CLIP_OFF ((double)INFINITY)
size_t y3_grad_norm_workspace_bytes(size_t count);
int y3_grad_accumulate(float* acc, const float* grad, size_t count, const int* first_dev, void* workspace,
                       y3_stream_t stream);
int y3_grad_sumsq(const float* grad, size_t count, void* workspace, y3_stream_t stream);
int y3_grad_clip_scale(const void* workspace, size_t count, int accumulate_steps, double clip_norm, float* norm_dev,
                       float* scale_dev, y3_stream_t stream);
int y3_adam_step_scaled(float* param, const float* grad, float* m, float* v, size_t count,
                        const float* lr_t_dev, float beta1, float beta2, float eps, const float* scale_dev,
                        y3_stream_t stream);
int y3_adam_step_ema_scaled(float* param, const float* grad, float* m, float* v, size_t count,
                            const float* lr_t_dev, float beta1, float beta2, float eps,
                            float* ema_param, const float* moving, float* ema_moving, size_t moving_count,
                            const float* omd_dev, const float* scale_dev, y3_stream_t stream);

/* ---- SGD with momentum and AdamW, with weight decay on some segments of the
 * arena (torch.optim.SGD(momentum, nesterov, weight_decay) and
 * AdamW as Keras and PyTorch apply it; the reference trains with plain Adam,
 * model.py:451, and declares a WEIGHT_DECAY it never applies).  One launch
 * over one flat arena, described by a HOST struct.  Each line one fp32
 * expression as written; D = element i lies in a decay range; g' = g, or
 * g * *scale_dev with scale_dev given (as y3_adam_step_scaled):
 *   Y3_OPT_SGD / Y3_OPT_SGD_NESTEROV   lr = hyper_dev[0]
 *     if D: g' = g' + weight_decay * p          (coupled L2)
 *     m = momentum * m + g'
 *     p = p - lr * m                            (p - lr * (g' + momentum * m) with Nesterov)
 *   Y3_OPT_ADAMW                       lr_t = hyper_dev[0], lw = hyper_dev[1] (lr * weight decay)
 *     if D: p = p - lw * p                      (decoupled, before the step)
 *     then y3_adam_step's update; with n_ranges == 0 its bits
 * With the EMA pointers given, y3_adam_step_ema's average of param and moving
 * follows in the same pass.  hyper_dev, omd_dev, scale_dev are DEVICE memory,
 * so a replayed graph picks up each step's values.  decay_ranges_host: HOST
 * array of n_ranges pairs [begin, end) in floats, copied into the kernel
 * arguments: sorted, disjoint (touching allowed), begin < end <= count,
 * begin % 4 == 0, end % 4 == 0 or end == count.  No per-element mask: 5 fp32
 * streams per element for SGD, 7 for AdamW, 2 more with the EMA.
 * Y3_EINVAL + message, nothing launched: null or 16-byte-misaligned arenas,
 * unknown kind, v null with Y3_OPT_ADAMW, momentum outside [0, 1),
 * weight_decay < 0, n_ranges outside 0..Y3_OPT_MAX_RANGES, a broken range
 * rule, a partial set of EMA pointers, count of 2^34 floats or more.
 * count == 0: Y3_OK, nothing launched.  Counts need not be multiples of 4. */
#define Y3_OPT_SGD 0
#define Y3_OPT_SGD_NESTEROV 1
#define Y3_OPT_ADAMW 2
#define Y3_OPT_MAX_RANGES 128
typedef struct y3_optim_desc {
    int kind;                            /* Y3_OPT_* */
    float* param;
    const float* grad;
    float* m;                            /* momentum buffer (SGD) / first moment (ADAMW) */
    float* v;                            /* second moment: ADAMW only, NULL otherwise */
    size_t count;
    const float* hyper_dev;              /* DEVICE float[2]: {lr (SGD) or lr_t (ADAMW), lr * weight decay (ADAMW; unused by SGD)} */
    float momentum, weight_decay;        /* SGD */
    float beta1, beta2, eps;             /* ADAMW */
    const long long* decay_ranges_host;  /* HOST: n_ranges pairs [begin, end) in floats */
    int n_ranges;                        /* 0 .. Y3_OPT_MAX_RANGES */
    float* ema_param;                    /* the five EMA members: all NULL / 0 = no EMA */
    const float* moving;
    float* ema_moving;
    size_t moving_count;
    const float* omd_dev;
    const float* scale_dev;              /* NULL = unscaled */
} y3_optim_desc;
int y3_optim_step(const y3_optim_desc* d, y3_stream_t stream);

/* ---- class-wise NMS (bbox_utils.py:200-281; inference.py:72-79) ------------
 * rows [N,Nb,5+K].  A row is a candidate of class c if w > min_box and
 * h > min_box (strict) and sqrt(cls_c*obj) >= score_thr; greedy suppression
 * keeps iou <= iou_thr, in descending score order (ties: higher row index
 * first).  Optional clip of the corners to [0,clip_w]x[0,clip_h] before
 * everything (inference.py:62-65 intent); pass clip_w <= 0 to disable.
 * keep_idx [N,K,max_keep] int32 row indices in selection order,
 * keep_cnt [N,K] int32, keep_score [N,K,max_keep] fp32.
 * workspace: y3_nms_workspace_bytes(). */
int y3_nms_per_class(const float* rows, int n, int nb, int num_classes, float min_box,
                     float score_thr, float iou_thr, float clip_w, float clip_h,
                     int* keep_idx, int* keep_cnt, float* keep_score, int max_keep,
                     void* workspace, size_t workspace_bytes, y3_stream_t stream);
size_t y3_nms_workspace_bytes(int n, int nb, int num_classes);

/* ---- opt-in NMS variants (not in the reference) ----------------------------------------------------
 * y3_nms_per_class_ex: y3_nms_per_class with a method.  Candidates are selected exactly as y3_nms_per_class selects
 * them (one device function): optional clip, strict > small-box filter, score = sqrtf(cls * obj) >= score_thr.  The
 * order key is (score bits << 32) | row: larger score first, equal scores -> higher row index first.  Outputs keep the
 * layout and truncation rule of y3_nms_per_class: keep_idx [N,K,max_keep], keep_cnt [N,K] = min(count, max_keep),
 * keep_score [N,K,max_keep], in emission order.  All fp32 below is evaluated in the order written, no contraction
 * (-ffp-contract=off), so a NumPy float32 restatement reproduces it bit for bit (except expf, see gaussian).
 * iou(k, j) is y3_nms_per_class's: xl = max(kx0,x0), yt = max(ky0,y0), xr = min(kx1,x1), yb = min(ky1,y1),
 *   inter = max(yb - yt, 0) * max(xr - xl, 0), iou = inter / ((karea + area) - inter), area = (x1 - x0) * (y1 - y0).
 *
 * Y3_NMS_HARD: exactly the launch of y3_nms_per_class (sigma ignored).
 * Y3_NMS_DIOU (Zheng et al. 2020): the greedy rounds of y3_nms_per_class; candidate j survives kept box k iff
 *     d = iou - rho2 / c2 <= iou_thr, with
 *     dx = (x0 + x1) * 0.5f - (kx0 + kx1) * 0.5f,  dy = (y0 + y1) * 0.5f - (ky0 + ky1) * 0.5f,  rho2 = dx * dx + dy * dy,
 *     ex = max(kx1, x1) - min(kx0, x0),  ey = max(ky1, y1) - min(ky0, y0),  c2 = ex * ex + ey * ey.
 *     A NaN d (zero union, or c2 == 0) drops the candidate.  sigma ignored.
 * Y3_NMS_SOFT_LINEAR / Y3_NMS_SOFT_GAUSSIAN (Bodla et al. 2017): s = the candidate scores; until no live candidate is left:
 *     1. pick the live candidate with the largest key (score bits = its CURRENT score s);
 *     2. emit its row and s (keep_score holds the decayed score);
 *     3. every other live candidate j: iou = iou(pick, j) and
 *          linear:   if (iou > iou_thr) s = s * (1.0f - iou)
 *          gaussian: s = s * expf(-(iou * iou) / sigma)
 *     4. drop j when iou is NaN or !(s >= score_thr).
 *     Emitted scores never increase, so the output is in keep order.  Requires score_thr > 0 and, for gaussian,
 *     sigma > 0 (else Y3_EINVAL + message, nothing launched).  expf is the device library's (within about 1 ulp of the
 *     exact value), so gaussian scores agree with a float64 restatement to rounding, not bit for bit.
 * workspace: y3_nms_workspace_bytes_ex(n, nb, num_classes, method) bytes (hard / diou: y3_nms_workspace_bytes; soft:
 * 0 for nb <= 8192, the candidate state then lives in registers; workspace may be NULL when 0 bytes are needed). */
#define Y3_NMS_HARD 0
#define Y3_NMS_DIOU 1
#define Y3_NMS_SOFT_LINEAR 2
#define Y3_NMS_SOFT_GAUSSIAN 3
int y3_nms_per_class_ex(const float* rows, int n, int nb, int num_classes, int method, float min_box,
                        float score_thr, float iou_thr, float sigma, float clip_w, float clip_h,
                        int* keep_idx, int* keep_cnt, float* keep_score, int max_keep,
                        void* workspace, size_t workspace_bytes, y3_stream_t stream);
size_t y3_nms_workspace_bytes_ex(int n, int nb, int num_classes, int method);

/* bbox_utils.single_class_nms (bbox_utils.py:217-237): rows5 [M,5] = x0,y0,x1,y1,score; every row is
 * a candidate, the score is used as is.  keep_idx/keep_score [M], keep_cnt [1].
 * workspace: y3_nms_workspace_bytes(1, M, 1). */
int y3_nms_single_class(const float* rows5, int m, float iou_thr, int* keep_idx, int* keep_cnt,
                        float* keep_score, void* workspace, size_t workspace_bytes, y3_stream_t stream);

/* ---- tiled inference: merge of the tiles' detections on the device (inference_tiled.py:230-301) -----
 * y3_tile_merge appends the detections of one batch of n tiles to a pool of whole-image detections, in the order the host
 * loop produces them: tile order, class-major inside a tile, keep order inside a class; calls append in call order.
 * rows [n, nb, ld] / keep_idx [n,K,max_keep] / keep_cnt [n,K] / keep_score [n,K,max_keep]: the decode rows and the outputs of
 * y3_nms_per_class(_ex) for them (no clip).  table_dev: DEVICE int32 [n][6], the rows {y0, ny, pre_y, x0, nx, pre_x} of
 * y3_tile_gather's table for these tiles; y0 / x0 are the CLAMPED origins the merge shifts by (Q12).  For every kept entry
 * with box b0,b1,b2,b3 of tile (ty, tx), fp32 in the order written, no contraction (E = edge, th x tw = tile, H x W = image):
 *   cx = (b2 + b0) / 2, cxg = cx + tx;  cy = (b3 + b1) / 2, cyg = cy + ty;
 *   dropped (centre in a ghost band) when  (cyg > E && cy < E - margin) || (cyg <= H - E && cy >= (th - E) + margin)
 *                                       || (cxg > E && cx < E - margin) || (cxg <= W - E && cx >= (tw - E) + margin);
 *     E - margin and (th - E) + margin are fp32 operations on (float)E, margin, (float)(th - E); margin == 0 is bit for bit
 *     merge_tile_detections' test, margin > 0 lets both tiles keep an object whose centre lies within margin of their
 *     zone boundary (y3_nms_labelled then removes the duplicate);
 *   x0 = int32(rint(b0 + tx)), y0 = int32(rint(b1 + ty)), x1 = int32(rint(b2 + tx)), y1 = int32(rint(b3 + ty))  (np.round:
 *     half to even; a value outside int32 converts to INT_MIN as NumPy's x86-64 cast does);
 *   dropped (centre outside the image) when x0 + x1 < 0 || x0 + x1 >= 2 W, likewise y (the int32 sums, which is what
 *     finalize_predictions' float64 (x1 + x0) / 2.0 comparison decides);
 *   pool row = clamp(x0, 0, W-1), clamp(y0, 0, H-1), clamp(x1, 0, W-1), clamp(y1, 0, H-1), keep_score, class index.
 * The coordinates are stored as fp32, exact below 2^24: img_h, img_w <= 2^24 (Y3_EINVAL above).
 * pool: fp32 [cap][6].  pool_count: DEVICE int32 [2] = {rows written so far, rows needed so far}; zero it before the first
 * batch of an image.  A call adds its survivors to pool_count[1] whatever cap is, writes only the rows at positions < cap
 * and sets pool_count[0] = min(pool_count[1], cap): when pool_count[1] > cap the caller re-merges into a larger pool.
 * Two launches (count per (tile, class) segment; exclusive prefix + ordered write by ballot ranks).  No atomics, nothing
 * read back by the host.  0 <= margin < edge.  n * num_classes <= Y3_TILE_MERGE_MAX_SEGMENTS per call (every workgroup of
 * the second launch sums the counts before its segment itself; split a larger batch into several calls) and
 * n * num_classes * max_keep < 2^31.  pool_count[1] saturates at INT_MAX (2^31 - 1) when the batches of an image add up to
 * more: treat that value as an error.  workspace: y3_tile_merge_workspace_bytes(n, num_classes). */
#define Y3_TILE_MERGE_MAX_SEGMENTS 65536
int y3_tile_merge(const float* rows, int n, int nb, int ld, int num_classes, const int* keep_idx, const int* keep_cnt,
                  const float* keep_score, int max_keep, const int* table_dev, int tile_h, int tile_w, int img_h, int img_w,
                  int edge, float margin, float* pool, int cap, int* pool_count, void* workspace, size_t workspace_bytes,
                  y3_stream_t stream);
size_t y3_tile_merge_workspace_bytes(int n, int num_classes);

/* y3_tile_merge for tiles whose kept boxes were replaced by box voting (tile test-time augmentation): voted
 * [n][K][max_keep][6] is y3_box_vote's out for the batch, and entry e = (t * K + c) * max_keep + j takes its box from
 * voted[e * 6 + 0 .. 3] and its score from voted[e * 6 + 4] instead of rows[keep_idx[e]] and keep_score[e].  Everything else is
 * y3_tile_merge's: the ghost test, the shift, the rounding, the centre test, the clamp, the ordered append, the two launches, the
 * limits and the workspace.  keep_idx is still range-checked against nb (an entry outside 0 .. nb-1 is skipped), so with voted
 * filled from rows[keep_idx] and keep_score the pool is y3_tile_merge's byte for byte. */
int y3_tile_merge_voted(const float* voted, int n, int nb, int num_classes, const int* keep_idx, const int* keep_cnt,
                        int max_keep, const int* table_dev, int tile_h, int tile_w, int img_h, int img_w, int edge, float margin,
                        float* pool, int cap, int* pool_count, void* workspace, size_t workspace_bytes, y3_stream_t stream);

/* y3_nms_labelled: class-wise NMS over such a pool.  pool [m][6] = x0,y0,x1,y1,score,class; workgroup c takes the rows whose
 * column 5 == (float)c (a label outside 0..K-1 belongs to no class) with score > 0 and score >= score_thr as candidates, the
 * score as is (the order key is the score's bit pattern, so a row with a zero, negative or NaN score is never a candidate,
 * whatever the method), and runs y3_nms_per_class_ex's method on them: the same
 * kernels, key order (larger score first, equal scores: higher row first), IoU, DIoU and soft decay.  Y3_NMS_NONE: no
 * suppression at all -- the candidates in key order, no IoU formed (two zero-area boxes have IoU 0/0 and would drop each other
 * under any threshold).  keep_idx [K][max_keep] pool row indices, keep_cnt [K], keep_score [K][max_keep]: the layout
 * y3_eval_match reads for n = 1.  m >= 1.  workspace: y3_nms_workspace_bytes_ex(1, m, num_classes, method) (Y3_NMS_NONE:
 * y3_nms_workspace_bytes(1, m, num_classes)). */
#define Y3_NMS_NONE 4   /* y3_nms_labelled only */
int y3_nms_labelled(const float* pool, int m, int num_classes, int method, float score_thr, float iou_thr, float sigma,
                    int* keep_idx, int* keep_cnt, float* keep_score, int max_keep, void* workspace, size_t workspace_bytes,
                    y3_stream_t stream);

/* ---- test-time augmentation: flipped / transposed views, boxes mapped back, box voting (not in the reference) ----
 * A view is a 3-bit code: Y3_TTA_TRANSPOSE (applied first), then Y3_TTA_FLIP_X and Y3_TTA_FLIP_Y; 0 is the identity.  With
 * T = transpose ? S^T : S, view[y][x] = T[flip_y ? H-1-y : y][flip_x ? W-1-x : x].  A view list is a HOST array of
 * 1 <= k <= Y3_TTA_MAX_VIEWS distinct codes; a code with Y3_TTA_TRANSPOSE needs H == W.  A bad list is Y3_EINVAL + message and
 * nothing is launched.
 *
 * y3_tta_views_nhwc: src fp32 [n][c][h][w] (z-scored already: the statistics of an image are those of its views) -> dst, the
 * network's NHWC input of n * k images, image-major and view-minor: image i * k + v is view views[v] of source image i.
 * dst->n == n * k, dst->h == h, dst->w == w, dst->c >= c and a multiple of 4 (channels c .. dst->c - 1 are written as zero, as
 * y3_nchw_to_nhwc writes them), dst->ld >= dst->c and a multiple of 4 (the floats of a pixel beyond dst->c are not touched),
 * dst->ptr 16-byte aligned.  Each 32 x 32 source tile is read once, four channel planes at a time, staged in LDS (row pitch 33
 * dwords) and stored to all k views as 16-byte pixels along the destination row, for transposed and straight views alike.  A
 * copy: bit-exact, NaN payloads included.
 *
 * y3_tta_unmap: rows [n_views][nb][ld] decode rows (corners x0, y0, x1, y1 first), n_views a multiple of k, image j being view
 * views[j % k].  In place, the inverse map (un-flip, then transpose), W = (float)img_w, H = (float)img_h:
 *   flip x:    (x0, x1) <- (W - x1, W - x0)
 *   flip y:    (y0, y1) <- (H - y1, H - y0)
 *   transpose: (x0, y0, x1, y1) <- (y0, x0, y1, x1)
 * one fp32 subtraction per value, as written.  Columns 4 .. ld-1 are not touched; rows of view 0 are not touched at all.
 * img_h, img_w <= 2^24. */
#define Y3_TTA_FLIP_X 1
#define Y3_TTA_FLIP_Y 2
#define Y3_TTA_TRANSPOSE 4
#define Y3_TTA_MAX_VIEWS 8
int y3_tta_views_nhwc(const float* src, int n, int c, int h, int w, const int* views, int k, const y3_tensor* dst,
                      y3_stream_t stream);
int y3_tta_unmap(float* rows, int n_views, int nb, int ld, const int* views, int k, int img_h, int img_w, y3_stream_t stream);

/* y3_box_vote (Gidaris & Komodakis 2015): every box the NMS kept becomes the score-weighted mean of the candidates that overlap
 * it.  rows [n][nb][5+K] with nb = views * rows_per_view: the unmapped rows of all views of an image, view v in rows
 * v * rows_per_view .. (v+1) * rows_per_view - 1.  keep_idx / keep_cnt / keep_score / max_keep: the outputs of
 * y3_nms_per_class(_ex) over those rows; min_box, score_thr, clip_w, clip_h: what that call got.  For keep j < keep_cnt[i][c]
 * with row r:
 *   candidates: the rows of image i that the NMS takes as candidates of class c (its device function: optional clip, strict >
 *     small-box filter, s = sqrtf(cls_c * obj) >= score_thr), boxes clipped as the NMS clips them;
 *   members: the candidates q with iou(r, q) >= vote_iou, iou being y3_nms_per_class_ex's fp32 expression in its order, no
 *     contraction; a NaN iou is no member (r itself has iou 1 unless its area is 0);
 *   box = sum s_q b_q / sum s_q over the members, products and sums in fp64, rounded to fp32 once.  Candidate p of the row-ordered
 *     candidate list goes to lane p % 64, a lane adds its members in increasing p, the 64 lanes are combined by an xor butterfly
 *     (32, 16, .. 1): no atomics, the same bits on every run, and within one fp32 unit in the last place of any other fp64
 *     summation order.  No member, or members whose scores sum to 0: the keep's own clipped box;
 *   score = Y3_VOTE_SCORE_KEEP: keep_score[i][c][j] unchanged;
 *           Y3_VOTE_SCORE_CONSENSUS: (sum over v < views of max{s_q : q member, q / rows_per_view == v}) / (float)views, a view
 *           without a member contributing 0; fp32, added in increasing v, divided once.
 * out [n][K][max_keep][6] = x0, y0, x1, y1, score, (float)c, written for j < keep_cnt[i][c] only.  A row kept under two classes
 * gets two independent results.  0 < vote_iou <= 1; n * num_classes <= 65535.  Two launches: the candidates of every
 * (image, class) compacted in row order, then one wave per keep.  workspace: y3_box_vote_workspace_bytes(n, nb, num_classes),
 * 4-byte aligned. */
#define Y3_VOTE_SCORE_KEEP 0
#define Y3_VOTE_SCORE_CONSENSUS 1
int y3_box_vote(const float* rows, int n, int nb, int num_classes, const int* keep_idx, const int* keep_cnt,
                const float* keep_score, int max_keep, float min_box, float score_thr, float clip_w, float clip_h,
                float vote_iou, int views, int rows_per_view, int score_mode, float* out, void* workspace,
                size_t workspace_bytes, y3_stream_t stream);
size_t y3_box_vote_workspace_bytes(int n, int nb, int num_classes);

/* bbox_utils.filter_small_boxes (bbox_utils.py:274-281): keep_idx[0..*keep_cnt) = indices, in row order, of the rows
 * [x0,y0,x1,y1,...] (pitch ld floats) with (x1-x0) > min_size and (y1-y0) > min_size (strict, Q19).  keep_idx holds m ints. */
int y3_filter_small_boxes(const float* rows, int m, int ld, float min_size, int* keep_idx, int* keep_cnt, y3_stream_t stream);

/* bbox_utils.compute_iou (bbox_utils.py:200-214): iou[i] = IoU(box4, boxes[i*ld .. i*ld+3]), corners, no +1, fp32 in the
 * reference's operation order (0/0 -> NaN as in NumPy). */
int y3_compute_iou(const float* box4, const float* boxes, int m, int ld, float* iou, y3_stream_t stream);

/* ---- imagereader.zscore_normalize (imagereader.py:34-46) -------------------
 * per image: mu = mean, sd = population std over all `count` values;
 * out = sd <= 1 ? x-mu : (x-mu)/sd.  workspace: y3_zscore_workspace_bytes(n). */
int y3_zscore(const float* in, float* out, int n, size_t count, void* workspace, y3_stream_t stream);
size_t y3_zscore_workspace_bytes(int n);

/* ---- inference_tiled.convert_image_to_tiles (inference_tiled.py:29-100) on the device -------------
 * img: HWC image resident in device memory, dtype 0 = uint8, 1 = uint16, 2 = float32.
 * table_dev: DEVICE int32 [ntiles][6] = {y0, ny, pre_y, x0, nx, pre_x}: tile t is the crop img[y0:y0+ny, x0:x0+nx]
 * with pre_y / pre_x reflected rows / columns in front and the rest of tile_h / tile_w reflected behind
 * (np.pad(mode='reflect'), inference_tiled.py:82-92).  out: float32 [ntiles][C][tile_h][tile_w] (astype + transpose,
 * inference_tiled.py:199-203). */
int y3_tile_gather(const void* img, int dtype, int height, int width, int channels, const int* table_dev,
                   int ntiles, int tile_h, int tile_w, float* out, y3_stream_t stream);

/* The same tiles, z-scored per tile (y3_zscore: whole-tile mean / population std, subtract-only when std <= 1) and written
 * straight into a network input buffer: out float32 NHWC [ntiles][tile_h][tile_w][channel_pitch] with the channels beyond C
 * zeroed (the layout y3_nchw_to_nhwc produces for the first conv_layer).  Two passes over the image instead of five over
 * the tiles; the results are the bits of y3_tile_gather -> y3_zscore -> y3_nchw_to_nhwc.  workspace:
 * y3_zscore_workspace_bytes(ntiles). */
int y3_tile_gather_zscore_nhwc(const void* img, int dtype, int height, int width, int channels, const int* table_dev,
                               int ntiles, int tile_h, int tile_w, float* out, int channel_pitch, void* workspace,
                               y3_stream_t stream);

/* The same tiles again, with their test-time augmentation views: out float32 NHWC
 * [ntiles * k][tile_h][tile_w][channel_pitch], tile-major and view-minor -- image t * k + v is view views_host[v] of tile t, the
 * layout y3_tta_views_nhwc gives images.  Bit for bit, view 0 of tile t is what y3_tile_gather_zscore_nhwc writes for tile t and
 * every other view is that tensor permuted by the view definition above (transpose first, then flip x, flip y); equivalently the
 * result is y3_tile_gather -> y3_zscore -> y3_tta_views_nhwc.  The statistics are per tile, computed once by the launches of
 * y3_tile_gather_zscore_nhwc; one 256-thread workgroup per 32 x 32 pixel block of a tile then gathers the block once through
 * the reflect index, normalises it, stages it in LDS (up to four channel planes, row pitch 33 dwords) and stores it to all k
 * views as 16-byte pixels along each destination row (straight views read LDS rows, transposed views LDS columns).
 * views_host: a HOST array, validated as y3_tta_views_nhwc validates it (a transposing code needs tile_h == tile_w).
 * channels <= 4; channel_pitch >= 4 and a multiple of 4 (every float of a pixel beyond `channels` is written as zero); out
 * 16-byte aligned; ntiles <= 65535.  workspace: y3_zscore_workspace_bytes(ntiles). */
int y3_tile_gather_zscore_views_nhwc(const void* img, int dtype, int height, int width, int channels, const int* table_dev,
                                     int ntiles, int tile_h, int tile_w, const int* views_host, int k, float* out,
                                     int channel_pitch, void* workspace, y3_stream_t stream);

/* ---- training augmentation on the device: augment.py:30-125, 275-297 at the severities of imagereader.py:369-391 ----------
 * The random decisions of augment_image_box_pair are drawn on the host (yolo3/augment.py draw_augmentation, same np.random
 * order up to the noise draw) into one record per image; the pixels never leave the device.  Per image i, with
 * H = h_out, W = w_out:
 *   1. resample + crop + flips.  Output pixel (r, c) reads the rescaled image (rows x cols) at row rr + dy, column cc + dx,
 *      rr = reflect_y ? H-1-r : r, cc = reflect_x ? W-1-c : c (the crop is taken before the flips, augment.py:289-296).
 *      Rescaled row q samples the source at ((2q+1) h_in - rows) / (2 rows) (skimage.transform.rescale's pixel centres),
 *      evaluated as an exact integer floor of that numerator plus an fp32 fraction of the remainder; columns alike.
 *      Bilinear; samples outside the source mirror without repeating the edge (scipy mode='mirror' = numpy 'reflect').
 *      rows == h_in and cols == w_in give an exact copy (uint8 / uint16 -> float32 exactly).
 *   2. noise (noise_severity > 0): x += s_i * N(0,1), s_i = noise_severity * (2 u_noise - 1) * (max_i - min_i), max / min over
 *      all channels of the crop after step 1 (the sign is kept, as augment.py does).  N(0,1) of element e = (ch*H + y)*W + x:
 *      Philox4x32-10, key = (seed low 32 bits, seed high 32 bits), counter = (e, 0, 0, 0); Box-Muller on the first two output
 *      words u1 = ((w0 >> 8) + 1) 2^-24, u2 = (w1 >> 8) 2^-24: sqrt(-2 ln u1) cos(2 pi u2).  The same record gives the same bits
 *      on every launch; it is NOT the host path's noise stream (np.random.standard_normal).
 *   3. blur (blur_sigma > 0): scipy.ndimage.gaussian_filter(img_hwc, blur_sigma, mode='reflect') -- truncate 4.0, radius
 *      int(4 sigma + 0.5) <= 8, weights exp(-k^2 / 2 sigma^2) normalised over -radius..radius -- on ALL THREE axes, the channel
 *      axis included (augment.py:122 passes a scalar sigma for an HWC image).  mode='reflect' repeats the edge (half-sample
 *      symmetric); on the channel axis the 1-D filter folds into a fixed C x C mix (for C = 3 the reflections wrap more than
 *      once; for C = 1 the fold is the identity).  radius 0 (sigma < 0.125) is the identity.
 *   4. out: float32 [n][C][H][W] (format_image's layout), ready for y3_zscore.
 * src: DEVICE [n][h_in][w_in][c], dtype 0 = uint8, 1 = uint16, 2 = float32 (as y3_tile_gather); c = 1 or 3; 2 source rows must
 * fit the LDS row stage (w_in * c * element size <= 30 KiB).  records: HOST array of n y3_aug_record, validated before any launch
 * (Y3_EINVAL + message: src_h / src_w != h_in / w_in, rows or cols < 1, dy + h_out > rows or dx + w_out > cols, negative
 * offsets, reflect flags not 0/1, non-finite or negative severity, u_noise outside [0, 1], non-finite blur_sigma or radius > 8,
 * bad dtype or c) and handed to the kernels as kernel arguments.  Passes: resample (+ min / max); noise + blur along W +
 * channel mix; blur along H -- the last two only for images that need them.  workspace: y3_augment_workspace_bytes(n, h_out,
 * w_out, c); after the call its first 2n uint32 words hold image i's max and -min as order-preserving keys (u = float bits;
 * key = sign ? ~u : u | 2^31). */
typedef struct y3_aug_record {
    int32_t src_h, src_w;        /* source image size (= h_in, w_in) */
    int32_t rows, cols;          /* rescaled size int(np.round(scale * src)) */
    int32_t dy, dx;              /* crop offset in the rescaled image */
    int32_t reflect_x, reflect_y;
    float noise_severity;        /* 0 = no noise */
    float u_noise;               /* the uniform of augment.py's noise sign / size draw */
    float blur_sigma;            /* <= 0 = no blur */
    int32_t reserved;            /* 0 */
    uint64_t seed;               /* Philox key of the noise */
} y3_aug_record;                 /* 56 bytes */
int y3_augment_batch(const void* src, int dtype, int n, int h_in, int w_in, int c, const y3_aug_record* records, int h_out, int w_out,
                     float* out, void* workspace, y3_stream_t stream);
size_t y3_augment_workspace_bytes(int n, int h_out, int w_out, int c);

/* ---- mosaic augmentation (not in the reference; yolo3/augment.py draw_mosaic / mosaic_boxes) -----------------
 * Every output image is put together from windows of up to four images of the SAME batch, one per quadrant around a seam
 * (cy, cx).  Quadrant q of output image i: 0 = rows [0,cy) x columns [0,cx), 1 = [0,cy) x [cx,w), 2 = [cy,h) x [0,cx),
 * 3 = [cy,h) x [cx,w); with (qy, qx) its origin and (qh, qw) its size,
 *     out[i][ch][y][x] = src[src[q]][ch][y - qy + oy[q]][x - qx + ox[q]]        for (y, x) in quadrant q, every channel ch.
 * A pure copy: the output bits are the input bits (NaN payloads and -0.0 included).  An empty quadrant (qh == 0 or qw == 0) reads
 * nothing and its fields are ignored.  cy = h, cx = w, src[0] = i, oy[0] = ox[0] = 0 copies image i through unchanged.
 * src, out: DEVICE float32 [n][c][h][w], c = 1 or 3, any h, w >= 1 (h * w < 2^31 - 8), 4-byte aligned; the ranges must not
 * overlap (the pass cannot run in place).  records: HOST array of n records, validated before any launch (Y3_EINVAL + message:
 * seam outside [0,h] x [0,w]; for a non-empty quadrant a source outside [0,n) or a window that leaves the source -- oy < 0,
 * oy + qh > h, likewise in x --; non-zero reserved; bad c, n, h, w; overlapping src / out) and handed to the kernel as kernel
 * arguments, 32 output images per launch; a source index may point anywhere in the batch.  Every output element is written by
 * exactly one thread: no atomics, no workspace, the same bits on every launch. */
typedef struct y3_mosaic_record {   /* 64 bytes, one per OUTPUT image */
    int32_t cy, cx;                 /* seam: 0 <= cy <= h, 0 <= cx <= w */
    int32_t src[4];                 /* source image of quadrant q, 0 <= src < n */
    int32_t oy[4], ox[4];           /* top-left corner of the window taken from that source */
    int32_t reserved[2];            /* 0 */
} y3_mosaic_record;
int y3_mosaic_batch(const float* src, int n, int c, int h, int w, const y3_mosaic_record* records_host, float* out,
                    y3_stream_t stream);

/* ---- affine warp (not in the reference; yolo3/augment.py draw_affine / affine_boxes / affine_reference) -------
 * Every output image is its own input image resampled through an affine map: rotation, shear, gain, translation.  The record
 * holds the INVERSE map, output pixel (x, y) -> source coordinate, pixel centres at the integers:
 *   coordinates    sx = (m0*x + m1*y) + m2, sy = (m3*x + m4*y) + m5 in fp32, x and y converted to fp32, every operation rounded on
 *                  its own in exactly this order (no fused multiply-add).  x0 = floor(sx), fx = sx - x0 in fp32; y alike.  NumPy
 *                  float32 arithmetic reproduces sx, sy, the floors and the fractions bit for bit (augment.affine_coords).
 *   interpolation  bilinear over the taps (y0 + {0,1}, x0 + {0,1}) of the pixel's own image and channel; a tap outside
 *                  [0,h) x [0,w) has the value `fill` -- scipy.ndimage.affine_transform(order=1, mode='grid-constant', cval=fill).
 *   weight zero    a tap whose weight is exactly zero (fx == 0: the right column; fx == 1, which fp32 gives for a tiny negative sx:
 *                  the left column; rows alike) contributes nothing and is not read: NaN or Inf there never reaches the output.
 *                  With fx == 0 and fy == 0 the output is the bits of the one tap, NaN payload and -0.0 included, so the identity
 *                  {1,0,0, 0,1,0}, integer translations, the flips {-1,0,w-1, 0,1,0} / {1,0,0, 0,-1,h-1} and the quarter turns
 *                  (square images: {0,-1,w-1, 1,0,0} and its powers) are exact copies / permutations (with `fill` where the
 *                  source lies outside).
 *   arithmetic     lerp(a, b, f) = f == 0 ? a : 1 - f == 0 ? b : (1 - f) * a + f * b, along x for both rows, then along y: at most
 *                  6 fp32 roundings on a tap's path, |out - exact| <= 6 * 2^-24 * sum |weight_i * tap_i| to first order.
 * src, out: DEVICE float32 [n][c][h][w], c = 1 or 3, any h, w >= 1 (h * w < 2^31 - 8, at most 2^23 tiles of 32 x 32), 4-byte
 * aligned; the ranges must not overlap (the pass cannot run in place).  records: HOST array of n records, validated before any
 * launch (Y3_EINVAL + message: null pointer; bad c, n, h, w; misaligned or overlapping src / out; non-zero reserved; a
 * non-finite coefficient or fill; |m0| (w-1) + |m1| (h-1) + |m2| > 2^30 or the same of m3..m5 with (w-1), (h-1) -- this sum bounds
 * the source coordinate at every corner of the output and every intermediate, so the float -> int conversion of the floor is
 * defined) and handed to the kernel as kernel arguments, 32 images per launch.  One thread per output pixel and all its
 * channels, 32 x 32 pixels per workgroup; every output element is written by exactly one thread: no atomics, no workspace, the
 * same bits on every launch. */
typedef struct y3_affine_record {   /* 32 bytes, one per image */
    float m[6];                     /* INVERSE map, output pixel -> source coordinate: sx = m0*x + m1*y + m2, sy = m3*x + m4*y + m5 */
    float fill;                     /* value of every tap outside the source */
    int32_t reserved;               /* 0 */
} y3_affine_record;
int y3_affine_batch(const float* src, int n, int c, int h, int w, const y3_affine_record* records_host, float* out,
                    y3_stream_t stream);

/* ---- colour / tone jitter and MixUp (not in the reference; yolo3/augment.py draw_photometric / draw_mixup / mixup_boxes /
 * photometric_reference) ------------------------------------------------------------------------------------------
 * One elementwise pass over an augmented batch, just before the z-score.  The z-score cancels a uniform gain and offset, so what
 * this pass offers is cross-channel (the matrix: hue, saturation) or non-linear (clamp, tone curve), and a blend of two images.
 * P_r(x), the photometric value of the pixel x (all its channels c0, c1, c2) under record r, is evaluated in fp32, every
 * operation rounded on its own in exactly this order (no fused multiply-add), so NumPy float32 reproduces stages 1, 2 and 4 bit
 * for bit (augment.photometric_reference):
 *   1 matrix   v_k = ((m_k0*c0 + m_k1*c1) + m_k2*c2) + bias_k.  A term whose coefficient is exactly 0 is not evaluated and its
 *              channel is not read for that row; a coefficient of exactly 1 passes its channel unmultiplied; a zero bias is not
 *              added; a row with no term and no bias is +0.  So a row with one coefficient 1, the others 0 and zero bias copies
 *              that channel's bits: the identity and the six channel permutations are exact copies, NaN payloads and -0.0
 *              included, and NaN or Inf in one channel never reaches a row that does not use it.  C == 1 uses m[0], bias[0] only.
 *   2 clamp    (white > 0)  t = v < 0 ? 0 : (v > white ? white : v): selects, so NaN stays NaN.
 *   3 curve    (gamma != 1) y = white * pow(t / white, gamma): IEEE division, pow(s, g) = exp2f(g * log2f(s)) with the device
 *              library's exp2f / log2f (the hardware exponential and logarithm with denormal scaling), pow(0, g) = 0 and
 *              pow(1, g) = 1 exactly, so t = 0 and t = white are fixed points.  No accuracy of these two functions is documented
 *              for this target; the one relied on is measured: |y - exact| <= K * (1 + g * |log2(t / white)|) * 2^-24 * |y| with
 *              K four times the worst ratio seen on an MI355X (tests/photometric_reference.py, profiles/photometric_err.txt).
 *              Only images whose record (or whose partner's record) has gamma != 1 execute it.
 *   4 MixUp    out_i = lambda == 1 ? P_i(src_i) : (lambda * P_i(src_i)) + ((1 - lambda) * P_p(src_partner)), 1 - lambda formed
 *              in fp32, P_p under the PARTNER's own record: a mixed image blends two finished images.  With lambda == 1 the
 *              partner is not read.  The payload of a NaN that goes through arithmetic (stages 1 with a product or sum, 3, 4) is
 *              the hardware's; that it is a NaN is guaranteed.
 * src, out: DEVICE float32 [n][c][h][w], c = 1 or 3, any h, w >= 1 (h * w < 2^31 - 8), 4-byte aligned; the ranges must not
 * overlap (output i reads images i and partner: the pass cannot run in place).  records: HOST array of n records, validated
 * before any launch (Y3_EINVAL + message: null pointer; bad c, n, h, w; misaligned or overlapping src / out; a non-finite
 * coefficient, bias, gamma, white or lambda; gamma <= 0; white < 0; white == 0 with gamma != 1; lambda outside [0, 1]; lambda < 1
 * with partner outside [0, n)) and handed to the kernel as kernel arguments, 16 output images per launch (each with its
 * partner's operator beside its own).  One thread per 16-byte-aligned group of four pixels of `out` and all their channel planes
 * when h * w is a multiple of 4 (16-byte loads at 4-byte alignment, aligned 16-byte stores, the partial first and last group of
 * a plane float by float), one pixel per thread otherwise; every output element is written by exactly one thread: no atomics,
 * no workspace, the same bits on every launch. */
typedef struct y3_photo_record {   /* 64 bytes, one per OUTPUT image */
    float   m[9];      /* colour matrix, row-major: out channel k = m[3k+0]*c0 + m[3k+1]*c1 + m[3k+2]*c2 (+ bias[k]); C == 1 uses m[0], bias[0] only */
    float   bias[3];
    float   gamma;     /* 1 = no tone curve */
    float   white;     /* > 0: clamp to [0, white] after the matrix and scale the tone curve by it; 0: no clamp, gamma must be 1 */
    int32_t partner;   /* MixUp source image in [0, n); ignored when lambda == 1 */
    float   lambda;    /* in [0, 1]; 1 = no MixUp */
} y3_photo_record;
int y3_photometric_batch(const float* src, int n, int c, int h, int w, const y3_photo_record* records_host, float* out,
                         y3_stream_t stream);

/* ---- letterbox front end of inference: images of any size into the network frame and the boxes back (opt-in, not in the
 * reference: inference.py / evaluate.py --letterbox, YoloV3.predict_letterbox) --------------------------------------
 * A ragged batch of 1 <= n <= Y3_LETTERBOX_MAX_IMAGES images lies in ONE device buffer src (16-byte aligned), image i densely
 * packed [src_h][src_w][c] at byte src_offset (a multiple of 16), dtype 0 = uint8, 1 = uint16, 2 = float32 (as y3_tile_gather),
 * c = 1 or 3.  records: HOST array, validated before any launch and handed to the kernels as kernel arguments.  Image i is
 * resampled to new_h x new_w (yolo3/letterbox.py letterbox_record: aspect ratio kept, rounded, at least 1, enlarged when smaller
 * than the frame) and placed at rows pad_y .., columns pad_x .. of the H x W frame.
 *
 * Resampling: separable, triangle filtered -- the function of torch's interpolate(mode='bilinear', antialias=True,
 * align_corners=False).  One axis, in -> out, in / out = a / b in lowest terms, D = 2 max(a, b); for output o:
 *   taps      j = lo .. hi-1, lo = max(0, floor((a (2o+1) - D + b) / (2b))), hi = min(in, floor((a (2o+1) + D + b) / (2b)))
 *             (= int(ctr - u + 0.5), int(ctr + u + 0.5) for ctr = (in / out)(o + 0.5), u = max(in / out, 1)), exact integers
 *   weight    wn_j = max(0, D - |(2j+1) b - (2o+1) a|), an integer <= 65536: D times the triangle max(0, 1 - |(j - ctr + 0.5) / u|)
 *   value     (sum over j ascending, wn_j > 0, of fl(fl(wn_j) * fl(v_j))) / fl(sum wn_j)          -- fp32, -ffp-contract=off
 * first along x for every source row (the taps of a row, ascending, for each channel), then along y over the reduced rows,
 * ascending.  fl(wn_j) and fl(sum wn_j) are exact (the sum is < 2^24 inside the limits below); the first product starts the sum
 * (nothing is added to zero).  A tap of weight zero is never read.  Hence in == out is an exact copy (uint8 / uint16 -> float32
 * exactly; a float NaN reaches only its own pixel) and a reduction by exactly 2 weighs 1, 3, 3, 1 over 8.  With Tx, Ty non-zero
 * taps on the two axes, |out - exact| <= (Tx + Ty + 3) 2^-24 sum |wy wx tap|.
 * Limits: source and frame sides 1 .. 32768; src / new <= 64 on each axis.  Refused with Y3_EINVAL + message, nothing launched:
 * those, a null pointer, bad dtype / c / n, new_* < 1, negative padding, pad + new beyond the frame, a misaligned src or offset.
 *
 * The resample kernel: one 256-thread workgroup per band of 8 output rows and group of 256 output elements (column x channel) of
 * one image, one element per thread.  A source row is read from memory once per workgroup whose filter reaches it: once per band
 * and per element group (neighbouring bands, and the groups of a band, share the filter support only).  It is read as 16-byte
 * slots from the 16-byte boundary below its first needed byte, whatever the row's own alignment; the last slot of an image is
 * read byte-wise up to the image's end.  The slots go through double-buffered LDS stages of 16 KiB that hold as many whole rows
 * as fit (their loads are in flight together) or one chunk of a longer row, so a row of any length works.  Each thread reduces
 * the taps of its output element from LDS, carries the partial sum across the chunks of a long row, and keeps the band's 8
 * partial sums in registers.  No [src_h][new_w] intermediate, no atomics, each output element written by one thread: the same
 * bits on every launch.
 *
 * y3_letterbox_batch: out float32 [n][c][H][W] = the un-normalised frame: the content at [pad_y, pad_y + new_h) x [pad_x,
 * pad_x + new_w), `fill` (any bits, NaN included) everywhere else.
 * y3_letterbox_zscore_nhwc: the network's NHWC input directly.  dst->n == n, H = dst->h, W = dst->w; dst->c >= c and a multiple
 * of 4, dst->ld >= dst->c and a multiple of 4, dst->ptr 16-byte aligned (refused as y3_tta_views_nhwc refuses them).  The content
 * values are those of y3_letterbox_batch bit for bit (staged in the workspace), z-scored per image over the CONTENT only: sum and
 * sum of squares in fp64 over the content as a [c][new_h][new_w] tensor in y3_zscore's partition (128 x 256 strided partials, the
 * same tree), then mean = s / count, var = max(0, q / count - mean^2), mu = (float)mean, sd = (float)sqrt(var),
 * out = sd <= 1 ? x - mu : (x - mu) / sd -- the expressions of y3_zscore.  Padding pixels are 0 (the content mean); channels
 * c .. dst->c - 1 are 0, as y3_nchw_to_nhwc writes them; the floats of a pixel beyond dst->c are not touched.  Pixels are stored
 * 16 bytes at a time.  workspace: y3_letterbox_workspace_bytes(n, H, W, c) bytes, 16-byte aligned.
 * y3_letterbox_unmap: rows [n][nb][ld] decode rows (corners x0, y0, x1, y1 first) of frame i -> image i's own pixels, in place:
 *   x <- (x - (float)pad_x) * sx,  y <- (y - (float)pad_y) * sy,   sx = (float)((double)src_w / new_w), sy likewise
 * one fp32 subtraction, then one fp32 multiplication (no contraction); with clip = 1 then v < 0 ? 0 : v > lim ? lim : v for
 * lim = (float)src_w or (float)src_h (a NaN stays).  Columns 4 .. ld-1 are not touched.  Needs no frame: the records' offsets and
 * the scale limit are not looked at. */
#define Y3_LETTERBOX_MAX_IMAGES 16
typedef struct y3_letterbox_record {
    uint64_t src_offset;      /* byte offset of this image in src; a multiple of 16 */
    int32_t  src_h, src_w;    /* its size; the image is [src_h][src_w][c], densely packed */
    int32_t  new_h, new_w;    /* content size in the frame */
    int32_t  pad_y, pad_x;    /* top / left padding */
} y3_letterbox_record;        /* 32 bytes */
int y3_letterbox_batch(const void* src, int dtype, int c, int n, const y3_letterbox_record* records, int H, int W,
                       float fill, float* out /* [n][c][H][W] */, y3_stream_t stream);
int y3_letterbox_zscore_nhwc(const void* src, int dtype, int c, int n, const y3_letterbox_record* records,
                             const y3_tensor* dst /* the network's NHWC input */, void* workspace, y3_stream_t stream);
size_t y3_letterbox_workspace_bytes(int n, int H, int W, int c);
int y3_letterbox_unmap(float* rows, int n, int nb, int ld, const y3_letterbox_record* records, int clip, y3_stream_t stream);

/* ---- ground-truth label tensors: ImageReader.__format_boxes (imagereader.py:252-324) on the device ------------------------
 * For ImageReader(..., label_device='gpu') and multi-scale training: the boxes of a batch cross PCIe, the three
 * label tensors are built where the loss reads them.  boxes: DEVICE int32 [n][max_boxes][5] = x, y, w, h, class with (x, y) the
 * top-left corner (what format_boxes takes); counts: DEVICE int32 [n], image i uses boxes[i][0 .. counts[i]) (clamped to
 * 0 .. max_boxes; boxes may be null when max_boxes == 0).  out1 / out2 / out3: float32 [n][G][G][A][5+K] for strides 32 / 16 / 8 of
 * an img_h x img_w image (multiples of 32); every element is written by this one launch, zeros included.
 * Bit-identical to format_boxes per image: box centre floor(xy + (wh - 1) / 2); best anchor by the IoU of co-centred (w, h) with
 * np.argmax's first-maximum rule, written at the SAME anchor slot of all three scales (Q5); row = [cx, cy, w, h, 1, one-hot];
 * boxes that share a cell and anchor behave like the host's sequential loop (coordinates of the last box in input order, the class
 * bits of all of them).  The cell index is the float32 evaluation floor((c / size) * G) of imagereader.py:309-310 as NumPy >= 2
 * performs it (IEEE float32 division, then float32 multiplication), NOT c / stride: they differ, e.g. size 352, stride 16, centre
 * 208 -> cell 12.  A box whose cell or class falls outside the tensor (the host loop raises or wraps there) writes nothing.
 * Deterministic: no atomics, each output word is owned by one workgroup.  No workspace.  anchors_host: host [A][2] (w, h). */
int y3_format_labels(const int* boxes, const int* counts, int n, int max_boxes, const float* anchors_host, int num_anchors,
                     int num_classes, int img_h, int img_w, float* out1, float* out2, float* out3, y3_stream_t stream);

/* ---- opt-in per-scale anchor assignment: each anchor owned by one scale (not in the reference) --------------------
 * The reference puts every anchor on every scale (Q5).  YOLOv3 partitions them: anchor_scale_host, a HOST array [A], gives each
 * anchor's scale, 0 = stride 32 (coarse), 1 = stride 16, 2 = stride 8 (fine).  A_s is the number of anchors of scale s, an anchor's
 * SLOT its rank among the anchors of its scale in index order.  Every scale owns at least one anchor and 3 <= A <= 16; an entry
 * outside 0..2, an empty scale, or any argument its all-scales counterpart refuses: Y3_EINVAL + message, nothing launched.
 *
 * y3_format_labels_scales: y3_format_labels with out_s = float32 [n][G_s][G_s][A_s][5+K].  The arithmetic is y3_format_labels',
 * word for word (centre, IoU against ALL A anchors with the first maximum winning, the float32 cell index, no contraction); the
 * row is written only on the scale that owns the best anchor, at that anchor's slot.  So out_s equals y3_format_labels' tensor of
 * scale s with its anchor axis gathered at the anchors scale s owns, bit for bit, collisions included (coordinates of the last
 * box in input order, class bits of all).  Every output word is written by this one launch, zeros included; no atomics, each
 * word is owned by one workgroup (a run of whole cells, whose length follows A_s (5+K) and so differs per scale).
 *
 * y3_decode_fwd_scales: y3_decode_fwd for three feature maps with fm[s].c == A_s (5+K) (ld >= c).  out: [N][Nb][5+K], rows run
 * scales coarse -> fine, then row, column, slot; Nb = sum of G_s^2 A_s.  Each row uses its own anchor's (w, h); the expression
 * order and the stride quirk Q6 are y3_decode_fwd's, so the rows equal y3_decode_fwd(nscales = 1) of each scale with that scale's
 * anchors in slot order.
 *
 * y3_truth_boxes_scales: the per-image box lists of y3_truth_boxes gathered from the three label tensors gt_s
 * [n][cells_anchors_s][d], coarse -> fine, each in index order (here a box lives on one scale only, so the fine tensor alone does
 * not hold the list).  One launch, one workgroup per image, the ordered append of y3_truth_boxes with its running base carried
 * across the tensors.  counts[i] is the TRUE total, also above cap; only the first cap boxes are stored. */
int y3_format_labels_scales(const int* boxes, const int* counts, int n, int max_boxes, const float* anchors_host,
                            const int* anchor_scale_host, int num_anchors, int num_classes, int img_h, int img_w,
                            float* out1, float* out2, float* out3, y3_stream_t stream);
int y3_decode_fwd_scales(const y3_tensor* fm, const float* anchors_host, const int* anchor_scale_host, int num_anchors,
                         int num_classes, int img_h, int img_w, float* out, y3_stream_t stream);
int y3_truth_boxes_scales(const float* gt1, const float* gt2, const float* gt3, int n, long long cells_anchors1,
                          long long cells_anchors2, long long cells_anchors3, int d, float* boxes, int* counts, int cap,
                          y3_stream_t stream);

/* ---- anchor fitting: P candidate anchor sets scored against n box sizes (opt-in, not in the reference: yolo3/anchors.py,
 * find_anchor_sizes.py --metric iou, train.py --auto_anchors) -------------------------------------------------------
 * wh_dev: DEVICE int32 [n][2] = (w, h) in pixels, 8-byte aligned (16-byte loads are used at either alignment); cand_dev: DEVICE
 * float32 [P][k][2] = (w, h), positive and finite.  For every box and every set p: the IoU of the co-centred box and anchor, in
 * the fp32 arithmetic of y3_format_labels (min / max / product / (sum - inter) / IEEE quotient, no contraction); the best anchor is
 * the FIRST maximum (np.argmax: the slot y3_format_labels writes); the score is the integer q = rint(iou * 2^24) (to nearest even)
 * in [0, 2^24].  Every accumulated quantity is an integer, so the sums depend neither on the order nor on the grid: two calls give
 * the same bytes, and a NumPy restatement (yolo3.anchors.anchor_stats(device='cpu')) gives them too.
 *   per_anchor != 0: out[P][k][5] = count, sum w, sum h, sum q, count(q >= thr_q) over the boxes whose best anchor it is;
 *   per_anchor == 0: out[P][2]    = sum q, count(q >= thr_q) over all boxes;
 * followed in both modes by ONE more int64: the number of skipped boxes.  A box whose w or h lies outside [1, 65535] is skipped and
 * contributes nothing else.  labels_dev (nullable; P == 1 only): labels[i] = best anchor of box i, 255 for a skipped box.
 * out_dev (8-byte aligned) need not be zeroed.  workspace: y3_anchor_stats_workspace_bytes(P, k) bytes, 8-byte aligned: one
 * partial row per workgroup, added up by a second launch (no float atomics, no global atomics).
 * The grid: a workgroup takes Y3_ANCHOR_BLOCK_BOXES boxes per pass, at most Y3_ANCHOR_MAX_BLOCKS workgroups run, so n above
 * Y3_ANCHOR_MAX_BLOCKS * Y3_ANCHOR_BLOCK_BOXES makes the workgroups stride.
 * Y3_EINVAL + message, nothing launched: k outside 1..Y3_ANCHOR_MAX_K (the 16 anchors the loss and decode take), P < 1, P * k > Y3_ANCHOR_MAX_CANDIDATES, n outside
 * 1..2^31-1, thr_q outside 0..2^24, labels_dev with P != 1, a null or misaligned pointer.  (The workspace query returns 0 for a
 * refused shape.) */
#define Y3_ANCHOR_MAX_K 16
#define Y3_ANCHOR_MAX_CANDIDATES 1024
#define Y3_ANCHOR_BLOCK_BOXES 512
#define Y3_ANCHOR_MAX_BLOCKS 512
size_t y3_anchor_stats_workspace_bytes(int P, int k);
int y3_anchor_stats(const int* wh_dev, long long n, const float* cand_dev, int P, int k, int thr_q, int per_anchor,
                    long long* out_dev, unsigned char* labels_dev, void* workspace, y3_stream_t stream);

/* ---- detection accuracy: matching + 101-point AP (not in the reference; yolo3/metrics.py, evaluate.py) ----
 * Detections are the keep lists of y3_nms_per_class: per (image, class) segment s = img * K + c the first
 * min(keep_cnt[s], max_keep, max_det) entries of keep_idx / keep_score, in keep order (descending score, ties: higher row
 * index).  A segment's pool entries start at offsets[s] (exclusive prefix over the segments, image-major) and run in keep
 * order, so the pool order is (image, class, keep rank) and does not depend on how the images were batched.
 *
 * y3_eval_offsets: offsets[0..nseg) = that prefix, offsets[nseg] = the total (the one count the host reads per batch to
 * size the pool).  One workgroup. */
int y3_eval_offsets(const int* keep_cnt, int nseg, int max_keep, int max_det, int* offsets, y3_stream_t stream);
/* y3_eval_match: rows [n, nb, ld floats] with corners x0,y0,x1,y1 first (the decode rows, ld = 5+K; or bare boxes, ld = 4),
 * clipped to [0,clip_w]x[0,clip_h] as y3_nms_per_class clips them (clip_w <= 0: no clip).  gt [n, max_gt, 5] = corners x0,y0,
 * x1,y1 + class (float), the first gt_cnt[i] rows valid.  max_gt_per_class: the host's bound on the GT boxes of one
 * (image, class); they are staged in LDS, at most 4096 (Y3_EINVAL + message above that, nothing launched).  Per segment
 * and threshold t (iou_thr_host: HOST array of num_thr in 1..32 values in (0, 1]): in keep order each detection takes the
 * unmatched GT box of its class with the largest IoU if that IoU >= t (IoU: y3_compute_iou's fp32 arithmetic, detection
 * first; equal IoU: the highest GT index) and is then a TP.  Writes, at pool position offsets[s] + j (< pool_capacity),
 * pool_key = (class << 32) | ~order_key(score) (int64; ascending = class ascending, score descending; order_key maps fp32
 * bits monotonically onto uint32) and pool_tp = TP mask (bit t).  One workgroup per segment, one wave per threshold. */
int y3_eval_match(const float* rows, int n, int nb, int ld, int num_classes, float clip_w, float clip_h, const int* keep_idx,
                  const int* keep_cnt, const float* keep_score, int max_keep, int max_det, const float* gt, const int* gt_cnt,
                  int max_gt, int max_gt_per_class, const float* iou_thr_host, int num_thr, const int* offsets,
                  long long* pool_key, unsigned* pool_tp, long long pool_capacity, y3_stream_t stream);
/* y3_eval_ap: keys / tp [m] = the pool stably sorted by key (so ties keep the (image, keep rank) order), npos [K] = GT boxes
 * per class.  Per (class c, threshold t): precision = tp_cum / (rank+1), its suffix maximum (envelope), AP = mean over
 * j = 0..100 of the envelope at the first rank with 100 tp_cum >= j npos (0 if none); npos == 0 -> AP and recall NaN.
 * ap, recall (final tp / npos), tp_count, fp_count: [K][T].  workspace: y3_eval_ap_workspace_bytes(m, num_thr). */
int y3_eval_ap(const long long* keys, const unsigned* tp, long long m, int num_classes, int num_thr, const int* npos,
               void* workspace, size_t workspace_bytes, float* ap, float* recall, int* tp_count, int* fp_count, y3_stream_t stream);
size_t y3_eval_ap_workspace_bytes(long long m, int num_thr);

/* ---- AP by area range, best-F1 score cuts and PR curves (opt-in: DetectionEvaluator(area_ranges=..., curves=...)) ----
 * y3_eval_match_ranges: y3_eval_match over num_ranges (1..8) closed area ranges [area_lo_host[a], area_hi_host[a]] (HOST
 * arrays of fp32, lo < hi, +-inf allowed, NaN refused).  A box's area is the fp32 product (x1 - x0) * (y1 - y0) of its corners (the
 * detection's after the clip).  Per segment, range a and threshold t, in keep order, among the unmatched GT boxes of the class
 * with IoU >= t: the detection takes the in-range box of largest IoU (ties: highest GT index) and is a TP; else the
 * out-of-range box of largest IoU (same tie rule), which is consumed, and is IGNORED; with no such box it is ignored if its own
 * area is out of range, else an FP.  pool_tp / pool_ign are entry-major [pool_capacity][num_ranges] words: bit t of word
 * [offsets[s] + j][a]; pool_key as y3_eval_match.  Same launch shape, LDS cap (4096 GT per (image, class)) and refusals as
 * y3_eval_match; the waves walk the num_ranges * num_thr pairs. */
int y3_eval_match_ranges(const float* rows, int n, int nb, int ld, int num_classes, float clip_w, float clip_h, const int* keep_idx,
                         const int* keep_cnt, const float* keep_score, int max_keep, int max_det, const float* gt, const int* gt_cnt,
                         int max_gt, int max_gt_per_class, const float* iou_thr_host, int num_thr, const float* area_lo_host,
                         const float* area_hi_host, int num_ranges, const int* offsets, long long* pool_key, unsigned* pool_tp,
                         unsigned* pool_ign, long long pool_capacity, y3_stream_t stream);
/* y3_eval_ap_ranges: keys [m], tp / ign [m][A] = the pool stably sorted by key, npos [K][A] = in-range GT boxes.  Per (class c,
 * range a, threshold t) over the entries whose ignore bit is clear, ranked as y3_eval_ap ranks them: ap, recall, tp_count,
 * fp_count as y3_eval_ap, ign_count = ignored entries; the best-F1 cut: among the cuts k (first k ranked entries kept) that do not
 * split a run of equal scores, the one of largest F1 = 2 TP(k) / (k + npos) (fp64; ties: smallest k): best_n = k, best_tp =
 * TP(k), best_score = score of entry k (0, 0, NaN without entries or without GT).  Optional (null: skipped) pr_precision /
 * pr_score [K][A][T][101]: the envelope precision at recall j / 100 (the 101 terms of the AP) and the score of the entry at
 * which that recall is first reached (NaN where it never is; both NaN where npos == 0).  All other outputs [K][A][T].
 * workspace: y3_eval_ap_ranges_workspace_bytes(m, num_ranges, num_thr). */
int y3_eval_ap_ranges(const long long* keys, const unsigned* tp, const unsigned* ign, long long m, int num_classes, int num_ranges,
                      int num_thr, const int* npos, void* workspace, size_t workspace_bytes, float* ap, float* recall, int* tp_count,
                      int* fp_count, int* ign_count, int* best_n, int* best_tp, float* best_score, float* pr_precision, float* pr_score,
                      y3_stream_t stream);
size_t y3_eval_ap_ranges_workspace_bytes(long long m, int num_ranges, int num_thr);

/* ---- per-class score cuts and the confusion matrix (opt-in: DetectionEvaluator(class_score_thresholds=..., confusion=True),
 * bbox_utils.cut_keep_lists) ----
 * y3_keep_cut: keep lists as y3_nms_per_class writes them, nseg = images * num_classes segments.  For segment s of class
 * c = s % num_classes, with m = min(max(keep_cnt[s], 0), max_keep): keep_cnt[s] = the length of the longest prefix j < m with
 * keep_score[s * max_keep + j] >= class_thr[c] (fp32 compare; class_thr: DEVICE array of num_classes values, finite or -inf, which
 * the host validates: -inf leaves the count at m, a NaN would keep nothing).  In keep order the scores do not increase, so the
 * prefix is every entry at or above the cut; the kernel itself relies on the prefix rule alone.  Writes keep_cnt only.  One
 * wave per segment, no atomics. */
int y3_keep_cut(const float* keep_score, int* keep_cnt, int nseg, int num_classes, int max_keep, const float* class_thr,
                y3_stream_t stream);
/* y3_eval_confusion: rows, clip, keep lists, max_det, gt, gt_cnt, max_gt, iou_thr_host and offsets as y3_eval_match; total =
 * offsets[n * num_classes].  Per image the admitted entries of all classes are put in one pooled order (score descending, fp32;
 * ties: lower class first, then keep rank; the keep lists' scores must not increase) and per threshold t, in that order, a
 * detection takes the unmatched GT box OF ANY CLASS with the largest IoU if that IoU >= t (y3_eval_match's arithmetic and tie
 * rule: the highest GT index).  confusion [num_thr][K + 1][K + 1] (int64, rows true, columns predicted, index K = background) is
 * ADDED to: [t][g][p] += 1 for a detection of class p on a box of class g, [t][K][p] += 1 for an unmatched detection,
 * [t][g][K] += 1 for a GT box left unmatched; [t][K][K] is never touched.  Integer atomics: two launches give the same bytes.
 * max_gt_per_image: the host's bound on the GT boxes of one image; all of them are staged in LDS (24 B each), at most 4096
 * (Y3_EINVAL + message above that, nothing launched).  workspace: y3_eval_confusion_workspace_bytes(total) (may be null for
 * total 0).  One workgroup per image, one wave per threshold, behind a small kernel that ranks the entries. */
int y3_eval_confusion(const float* rows, int n, int nb, int ld, int num_classes, float clip_w, float clip_h, const int* keep_idx,
                      const int* keep_cnt, const float* keep_score, int max_keep, int max_det, const float* gt, const int* gt_cnt,
                      int max_gt, int max_gt_per_image, const float* iou_thr_host, int num_thr, const int* offsets, long long total,
                      void* workspace, size_t workspace_bytes, long long* confusion, y3_stream_t stream);
size_t y3_eval_confusion_workspace_bytes(long long total);

/* ---- gradient exchange: tf.distribute.MirroredStrategy's all-reduce (train.py:38-39, model.py:500,510-515) -------
 * One process per GPU; SUM over the replicas (the loss is already divided by the global batch, model.py:492).  RCCL over
 * xGMI underneath (librccl.so is opened on first use).  Rank 0 calls y3_comm_unique_id and hands the 128 bytes to the
 * other ranks out of band; every rank then calls y3_comm_init with its HIP device current.  The Python host issues the
 * same collective through torch.distributed (backend "nccl" = RCCL) by default and through these entry points with
 * yolo3.parallel.DataParallel(transport='native') / Y3_DP_TRANSPORT=native (the torch group then only carries the id).
 * Exercised so far with ONE-rank communicators only (the builder's boxes have one GPU and RCCL refuses two ranks on
 * one device): N > 1 is first run by the driver's multi-GPU bench, with the default torch transport.
 * y3_comm_info: what the communicator itself reports -- ncclCommCount and ncclGetVersion (-1 where the symbol is missing). */
int y3_comm_unique_id(void* id128);
int y3_comm_init(const void* id128, int nranks, int rank, void** comm);
int y3_allreduce_sum_f32(void* comm, float* buf, size_t count, y3_stream_t stream); /* in place, asynchronous on stream */
int y3_comm_info(void* comm, int* nranks, int* version);
int y3_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* YOLO3HIP_H */

/*
 * sfvos.h -- C ABI of libsfvos.so: hand-written HIP (gfx950 / CDNA4) kernels for the
 * SlowFastLayers hot path of ChantalMP/Applying-SlowFast-networks-to-video-object-segmentation.
 *
 * The reference has no FFI layer; its boundary is the nn.Module surface of
 * `SlowFastLayers` (reference code/helpers/model.py:30-165).  The Python host
 * (sfvos_amd.SlowFastLayers) mirrors that surface and binds exactly the entry
 * points below through ctypes.  Each entry point names the
 * reference lines whose ATen dispatch it replaces.
 *
 * Conventions:
 *   - plain C; raw DEVICE pointers + explicit dims/strides; no torch types;
 *   - no allocation, no ownership transfer, no implicit device sync: every byte of
 *     workspace is caller-provided, every launch goes to the caller's hipStream_t;
 *   - re-entrant per stream, no thread-local or global mutable state except the
 *     per-thread last-error string;
 *   - return 0 on success, a negative SFVOS_E_* code otherwise; sfvos_last_error()
 *     gives the message for the calling thread.
 *
 * Pyramid layout ("pyramid NDHWC").  temporally_enhance_features (model.py:151-165) runs the
 * same 8 conv+BN blocks on every FPN level; here ONE launch covers all levels.  An activation
 * with T frames over a pyramid of L levels (H_l x W_l pixels) and B clips is one buffer of
 * M = B*T*sum_l(H_l*W_l) positions, level-major:
 *     position(l,b,t,h,w) = B*T*sum_{l'<l}(H_l'*W_l') + ((b*T + t)*H_l + h)*W_l + w
 *     element (.., c)      at base + position*ld + c
 * `ld` >= C is the per-position pitch in ELEMENTS, so a producer can write into a channel slice
 * of a wider buffer (this is how torch.cat at model.py:115,162 is eliminated).  BatchNorm
 * statistics stay per level (the reference normalises each level's call separately).
 */
#ifndef SFVOS_H
#define SFVOS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sfvos_stream_t; /* hipStream_t */

enum { SFVOS_F32 = 0, SFVOS_BF16 = 1,
       SFVOS_FP8 = 2 /* OCP e4m3 operands; inference-only first step, see sfvos_conv_desc.dtype */,
       SFVOS_U8 = 3 /* bytes: a source dtype of sfvos_transform_image only */ };

enum {
  SFVOS_OK = 0,
  SFVOS_E_ARG = -1,     /* bad argument / unsupported shape */
  SFVOS_E_LAUNCH = -2,  /* HIP launch error */
  SFVOS_E_NODEV = -3    /* no gfx950 device */
};

#define SFVOS_MAX_LEVELS 8

typedef struct sfvos_pyramid {
  int n_levels;
  int h[SFVOS_MAX_LEVELS];
  int w[SFVOS_MAX_LEVELS];
} sfvos_pyramid;

/* How a flat run of positions splits into levels: m[l] = B*T*H_l*W_l. */
typedef struct sfvos_levels {
  int n_levels;
  int64_t m[SFVOS_MAX_LEVELS];
} sfvos_levels;

/* ABI revision: 100 = round 1; 200 = struct_size in sfvos_conv_desc, no `zeros` argument, sfvos_abi_sizes,
 * sfvos_add_inplace, sfvos_mse_loss / _grad, mask-head entry points; 201 = sfvos_bn_running argument of the BN-apply
 * calls, mask-branch training entry points, sfvos_pack_weights_batch, sfvos_pyramid_to_frames / sfvos_frames_to_pyramid;
 * 300 (round 3) = sfvos_roi_levels / sfvos_roi_align / sfvos_roi_align_bwd (+ workspace query); 301 =
 * sfvos_shift_frames / sfvos_shift_frames_stat_rows (first-layer reuse across consecutive training windows); 302 = the
 * box branch of roi_heads: sfvos_dense and its packers / gradients, sfvos_box_predictor, sfvos_fastrcnn_loss,
 * sfvos_box_decode / _encode, sfvos_detections; 303 = sfvos_relu_bwd takes any whole number of 16-byte chunks per row;
 * its twin for wide rows (the box head's) is removed; 304 = the region proposal network's filter: sfvos_rpn_select /
 * _decode / _nms (+ workspace query); 305 = the training targets of roi_heads: sfvos_roi_match, sfvos_roi_sample (+
 * workspace query), sfvos_mask_targets; 306 = the training call of the region proposal network: sfvos_rpn_match,
 * sfvos_rpn_sample, sfvos_rpn_loss (+ workspace query); 307 = the feature pyramid network: sfvos_fpn_lateral,
 * sfvos_fpn_pool; 308 = the ResNet-50 body: sfvos_conv2d (+ sfvos_conv2d_plan, sfvos_conv2d_workspace_bytes),
 * sfvos_body_stem, sfvos_maxpool3x3s2 (5 entry points; 94 in all); 309 = the image transform: sfvos_transform_image,
 * sfvos_transform_masks (96 in all). */
int sfvos_version(void);
/* sizes[0..n) = sizeof(sfvos_conv_desc), sizeof(sfvos_pyramid), sizeof(sfvos_levels), sizeof(sfvos_mse_table),
 * sizeof(sfvos_bn_running), sizeof(sfvos_pack_item), sizeof(sfvos_planar_level) as THIS library was compiled; returns
 * how many entries exist (7).  A binder compares them with its own mirrors of the structs once at load time (a short struct would make the
 * library read strides from whatever follows it). */
int sfvos_abi_sizes(int* sizes, int n);
const char* sfvos_last_error(void);
/* 0 when the current HIP device is a gfx950; SFVOS_E_NODEV otherwise. */
int sfvos_check_device(void);

/* ---- layout (one level per call: the caller's tensors are separate per level) ------------- */

/* Frames fp32 [T][C][H][W] addressed through explicit ELEMENT strides (the reference's
 * stack().transpose(1,2) view is non-contiguous, model.py:157-158) -> NDHWC dst[T][H][W][ld].
 * Never writes the source. */
int sfvos_frames_to_ndhwc(const float* src, int64_t stride_t, int64_t stride_c, int64_t stride_h,
                          int64_t stride_w, void* dst, int dtype, int T, int C, int H, int W, int ld,
                          sfvos_stream_t stream);

/* Same source -> the channel-group-major layout of sfvos_conv_desc.x_group_stride (bf16 only): element
 * (t,h,w,c) at dst + (c/32)*group_stride + ((t*H+h)*W+w)*32 + c%32; C a multiple of 32. */
int sfvos_frames_to_groups(const float* src, int64_t stride_t, int64_t stride_c, int64_t stride_h,
                           int64_t stride_w, void* dst, int dtype, int T, int C, int H, int W,
                           int64_t group_stride, sfvos_stream_t stream);

/* NDHWC src[M][ld] (first C channels) -> planar fp32 dst[C][M]. */
int sfvos_ndhwc_to_planar(const void* src, int dtype, float* dst, int64_t M, int C, int ld,
                          sfvos_stream_t stream);

/* planar fp32 src[C][M] -> NDHWC dst[M][ld]. */
int sfvos_planar_to_ndhwc(const float* src, void* dst, int dtype, int64_t M, int C, int ld,
                          sfvos_stream_t stream);

/* NDHWC src[T][H][W][ld] (first C channels) accumulated (+=) or stored into fp32 frames
 * [T][C][H][W] with explicit strides: the fused output of model.py:162 as the caller's NCHW
 * tensor, and the input gradient of model.py:157-158 (reference code/osvos/osvos_model.py:50,64). */
int sfvos_ndhwc_to_frames(const void* src, int dtype, float* dst, int64_t stride_t, int64_t stride_c,
                          int64_t stride_h, int64_t stride_w, int T, int C, int H, int W, int ld,
                          int accumulate, sfvos_stream_t stream);

/* The two passes above for EVERY level of a pyramid in ONE launch (SlowFastLayers hands its five fused maps / takes
 * their gradients level by level: five launches of a few microseconds become one).  Level l: planar fp32 tensor
 * [T][C][h][w] addressed through element strides <-> the level's T*h*w positions of a level-major NDHWC pyramid buffer
 * with pitch ld (levels in order, level l at position T * sum_{l' < l} h_l' w_l'). */
typedef struct sfvos_planar_level {
  float* ptr;
  int64_t stride_t, stride_c, stride_h, stride_w;
  int h, w;
} sfvos_planar_level;
int sfvos_pyramid_to_frames(const void* src, int dtype, const sfvos_planar_level* levels, int n_levels, int T, int C,
                            int ld, int accumulate, sfvos_stream_t stream);
int sfvos_frames_to_pyramid(const sfvos_planar_level* levels, int n_levels, void* dst, int dtype, int T, int C, int ld,
                            sfvos_stream_t stream);

/* ---- weights ------------------------------------------------------------------------- */

/* Bytes of a packed weight image for a conv with these dims (same for fwd and dgrad packs). */
size_t sfvos_packed_weight_bytes(int dtype, int c_out, int c_in, int kt, int taps);

/* fp32 nn.Conv3d weight w[Cout][Cin][kt][kh][kw] (taps = kh*kw = 9 or 1; state-dict layout,
 * SURVEY.md 8b) -> the MFMA B-operand image consumed by sfvos_conv3d (forward). */
int sfvos_pack_weights_fwd(const float* w, void* packed, int dtype, int c_out, int c_in, int kt, int taps,
                           sfvos_stream_t stream);

/* Same weight -> the image for the data-gradient conv: channels swapped, all three kernel axes
 * flipped.  Feeding it to sfvos_conv3d with pad_t = kt-1 computes aten::convolution_backward's
 * grad_input. */
int sfvos_pack_weights_dgrad(const float* w, void* packed, int dtype, int c_out, int c_in, int kt, int taps,
                             sfvos_stream_t stream);

/* Several images in ONE launch (every layer of the model after an optimiser step): items[i] is one
 * sfvos_pack_weights_fwd (dgrad == 0) or sfvos_pack_weights_dgrad (dgrad != 0) call; 1 <= n <= SFVOS_MAX_PACK_ITEMS. */
#define SFVOS_MAX_PACK_ITEMS 16
typedef struct sfvos_pack_item {
  const float* w;
  void* packed;
  int c_out, c_in, kt, taps, dgrad;
} sfvos_pack_item;
int sfvos_pack_weights_batch(const sfvos_pack_item* items, int n, int dtype, sfvos_stream_t stream);

/* e4m3 operands (SFVOS_FP8).  Frames fp32 -> 64-channel groups of e4m3: element (t,h,w,c) = sat(src * scale) at byte
 * dst + (c/64)*group_stride + ((t*H+h)*W+w)*64 + c%64; C a multiple of 64.
 * sat(v), here and in the two calls below: v rounded to the nearest e4m3 value, ties to the even code; every finite
 * |v| > 448 and +-inf give +-448 (0x7e / 0xfe), never a NaN code; a NaN stays a NaN code (0x7f or 0xff); -0 keeps its
 * sign. */
int sfvos_frames_to_groups_fp8(const float* src, int64_t stride_t, int64_t stride_c, int64_t stride_h,
                               int64_t stride_w, void* dst, int T, int C, int H, int W, int64_t group_stride,
                               float scale, int* sat_count, sfvos_stream_t stream);
/* sat_count (device int, may be NULL): += number of elements with |src * scale| > 448 in fp32, +-inf included, NaN not
 * (they saturate silently in e4m3; FPN features are unbounded conv outputs, so a fixed scale must be checked against
 * the data). */

/* *amax (device float holding a non-negative value, e.g. 0) = max(*amax, max |src|) over the strided fp32 frames:
 * calibration of the e4m3 activation scale (scale = 448 / amax with head-room).  Order-independent, deterministic. */
int sfvos_frames_absmax(const float* src, int64_t stride_t, int64_t stride_c, int64_t stride_h, int64_t stride_w,
                        int T, int C, int H, int W, float* amax, sfvos_stream_t stream);

/* conv weight fp32 [c_out][c_in][kt][kh][kw] -> e4m3 forward image for sfvos_conv3d (dtype SFVOS_FP8), quantised per
 * output channel: weight_scale[n] = 448 / max|w[n]|.  bias_descale: [3][c_out] floats: row 0 = bias (zeros when bias is
 * NULL), row 1 = 1 / (act_scale * weight_scale[n]), row 2 = weight_scale[n] (sfvos_conv3d reads rows 0 and 1).
 * weight_scale[n] = 1 for an all-zero channel.  The image holds sat(w * weight_scale[n]) as defined above: a +-inf weight
 * makes its channel's scale 0 (every finite weight of the channel becomes 0, the infinite one NaN), a NaN weight stays
 * a NaN code.  c_in a multiple of 64. */
int sfvos_pack_weights_fp8(const float* w, const float* bias, void* packed, float* bias_descale, int c_out, int c_in,
                           int kt, int taps, float act_scale, sfvos_stream_t stream);

/* ---- convolution (replaces aten::convolution at model.py:112,120,124,132,136,144,147) ---- */

typedef struct sfvos_conv_desc {
  int struct_size; /* = sizeof(sfvos_conv_desc) of the binder's mirror; every entry point taking a desc rejects a mismatch */
  int dtype;       /* SFVOS_F32: f32 storage, exact-f32 MFMA; SFVOS_BF16: bf16 storage, f32 accumulate;
                    * SFVOS_FP8 (sfvos_conv3d only, forward 3x3 layers with c_in a multiple of 64): x and the weight image are OCP e4m3
                    * (x in 64-channel = 64-byte groups: x_group_stride > 0 counted in elements = bytes, or plain NDHWC
                    * with ld_x a multiple of 64), products on v_mfma_scale_f32_32x32x64_f8f6f4 (2x the bf16 rate),
                    * f32 accumulate, y stored as bf16; `bias` then points to [2][c_out] floats: row 0 the bias, row 1
                    * the per-output-channel de-quantisation factor 1/(activation scale * weight scale[n])
                    * (sfvos_pack_weights_fp8 writes both rows): y = acc * row1 + row0 */
  int batch;       /* clips B */
  int t_in;        /* input frames the conv sees: its window is frames [t_offset, t_offset + t_in) of the x buffer */
  int t_alloc;     /* frames per clip the x BUFFER holds.  Lets the slow pathway read its centre frames            */
  int t_offset;    /* (model.py:242-248) straight out of the fast clip's buffer.  Level-major x only: the window may
                    * stick out of [0, t_alloc) on either side (t_offset < 0, or t_offset + t_in > t_alloc); those
                    * frames are ZERO frames that are never read -- the reference's zero feature padding beyond the
                    * ends of a sequence (model.py:215-225) without materialising zeros */
  int c_in, c_out; /* multiples of 32 */
  int kt;          /* temporal taps */
  int taps;        /* 9 = 3x3 spatial, zero pad 1 ; 1 = 1x1 spatial, no pad */
  int pad_t;       /* zero frames each side in time: 0 (forward), kt-1 (data gradient) */
  int ld_x, ld_y;  /* per-position pitch of x / y in elements */
  int accumulate;  /* y += conv(x) instead of y = conv(x)  (gradient fan-in) */
  int relu;        /* y = max(conv(x) + bias, 0): the conv3x3 + ReLU blocks of the mask head (no statistics, no
                    * accumulate with it) */
  sfvos_pyramid pyr; /* spatial extents of the levels (stride 1: output spatial == input spatial) */
  int64_t x_group_stride; /* 0: x is pyramid NDHWC with pitch ld_x.  > 0 (bf16 only): x is stored as 64-byte
                           * channel groups, element (position, c) at (c/32)*x_group_stride + position*32 + c%32
                           * (ld_x ignored): every 128-byte line a kernel touches is used whole, so the
                           * temporal re-reads of the input hit in L2 instead of fetching half-used lines. */
  int64_t x_frame_stride; /* 0: x is level-major (all t_alloc frames of a level are consecutive).  > 0: x is a
                           * FRAME-major ring (sequence inference): frame t of every level sits at position
                           * t*x_frame_stride + B*sum_{l'<l} H_l'W_l' + (b*H_l+h)*W_l+w, so one frame of the whole
                           * pyramid is one contiguous slot; sfvos_conv3d only (no weight gradient). */
  int64_t y_frame_stride; /* the same for y: 0 level-major, > 0 frame-major (output frame t of every level at
                           * position t*y_frame_stride + ...): consecutive output frames are whole-pyramid slots. */
} sfvos_conv_desc;

/* Partial-statistics rows ([2][c_out] fp32 each, one per workgroup tile) sfvos_conv3d writes for
 * this desc: returns the total and, when rows_per_level != NULL, the count per level (rows are
 * level-major).  They are summed in fixed order by sfvos_bn_finalize -> deterministic. */
int sfvos_conv3d_stat_rows(const sfvos_conv_desc* d, int* rows_per_level);

/* y (=|+=) bias + sum_{dt,dh,dw,c} x[l][b][t_offset+t+dt-pad_t][h+dh-1][w+dw-1][c] * W over every level.
 * x: pyramid buffer with t_alloc frames; y: pyramid buffer with t_out = t_in + 2*pad_t - kt + 1 frames.
 * bias may be NULL.  stat_part may be NULL; otherwise it receives per-tile partial (sum, sum of
 * squares) of the values written.  Spatial / temporal zero padding is produced by the buffer descriptors' range
 * check (frames outside [0, t_in) and pixels outside the image are never read). */
int sfvos_conv3d(const sfvos_conv_desc* d, const void* x, const void* w_packed, const float* bias, void* y,
                 float* stat_part, sfvos_stream_t stream);

/* ---- window shift (SlowFastWindows: consecutive centre frames of the reference's training loop, model.py:316-374) ----
 * The pre-BatchNorm output of a first-layer conv depends only on the weights and the input frames, so the window one
 * centre frame later is the previous window's frames s .. T-1 followed by s new frames.  For every level l, clip b and
 * frame t of level-major pyramid buffers with pitch ld (first C channels):
 *     out[l][b][t] = prev[l][b][t + s]             t <  T - s
 *     out[l][b][t] = fresh[l][b][t - (T - s)]      t >= T - s   (fresh: a pyramid buffer of s frames, pitch ld)
 * stat_part (may be NULL): partial (sum, sum of squares) rows [rows][2][C] fp32 of the values written, level-major as
 * the rows of sfvos_conv3d_stat_rows, to be reduced by the BatchNorm finalize (fixed order, deterministic).
 * dtype f32 or bf16; C a multiple of 32, <= 256; 1 <= s < T; out must not overlap prev or fresh (never in place). */

/* Rows of stat_part for these dims: returns the total and, when rows_per_level != NULL, the count per level. */
int sfvos_shift_frames_stat_rows(const sfvos_pyramid* pyr, int B, int T, int C, int* rows_per_level);
int sfvos_shift_frames(const void* prev, const void* fresh, void* out, int dtype, const sfvos_pyramid* pyr, int B, int T,
                       int s, int C, int ld, float* stat_part, sfvos_stream_t stream);

/* ---- weight gradient (aten::convolution_backward grad_weight / grad_bias) -------------- */

/* Workspace bytes for sfvos_conv3d_wgrad (fp32 split-K slabs). `d` describes the FORWARD conv. */
size_t sfvos_conv3d_wgrad_workspace_bytes(const sfvos_conv_desc* d);

/* grad_w[Cout][Cin][kt][kh][kw] (fp32, state-dict layout) (=|+=) sum over levels/clips/pixels of
 * dy[pos][n] * x[pos+shift][c].  x is the forward input (pyramid buffer, ld_x, t_alloc/t_offset),
 * dy the gradient w.r.t. the conv output (pyramid buffer with t_out frames, ld_y).
 * accumulate != 0 adds into grad_w (model.py:369-374 accumulates two clips before stepping). */
int sfvos_conv3d_wgrad(const sfvos_conv_desc* d, const void* x, const void* dy, float* grad_w, int accumulate,
                       void* workspace, sfvos_stream_t stream);

/* ---- batch norm (aten::native_batch_norm / _backward at model.py:113,121,...,148) -------
 * Per-level coefficient tables: quantity q of level l lives at q_ptr + l*coef_stride (elements). */

/* Reduce the partial rows of each level (rows_per_level, level-major) in fixed order; train statistics
 * over count_per_level values per channel: mean, biased var -> rstd = 1/sqrt(var+eps),
 * scale = gamma*rstd, shift = beta - mean*scale, plus the unbiased variance for the running stats. */
int sfvos_bn_finalize(const float* part, int n_levels, const int* rows_per_level, const int64_t* count_per_level,
                      const float* gamma, const float* beta, float eps, int C, float* mean, float* rstd, float* scale,
                      float* shift, float* save_var_unbiased, int coef_stride, sfvos_stream_t stream);

/* Eval mode: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale; also
 * mean = running_mean, rstd = 1/sqrt(running_var+eps) (for an eval-mode backward); one level row. */
int sfvos_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, float eps, int C, float* mean, float* rstd, float* scale,
                         float* shift, sfvos_stream_t stream);

/* running = (1-momentum)*running + momentum*batch, applied for `n_updates` consecutive level rows
 * (means + l*coef_stride) in order: the reference updates once per FPN level (model.py:156-159);
 * num_batches_tracked (device int64 scalar, may be NULL) += n_updates. */
int sfvos_bn_running_update(float* running_mean, float* running_var, const float* means, const float* vars_unbiased,
                            int n_updates, int coef_stride, int C, float momentum, int64_t* num_batches_tracked,
                            sfvos_stream_t stream);

/* The running-statistics update of sfvos_bn_running_update folded into the BN-apply launch (its first workgroup does
 * it; one launch less per layer in training): means / vars_unbiased are coefficient-table rows, level l at
 * + l*coef_stride (the coef_stride of the apply call), n_updates consecutive rows applied in order. */
typedef struct sfvos_bn_running {
  float* running_mean;
  float* running_var;
  const float* means;
  const float* vars_unbiased;
  int64_t* num_batches_tracked; /* device int64 scalar += n_updates; may be NULL */
  int n_updates;
  float momentum;
} sfvos_bn_running;

/* y[m][0..C) = act(x[m][0..C) * scale_l + shift_l), act = ReLU when relu != 0 (model.py:114,122,...).
 * running (may be NULL): also update the running statistics (see sfvos_bn_running). */
int sfvos_bn_apply(const void* x, int ld_x, void* y, int ld_y, int dtype, const sfvos_levels* lv, int C,
                   const float* scale, const float* shift, int coef_stride, int relu, const sfvos_bn_running* running,
                   sfvos_stream_t stream);

/* The same with an e4m3 result (BASELINE config 5: the activation becomes the e4m3 operand of the next 3x3 conv):
 * y[m][c] = sat_e4m3(act(x*scale_l + shift_l) * act_scale); x bf16 with pitch ld_x (elements), y bytes with pitch ld_y;
 * C a multiple of 16; sat_count (device int, may be NULL) += values beyond +-448 before saturation (+-inf included, NaN
 * not).  sat_e4m3 is the sat() of sfvos_frames_to_groups_fp8: +-inf give +-448, a NaN stays a NaN code. */
int sfvos_bn_apply_fp8(const void* x, int ld_x, void* y, int ld_y, const sfvos_levels* lv, int C, const float* scale,
                       const float* shift, int coef_stride, int relu, float act_scale, int* sat_count,
                       const sfvos_bn_running* running, sfvos_stream_t stream);

/* Rows of partials sfvos_bn_bwd_reduce / _apply write for these levels (level-major). */
int sfvos_bn_bwd_rows(const sfvos_levels* lv);

/* Pass 1 of BN(+ReLU) backward: dz = dy * (relu ? (x*scale+shift > 0) : 1);
 * part[row] = (sum dz, sum dz * xhat), xhat = (x-mean)*rstd, [2][C] per row. */
int sfvos_bn_bwd_reduce(const void* dy, int ld_dy, const void* x, int ld_x, int dtype, const sfvos_levels* lv, int C,
                        const float* scale, const float* shift, const float* mean, const float* rstd, int coef_stride,
                        int relu, float* part, sfvos_stream_t stream);

/* Finish pass 1, all levels in parallel: per level the sums (sum_dz, sum_dzx: coefficient-table rows, level l at
 * + l*coef_stride) and the three coefficients of pass 2:  dx = A*dz + B*x + K.  train != 0: batch-stat backward; else
 * eval (A = gamma*rstd, B = K = 0). */
int sfvos_bn_bwd_finalize(const float* part, const sfvos_levels* lv, const float* gamma, const float* mean,
                          const float* rstd, int coef_stride, int C, int train, float* coefA, float* coefB,
                          float* coefK, float* sum_dz, float* sum_dzx, sfvos_stream_t stream);

/* Pass 2: dx[m][c] = A*dz + B*x + K (dz as in pass 1), stored as dtype with pitch ld_dx;
 * bias_part (may be NULL) receives per-block partial sums of dx: sfvos_bn_bwd_rows(lv) rows of [C];
 * dgamma / dbeta (may be NULL) (=|+=) the per-level sums of pass 1 added in level order:
 * dgamma = sum_l sum dz*xhat, dbeta = sum_l sum dz. */
int sfvos_bn_bwd_apply(const void* dy, int ld_dy, const void* x, int ld_x, void* dx, int ld_dx, int dtype,
                       const sfvos_levels* lv, int C, const float* scale, const float* shift, int coef_stride,
                       int relu, const float* coefA, const float* coefB, const float* coefK, float* bias_part,
                       const float* sum_dz, const float* sum_dzx, float* dgamma, float* dbeta, int accumulate,
                       sfvos_stream_t stream);

/* out[c] (=|+=) sum_rows part[row][c]   (bias gradient from sfvos_bn_bwd_apply partials). */
int sfvos_reduce_rows(const float* part, int rows, int C, float* out, int accumulate, sfvos_stream_t stream);

/* ---- optimiser (torch.optim.SGD as built at reference train.py:80) ---------------------- */

/* g' = g + wd*p ; buf = first_step ? g' : momentum*buf + g' ; p -= lr*buf   over n fp32 elements. */
int sfvos_sgd_step(float* p, const float* g, float* momentum_buf, int64_t n, float lr, float momentum,
                   float weight_decay, int first_step, sfvos_stream_t stream);

/* x[i] *= s  (gradient averaging after the data-parallel all-reduce). */
int sfvos_scale(float* x, int64_t n, float s, sfvos_stream_t stream);

/* dst[i] += src[i] over n elements of `dtype` (n a multiple of 8): gradient fan-in where two consumers read the same
 * frames -- the slow pathway's window of the input clip (model.py:242-248: its gradient adds into frames
 * [k, k+sp) of the fast clip's gradient). */
int sfvos_add_inplace(void* dst, const void* src, int dtype, int64_t n, sfvos_stream_t stream);

/* ---- stand-in training loss (bench / tests) ---------------------------------------------------
 * The reference's loss is the sum of torchvision's RoI-head losses (model.py:346-368; torchvision is absent here and
 * out of scope); the benchmark and the parity fixtures use  loss = sum_l mean((out_l - target_l)^2)  over the fused
 * maps out_l [B,256,H_l,W_l] fp32 (oracle/slowfast_ref.py proxy_loss).  Two launches: value, gradient. */
typedef struct sfvos_mse_table {
  int n;                                   /* tensors (FPN levels), 1..SFVOS_MAX_LEVELS */
  const float* out[SFVOS_MAX_LEVELS];      /* contiguous fp32, numel[l] elements */
  const float* target[SFVOS_MAX_LEVELS];
  float* grad[SFVOS_MAX_LEVELS];           /* written by sfvos_mse_loss_grad only (may be NULL for sfvos_mse_loss) */
  int64_t numel[SFVOS_MAX_LEVELS];
} sfvos_mse_table;

/* fp32 partial rows sfvos_mse_loss needs in `part` for this table. */
int sfvos_mse_loss_rows(const sfvos_mse_table* t);
/* loss[0] = sum_l (1/numel_l) sum_i (out_l[i] - target_l[i])^2, reduced in a fixed order (f64 accumulate). */
int sfvos_mse_loss(const sfvos_mse_table* t, float* part, float* loss, sfvos_stream_t stream);
/* grad_l[i] = upstream * 2 (out_l[i] - target_l[i]) / numel_l; upstream: device scalar (autograd's grad_output) or
 * NULL for 1. */
int sfvos_mse_loss_grad(const sfvos_mse_table* t, const float* upstream, sfvos_stream_t stream);

/* ---- mask branch behind RoIAlign (model.py:17-25 MaskRCNNPredictor(256, 256, 2), model.py:346-347) -----
 * torchvision's MaskRCNNHeads / MaskRCNNPredictor / maskrcnn_inference / paste_masks_in_image on RoI features
 * [N,256,14,14] (RoIAlign itself is torchvision, out of scope).  The four conv3x3 + ReLU blocks are sfvos_conv3d calls
 * (kt = 1, taps = 9, relu = 1, batch = N RoIs, one 14x14 "level"); the rest: */

/* ConvTranspose2d(Cin, Cout, 2, 2, 0) weight [Cin][Cout][2][2] fp32 -> packed image (4*Cin*Cout elements of dtype). */
int sfvos_pack_deconv2x2(const float* w, void* packed, int dtype, int c_in, int c_out, sfvos_stream_t stream);
/* y[n][2i+a][2j+b][co] = act(bias[co] + sum_ci x[n][i][j][ci] * w[ci][co][a][b]); x: NHWC [n][h][w][c_in], y: NHWC
 * [n][2h][2w][c_out], both `dtype`; act = ReLU when relu != 0 (conv5_mask + relu of MaskRCNNPredictor). */
int sfvos_deconv2x2_relu(const void* x, const void* w_packed, const float* bias, void* y, int dtype, int n, int h, int w,
                         int c_in, int c_out, int relu, sfvos_stream_t stream);
/* mask_fcn_logits (conv1x1 c -> num_classes, weight [num_classes][c] fp32) on x: NHWC [n][positions][c]:
 * logits (may be NULL): [n][num_classes][positions] fp32; prob (may be NULL): [n][1][positions] = sigmoid of the logit
 * of class labels[n] (maskrcnn_inference). */
int sfvos_mask_logits(const void* x, int dtype, const float* w, const float* bias, const int64_t* labels, int n,
                      int positions, int c, int num_classes, float* logits, float* prob, sfvos_stream_t stream);
/* paste_masks_in_image: masks [n][1][mask_size][mask_size] fp32, boxes [n][4] fp32 (x1,y1,x2,y2) -> out
 * [n][1][img_h][img_w] fp32: masks zero-padded by `padding`, boxes expanded by (mask_size + 2 padding) / mask_size
 * and truncated to integers, bilinear resize (align_corners = false) to the box, zero outside it. */
int sfvos_paste_masks(const float* masks, const float* boxes, int n, int mask_size, int padding, int img_h, int img_w,
                      float* out, sfvos_stream_t stream);

/* ---- MultiScaleRoIAlign in front of the mask branch (model.py:346: roi_heads' mask_roi_pool =
 * MultiScaleRoIAlign(['0','1','2','3'], output_size 14, sampling_ratio 2) on the fused maps SlowFastLayers returns).
 * rois: [n][5] fp32 (image index in the batch, x1, y1, x2, y2), image coordinates.  torchvision's arithmetic, restated
 * (parity unpinned by the reference: torchvision is neither vendored nor installed). ---- */

/* LevelMapper: levels[r] = clamp(floor(canonical_level + log2(sqrt(box area) / canonical_scale) + eps), k_min, k_max) - k_min
 * (device int32 per RoI; torchvision: canonical_scale 224, canonical_level 4, eps 1e-6, k_min / k_max = -log2 of the first /
 * last feature level's scale). */
int sfvos_roi_levels(const float* rois, int n, int k_min, int k_max, float canonical_scale, float canonical_level,
                     float eps, int* levels, sfvos_stream_t stream);

/* Bytes of `workspace` for n RoIs (per-RoI tables of the separable bilinear parameters). */
size_t sfvos_roi_align_workspace_bytes(int n);

/* torchvision.ops.roi_align(feat, rois, pooled, spatial_scale, sampling_ratio, aligned = False) for the RoIs r with
 * levels[r] == level (levels == NULL: all of them): feat [B][C][H][W] fp32 contiguous; out [n][C][pooled][pooled] fp32
 * (rows of other levels are left untouched); sampling_ratio >= 1 and pooled * sampling_ratio <= 64. */
int sfvos_roi_align(const float* feat, int B, int C, int H, int W, const float* rois, const int* levels, int level, int n,
                    float spatial_scale, int pooled, int sampling_ratio, void* workspace, float* out,
                    sfvos_stream_t stream);

/* Its backward: dfeat [B][C][H][W] (=|+=) the gradient of the level's RoIs (dout [n][C][pooled][pooled]); a gather in a
 * fixed order (deterministic; torchvision scatters with atomics).  n == 0 writes zeros (accumulate == 0). */
int sfvos_roi_align_bwd(const float* dout, int B, int C, int H, int W, const float* rois, const int* levels, int level,
                        int n, float spatial_scale, int pooled, int sampling_ratio, void* workspace, float* dfeat,
                        int accumulate, sfvos_stream_t stream);

/* ---- training side of the mask branch (the reference trains roi_heads: only backbone and RPN are frozen,
 * model.py:176-179; losses.backward() at model.py:369 runs through torchvision's maskrcnn_loss and these modules).
 * The 3x3 convs: sfvos_conv3d with a sfvos_pack_weights_dgrad image (data gradient) and sfvos_conv3d_wgrad. ---- */

/* ReLU backward + bias gradient partials: dz[m][c] = a[m][c] > 0 ? dy[m][c] : 0 (a == NULL: dz = dy; dz may alias dy or
 * be NULL); col_part (may be NULL, but not both it and dz): sfvos_relu_bwd_rows(m) rows of [c] fp32, row r = column
 * sums of dz over its 64 rows (sum them with sfvos_reduce_rows: the bias gradient of the conv or dense layer that
 * produced a).  dy, a, dz: [m][c] dtype; c: a whole number of 16-byte chunks (4 fp32 / 8 bf16 elements) up to 2^20. */
int sfvos_relu_bwd_rows(int64_t m);
int sfvos_relu_bwd(const void* dy, const void* a, void* dz, int dtype, int64_t m, int c, float* col_part,
                   sfvos_stream_t stream);

/* torchvision roi_heads.maskrcnn_loss behind the RoIAlign of the ground-truth masks:
 * loss[0] = mean_{n,p} BCEWithLogits(logits[n][labels[n]][p], targets[n][p]); logits [n][num_classes][positions] fp32,
 * targets [n][positions] fp32, labels int64; reduced in a fixed order (f64). */
int sfvos_mask_bce_loss(const float* logits, const int64_t* labels, const float* targets, int n, int num_classes,
                        int positions, float* loss, sfvos_stream_t stream);
/* dlogits[n][k][p] = k == labels[n] ? upstream * (sigmoid(logit) - target) / (n * positions) : 0;
 * upstream: device scalar (autograd's grad_output) or NULL for 1. */
int sfvos_mask_bce_loss_grad(const float* logits, const int64_t* labels, const float* targets, const float* upstream,
                             int n, int num_classes, int positions, float* dlogits, sfvos_stream_t stream);

/* Backward of mask_fcn_logits (conv1x1 c -> num_classes) and of the ReLU in front of it.  y: the deconv's post-ReLU
 * output, NHWC [n][positions][c] dtype; dlogits [n][num_classes][positions] fp32; w [num_classes][c] fp32.
 * dz[n][p][c] = (relu == 0 || y > 0) ? sum_k dlogits[n][k][p] w[k][c] : 0   (dtype, same shape as y);
 * part: sfvos_mask_logits_bwd_rows(n, positions) rows of [num_classes*c + num_classes + c] fp32 =
 * (grad of w | grad of the logits bias | column sums of dz = grad of the deconv bias) partials (sfvos_reduce_rows).
 * Each partial row covers 64 consecutive rows (n, p) of y.  c: a multiple of 64 up to 512; num_classes <= 8. */
int sfvos_mask_logits_bwd_rows(int n, int positions);
int sfvos_mask_logits_bwd(const void* y, int dtype, const float* dlogits, const float* w, int n, int positions, int c,
                          int num_classes, int relu, void* dz, float* part, sfvos_stream_t stream);

/* ConvTranspose2d(Cin, Cout, 2, 2, 0) backward.  Data gradient: weight [Cin][Cout][2][2] fp32 -> packed image, then
 * dx[n][i][j][ci] = sum_{a,b,co} dz[n][2i+a][2j+b][co] w[ci][co][a][b]; dz NHWC [n][2h][2w][c_out], dx NHWC
 * [n][h][w][c_in], both dtype. */
int sfvos_pack_deconv2x2_dgrad(const float* w, void* packed, int dtype, int c_in, int c_out, sfvos_stream_t stream);
int sfvos_deconv2x2_dgrad(const void* dz, const void* w_packed, void* dx, int dtype, int n, int h, int w, int c_in,
                          int c_out, sfvos_stream_t stream);
/* Weight gradient: grad_w[ci][co][a][b] (fp32, state-dict layout) (=|+=) sum_{n,i,j} x[n][i][j][ci] dz[n][2i+a][2j+b][co]
 * (exact-f32 MFMA, fixed-order split reduction); workspace: sfvos_deconv2x2_wgrad_workspace_bytes. */
size_t sfvos_deconv2x2_wgrad_workspace_bytes(int n, int h, int w, int c_in, int c_out);
int sfvos_deconv2x2_wgrad(const void* x, const void* dz, int dtype, int n, int h, int w, int c_in, int c_out,
                          float* grad_w, int accumulate, void* workspace, sfvos_stream_t stream);

/* ---- box branch of roi_heads (model.py:346: box_roi_pool -> box_head = TwoMLPHead(12544, 1024) -> box_predictor =
 * FastRCNNPredictor(1024, 2) -> fastrcnn_loss | postprocess_detections; model.py:347: transform.postprocess resizes the
 * boxes).  torchvision's arithmetic, restated from its published sources (parity unpinned by the reference: torchvision
 * is neither vendored nor installed).  No atomics on data: every result is bit-identical from run to run. ---- */

/* Dense layer y[m][n] = act(x[m][k] . W^T + bias): x, y row-major `dtype`, w_packed the image sfvos_pack_dense_fwd makes
 * of nn.Linear's weight [n_out][k_in] fp32; act = ReLU when relu != 0; bias (fp32, may be NULL).  n and k: multiples of
 * 32.  The same call with the image of sfvos_pack_dense_dgrad (sizes swapped: n = k_in, k = n_out), bias NULL, relu 0 is
 * the data gradient dx[m][k_in] = dz[m][n_out] . W.  positions (HW) > 1: the k_in columns of the state-dict weight are
 * (c, p)-ordered (torchvision flattens NCHW RoI features, column c*HW + p) while the rows of x / dx are channels-last
 * (column p*C + c, C = k_in / HW); the images carry that permutation.  fc6: positions = 49.
 * K is split into sfvos_dense_splits(dtype, m, n, k) fp32 slabs in `workspace` (sfvos_dense_workspace_bytes, may be
 * NULL when that is 0), summed in a fixed order by a second launch that applies bias, ReLU and the store's rounding. */
int sfvos_pack_dense_fwd(const float* w, void* packed, int dtype, int n_out, int k_in, int positions,
                         sfvos_stream_t stream);
int sfvos_pack_dense_dgrad(const float* w, void* packed, int dtype, int n_out, int k_in, int positions,
                           sfvos_stream_t stream);
int sfvos_dense_splits(int dtype, int m, int n, int k);
size_t sfvos_dense_workspace_bytes(int dtype, int m, int n, int k);
int sfvos_dense(const void* x, const void* w_packed, const float* bias, void* y, int dtype, int m, int n, int k, int relu,
                void* workspace, sfvos_stream_t stream);
/* grad_w[n][k] (fp32, state-dict layout and column order) (=|+=) sum_m dz[m][n] x[m][k']; x [m][k] (channels-last
 * columns when positions > 1), dz [m][n], both `dtype`; one exact-f32 MFMA chain over the m rows per output. */
int sfvos_dense_wgrad(const void* x, const void* dz, int dtype, int m, int n, int k, int positions, float* grad_w,
                      int accumulate, sfvos_stream_t stream);

/* FastRCNNPredictor: logits[m][num_classes] = x . w_cls^T + b_cls, deltas[m][4 num_classes] = x . w_box^T + b_box;
 * x [m][c] `dtype`, weights and outputs fp32; num_classes <= 8. */
int sfvos_box_predictor(const void* x, int dtype, const float* w_cls, const float* b_cls, const float* w_box,
                        const float* b_box, int m, int c, int num_classes, float* logits, float* deltas,
                        sfvos_stream_t stream);
/* Its backward and that of the ReLU that produced x (relu != 0): with g = (dlogits | ddeltas) [m][J], J = 5 num_classes,
 * w = (w_cls | w_box) [J][c]:  dz[m][c] = (relu == 0 || x > 0) ? sum_j g[m][j] w[j][c] : 0  (`dtype`);
 * part: sfvos_box_predictor_bwd_rows(m) rows of [J*c + J + c] fp32 = (grad of w | grad of the biases | column sums of
 * dz = bias gradient of the layer that produced x) over 64 rows each (sfvos_reduce_rows). */
int sfvos_box_predictor_bwd_rows(int m);
int sfvos_box_predictor_bwd(const void* x, int dtype, const float* dlogits, const float* ddeltas, const float* w_cls,
                            const float* w_box, int m, int c, int num_classes, int relu, void* dz, float* part,
                            sfvos_stream_t stream);

/* roi_heads.fastrcnn_loss on the n sampled RoIs: losses[0] = mean cross_entropy(logits [n][K], labels),
 * losses[1] = sum over the RoIs with label > 0 of smooth_l1(deltas[i][4 label .. +3] - targets[i][0..3], beta) / n
 * (torchvision: beta = 1/9); fixed-order f64 reduction.  A label outside [0, K) makes both losses NaN and its rows of
 * the gradient zero; nothing is read through it.  upstream: two device floats (grad of the two losses) or NULL for 1. */
int sfvos_fastrcnn_loss(const float* logits, const float* deltas, const int64_t* labels, const float* targets, int n,
                        int num_classes, float beta, float* losses, sfvos_stream_t stream);
int sfvos_fastrcnn_loss_grad(const float* logits, const float* deltas, const int64_t* labels, const float* targets,
                             const float* upstream, int n, int num_classes, float beta, float* dlogits, float* ddeltas,
                             sfvos_stream_t stream);

/* BoxCoder.decode of the classes [first_class, K) of each of the m RoIs (deltas [m][4K], proposals [m][4], weights
 * (wx, wy, ww, wh), dw / dh clamped at `clip`), clipped to the image when img_w > 0: boxes [m (K - first_class)][4];
 * scores (may be NULL; needs logits [m][K]) = softmax probability of the class, labels (may be NULL) = the class.
 * postprocess_detections: first_class = 1, weights (10, 10, 5, 5), clip = log(1000 / 16). */
int sfvos_box_decode(const float* logits, const float* deltas, const float* proposals, int m, int num_classes,
                     int first_class, float wx, float wy, float ww, float wh, float clip, float img_h, float img_w,
                     float* boxes, float* scores, int64_t* labels, sfvos_stream_t stream);
/* BoxCoder.encode_single: targets[m][4] of the reference boxes [m][4] against the proposals [m][4]. */
int sfvos_box_encode(const float* reference, const float* proposals, int m, float wx, float wy, float ww, float wh,
                     float* targets, sfvos_stream_t stream);

/* transform.resize_boxes: out[i] = (x1 ratio_w, y1 ratio_h, x2 ratio_w, y2 ratio_h) of boxes[i], n boxes. */
int sfvos_box_scale(const float* boxes, int n, float ratio_h, float ratio_w, float* out, sfvos_stream_t stream);

/* The rest of postprocess_detections on n candidates (boxes [n][4], scores [n], labels [n] int64): keep score >
 * score_thresh and both sides >= min_size, rank by descending score (ties: the lower index first), greedy NMS at IoU >
 * nms_thresh among candidates of the same label (batched_nms), the first max_det survivors.  count[0] = their number d;
 * out_* hold max_det entries, the first d in descending score: boxes (x scaled by ratio_w, y by ratio_h: resize_boxes),
 * scores, labels, out_index = the candidate's index, out_roi = out_index / classes_per_roi (the RoI it came from);
 * entries behind d are 0 / -1.  Meant for the few thousand candidates of one image (1000 proposals x (K - 1) classes): the
 * ranking counts over all pairs (n^2 steps) and the masks take n^2 / 8 bytes, so n <= 8192 and larger sets are refused;
 * workspace: sfvos_detections_workspace_bytes(n) (0 for a refused n). */
size_t sfvos_detections_workspace_bytes(int n);
int sfvos_detections(const float* boxes, const float* scores, const int64_t* labels, int n, int classes_per_roi,
                     float score_thresh, float min_size, float nms_thresh, int max_det, float ratio_h, float ratio_w,
                     void* workspace, int* count, float* out_boxes, float* out_scores, int64_t* out_labels,
                     int* out_index, int* out_roi, sfvos_stream_t stream);

/* ---- region proposal network (model.py:236-240, called at :329-335: torchvision's RegionProposalNetwork in inference,
 * frozen and under no_grad in the reference).  The head is two existing calls: sfvos_conv3d (3x3 256 -> 256 + ReLU, kt = 1,
 * one launch over the pyramid) and sfvos_box_predictor with num_classes = A anchors per position, which leave
 * objectness [positions][A] and deltas [positions][4A] fp32 in the pyramid's level-major order (T = 1), i.e. torchvision's
 * (h, w, a) flattening with segment (level l, image b) contiguous.  Segments are numbered s = l * batch + b.  The filter
 * below restates filter_proposals, AnchorGenerator and BoxCoder(1, 1, 1, 1) (parity unpinned by the reference).
 * Order everywhere: logit descending, ties by (level, anchor index) ascending; values compare as floats (-0 == +0, +-inf
 * are ordinary values) and a NaN ranks below every number (torch.topk ranks it above; it can never become a proposal
 * because its score fails the threshold).  Results are bit-identical from run to run.  Limits: pre_nms_top_n <= 4096
 * per level, A <= 8, SFVOS_MAX_LEVELS levels; anything beyond is refused. ---- */

/* Bytes of `workspace` of sfvos_rpn_nms; 0 for a refused size. */
size_t sfvos_rpn_workspace_bytes(int n_levels, int batch, int pre_nms_top_n);

/* Per segment: counts[s] = min(pre_nms_top_n, A H_l W_l) and index[s][0 .. counts[s]) = the anchor indices
 * ((h W_l + w) A + a) of the largest logits in the order above; index[s][counts[s] .. pre_nms_top_n) = -1.
 * counts: [n_levels * batch], index: [n_levels * batch][pre_nms_top_n] int32. */
int sfvos_rpn_select(const float* objectness, const sfvos_pyramid* pyr, int batch, int num_anchors, int pre_nms_top_n,
                     int* counts, int* index, sfvos_stream_t stream);

/* For every (segment, rank): anchor = base_anchors[l][a] + (w stride_w, h stride_h, w stride_w, h stride_h) with
 * stride_h = tensor_h / H_l, stride_w = tensor_w / W_l (integer division; tensor = the padded batch tensor), decoded with
 * its 4 deltas (dw, dh clamped at `clip` = log(1000 / 16)), clipped to the image's own size image_sizes[b] = (height,
 * width) (device floats [batch][2]); logits = the objectness logit, scores = its sigmoid; valid = both sides >= min_size
 * and score > score_thresh.  base_anchors: device floats [n_levels][A][4].  boxes [segments][pre_nms_top_n][4], logits,
 * scores, valid (int32) [segments][pre_nms_top_n]; ranks behind counts[s] are zeros. */
int sfvos_rpn_decode(const float* objectness, const float* deltas, const int* counts, const int* index,
                     const sfvos_pyramid* pyr, int batch, int num_anchors, int pre_nms_top_n, const float* base_anchors,
                     int tensor_h, int tensor_w, const float* image_sizes, float clip, float min_size, float score_thresh,
                     float* boxes, float* logits, float* scores, int* valid, sfvos_stream_t stream);

/* Greedy NMS at IoU > nms_thresh among the valid candidates of each segment, visited in rank order (a blocked scan: 64
 * candidates per step), then per image the survivors of all levels merged in the order above and the first
 * post_nms_top_n kept: out_boxes [batch][post_nms_top_n][4], out_scores, out_index (= l * pre_nms_top_n + rank of the
 * candidate) [batch][post_nms_top_n], out_count [batch]; zeros / -1 behind the count. */
int sfvos_rpn_nms(const float* boxes, const float* logits, const float* scores, const int* valid, const int* counts,
                  int n_levels, int batch, int pre_nms_top_n, float nms_thresh, int post_nms_top_n, void* workspace,
                  float* out_boxes, float* out_scores, int* out_index, int* out_count, sfvos_stream_t stream);

/* ---- training targets of roi_heads (model.py:346 with targets; torchvision's select_training_samples and
 * project_masks_on_boxes, parity unpinned by the reference).  One image per call; the candidate list of an image is its n_p
 * proposals followed by its G ground-truth boxes (add_gt_proposals), N = n_p + G, read through the two pointers.  Limits,
 * refused by message: N <= 8192, G <= 1024, batch_size_per_image <= 4096, M <= 64.  Bit-identical from run to run. ---- */

/* box_iou + Matcher(high, low, allow_low_quality_matches = False) + the labels of assign_targets_to_proposals, for each
 * candidate i: with the largest IoU over the ground truth (the lower index on a tie; a NaN IoU never wins),
 *   IoU >= high: matched[i] = that index, labels[i] = gt_labels[matched[i]];
 *   IoU <  low : matched[i] = 0, labels[i] = 0 (background);  otherwise matched[i] = 0, labels[i] = -1 (ignored);
 * max_iou[i] (may be NULL) = that IoU.  IoU = inter / (area_a + area_b - inter) in fp32, every operation rounded on its
 * own, as sfvos_detections and sfvos_rpn_nms compute it.  G = 0: every label, match and max_iou is 0.
 * proposals [n_p][4], gt_boxes [G][4], gt_labels [G] int64; matched [N] int32, labels [N] int64, max_iou [N]. */
int sfvos_roi_match(const float* proposals, int n_p, const float* gt_boxes, const int64_t* gt_labels, int G, float high,
                    float low, int* matched, int64_t* labels, float* max_iou, sfvos_stream_t stream);

/* Bytes of `workspace` of sfvos_roi_sample for n = N candidates; 0 for a refused n. */
size_t sfvos_roi_sample_workspace_bytes(int n);

/* BalancedPositiveNegativeSampler + the gathers of select_training_samples.  With #pos candidates of label >= 1 and #neg of
 * label 0: n_pos = min(#pos, int(batch_size_per_image * positive_fraction)), n_neg = min(#neg, batch_size_per_image -
 * n_pos); the n_pos positives with the smallest (keys[i], i) pairs are chosen (lexicographic; -0 == +0; a NaN key ranks
 * behind every number), the negatives likewise; label -1 is never chosen.  With independent uniform keys that is a
 * uniformly random subset without replacement, torchvision's randperm draw in distribution (not its random stream).
 * The chosen candidates, in ascending index (torchvision's where(pos | neg)): counts[0] = S = n_pos + n_neg rows are
 * valid in every per-row output, counts[1] = P = n_pos.  All per-row outputs hold batch_size_per_image rows:
 *   index int32 (-1 behind row S), out_boxes [.][4], out_labels int64, out_matched int32,
 *   regression_targets [.][4] = sfvos_box_encode's arithmetic with weights (wx, wy, ww, wh) of the box gt_boxes[matched]
 *   (a box of zeros when G = 0, as torchvision substitutes) against the chosen box,
 *   pos_slot int32 = the rows whose label is >= 1, ascending, P of them.
 * Rows behind S (P for pos_slot) are left untouched, index excepted.  labels / matched: sfvos_roi_match's; keys [N]. */
int sfvos_roi_sample(const int64_t* labels, const int* matched, const float* keys, const float* proposals, int n_p,
                     const float* gt_boxes, int G, int batch_size_per_image, double positive_fraction, float wx, float wy,
                     float ww, float wh, void* workspace, int* counts, int* index, float* out_boxes, int64_t* out_labels,
                     int* out_matched, float* regression_targets, int* pos_slot, sfvos_stream_t stream);

/* project_masks_on_boxes: targets[P][M][M] = roi_align(masks[:, None], [matched, boxes], (M, M), spatial_scale 1,
 * sampling_ratio -1, aligned False)[:, 0] -- the ADAPTIVE grid sfvos_roi_align does not have: per box roi_w = max(x2 - x1,
 * 1), bin_w = roi_w / M, grid_w = ceil(bin_w) (the same for the height); sample x = (x1 + pw bin_w) + ((ix + .5) bin_w) /
 * grid_w in fp32, every operation rounded on its own; a sample with y < -1, y > H, x < -1 or x > W adds 0, the others are
 * clamped at 0 and interpolated as torchvision's bilinear_interpolate does (the last row / column branch included); the
 * sum is divided by max(grid_h grid_w, 1).  The grid is device data: any size is looped over, none refused.
 * masks: G planes [H][W] of uint8 (masks_are_u8 != 0, what a dataset delivers) or fp32; boxes [P][4]; matched [P] int32
 * (a value outside [0, G) gives zeros).  P = 0 is a no-op. */
int sfvos_mask_targets(const void* masks, int masks_are_u8, int G, int H, int W, const float* boxes, const int* matched,
                       int P, int M, float* targets, sfvos_stream_t stream);

/* ---- training call of the region proposal network (model.py:236-240 and :329-335 with targets; loss_objectness and
 * loss_rpn_box_reg enter total_loss at :361-368).  The RPN is frozen and the call runs under no_grad: no backward.  Restated
 * from torchvision's assign_targets_to_anchors, Matcher(high, low, allow_low_quality_matches = True),
 * BalancedPositiveNegativeSampler, BoxCoder(1, 1, 1, 1).encode and compute_loss (parity unpinned by the reference).
 * Anchor n of an image is n = A (sum_{l' < l} H_l' W_l' + h W_l + w) + a -- torchvision's per-image concatenation (level,
 * h, w, a) -- and its box is base_anchors[l][a] + (w stride_w, h stride_h, w stride_w, h stride_h) with the strides of
 * sfvos_rpn_decode; no anchor array is ever in memory.  Objectness and deltas stay in the pyramid's level-major storage
 * (segment (l, b) contiguous).  Matching and sampling take one image per call, the loss all images at once; nothing
 * synchronises with the host.  Integer atomics only (a maximum, histograms, a slot counter whose order is re-ranked):
 * bit-identical from run to run.  Limits, refused by message before any launch: A <= 8, SFVOS_MAX_LEVELS levels, G <= 1024,
 * batch_size_per_image <= 4096, N < 2^24 anchors per image, thresholds and fraction in [0, 1], beta >= 0. ---- */

/* Bytes of `workspace` of sfvos_rpn_match and sfvos_rpn_sample (one buffer serves both, one after the other); 0 for a
 * refused size. */
size_t sfvos_rpn_targets_workspace_bytes(const sfvos_pyramid* pyr, int num_anchors, int G, int batch_size_per_image);

/* For every anchor n the largest IoU over the ground truth (fp32, every operation rounded on its own, the arithmetic of
 * sfvos_roi_match; the lower ground-truth index on a tie; a NaN IoU never wins):
 *   IoU >= high: labels[n] = 1, matched[n] = that index;  IoU < low: labels[n] = 0;  otherwise labels[n] = -1;
 *   matched[n] = 0 wherever the label is not 1 (Matcher's -1 / -2 clamped at 0);  max_iou[n] (may be NULL) = that IoU.
 * allow_low_quality != 0 is Matcher.set_low_quality_matches_, literally: with highest[g] = max_n IoU(g, n), every anchor n
 * with IoU(g, n) == highest[g] for some g gets labels[n] = 1 and matched[n] = its OWN argmax (not g).  A ground-truth box
 * that no anchor overlaps has highest = 0 and so marks every anchor whose IoU with it is 0.  The comparison is exact: a
 * second launch recomputes the IoUs with the same code.  G = 0: every label, match and max_iou is 0.
 * base_anchors: device floats [n_levels][A][4]; gt_boxes [G][4]; matched, labels int32 [N]; max_iou [N]. */
int sfvos_rpn_match(const sfvos_pyramid* pyr, int num_anchors, const float* base_anchors, int tensor_h, int tensor_w,
                    const float* gt_boxes, int G, float high, float low, int allow_low_quality, void* workspace,
                    int* matched, int* labels, float* max_iou, sfvos_stream_t stream);

/* BalancedPositiveNegativeSampler under sfvos_roi_sample's contract: with #pos anchors of label >= 1 and #neg of label 0,
 * n_pos = min(#pos, int(batch_size_per_image * positive_fraction)), n_neg = min(#neg, batch_size_per_image - n_pos); of
 * each class the anchors with the smallest (keys[i], i) pairs are chosen (-0 == +0; a NaN key ranks behind every number);
 * label -1 is never chosen.  The selection is a radix select of the 56-bit word (key, index) over several workgroups, one
 * launch per digit.  counts[0] = S = n_pos + n_neg, counts[1] = P = n_pos;
 *   index int32 [batch_size_per_image]: the P positives in ascending anchor index, then the S - P negatives in ascending
 *   anchor index (torchvision's cat([pos, neg])), -1 behind S;
 *   regression_targets [batch_size_per_image][4]: for the first P rows sfvos_box_encode's arithmetic with weights (1, 1, 1,
 *   1) of gt_boxes[matched] against the anchor; the other rows are left untouched.
 * N must be the pyramid's anchors per image.  labels, matched: sfvos_rpn_match's; keys [N]. */
int sfvos_rpn_sample(const int* labels, const int* matched, const float* keys, int N, const sfvos_pyramid* pyr,
                     int num_anchors, const float* base_anchors, int tensor_h, int tensor_w, const float* gt_boxes, int G,
                     int batch_size_per_image, double positive_fraction, void* workspace, int* counts, int* index,
                     float* regression_targets, sfvos_stream_t stream);

/* compute_loss over all images: index [batch][batch_size_per_image], counts [batch][2], regression_targets
 * [batch][batch_size_per_image][4] are sfvos_rpn_sample's outputs of each image, read on the device.  With S_tot = sum S:
 *   out[0] = sum over the sampled rows of (max(x, 0) - x z + log1p(exp(-|x|))) / S_tot, x = the anchor's logit, z = row < P
 *   out[1] = sum over the positive rows and 4 coordinates of smooth_l1(delta - target; beta) / S_tot; beta = 0 is plain L1
 * (torchvision releases differ between L1 and beta = 1/9).  Sums in double, fixed order, one workgroup; S_tot = 0 gives
 * 0 / 0 as torch does.  per_sample [batch][batch_size_per_image][2] (may be NULL) receives the two terms of each sampled
 * row (0 for the box term of a negative); rows behind S are left untouched.  An index outside [0, N) gives NaN. */
int sfvos_rpn_loss(const float* objectness, const float* deltas, const sfvos_pyramid* pyr, int batch, int num_anchors,
                   const int* index, const int* counts, const float* regression_targets, int batch_size_per_image,
                   float beta, float* per_sample, float* out, sfvos_stream_t stream);

/* ---- feature pyramid network (model.py:204, `maskrcnn_model.backbone(...)`: the FPN half of torchvision's
 * BackboneWithFPN, frozen in the reference at :176-177, so inference only; restated from torchvision's
 * FeaturePyramidNetwork + LastLevelMaxPool, parity unpinned by the reference).  The four 3x3 output convs are
 * sfvos_conv3d (kt = 1, taps = 9, a one-level pyramid per call); the two calls below are the rest.  Bit-identical from run
 * to run (no atomics). ---- */

/* inner_blocks[i](x) + F.interpolate(top, size = (h, w), mode = 'nearest') in one pass:
 *   y[(b h + i) w + j][n] = bias[n] + sum_c x[b][c][i][j] weight[n][c] + top[(b top_h + (i >> 1)) top_w + (j >> 1)][n]
 * x: planar fp32 [batch][c_in][h][w] through ELEMENT strides (stride_w must be 1), read once, never copied to a
 * channels-last form; c_in a multiple of 32.  weight: [c_out][c_in] in the compute dtype (the natural layout cast; no
 * packer), 16-byte aligned; c_out a multiple of 32, <= 256.  bias: fp32 [c_out].  top: NULL, or the coarser level's inner
 * map, [batch top_h top_w] positions x ld_top in the compute dtype; h must be 2 top_h or 2 top_h - 1 and w likewise (what a
 * stride-2 body gives; exactly there `nearest` reads index >> 1).  y: channels-last, pitch ld_y >= c_out, compute dtype.
 * dtype: SFVOS_F32 (exact-f32 MFMA) or SFVOS_BF16 (x and weight rounded to bf16, fp32 accumulation). */
int sfvos_fpn_lateral(const float* x, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w, int batch,
                      int c_in, int h, int w, const void* weight, const float* bias, int c_out, const void* top,
                      int top_h, int top_w, int ld_top, void* y, int ld_y, int dtype, sfvos_stream_t stream);

/* LastLevelMaxPool = max_pool2d(kernel 1, stride 2), a subsample: dst[b][i][j][0 .. C) = src[b][2 i][2 j][0 .. C) for
 * i < (h - 1) / 2 + 1, j < (w - 1) / 2 + 1.  src: [batch h w] positions x ld_src, dst: [batch oh ow] positions x ld_dst,
 * both 16-byte aligned with pitches of whole 16-byte chunks; C any whole number of 16-byte chunks; f32 or bf16. */
int sfvos_fpn_pool(const void* src, int ld_src, void* dst, int ld_dst, int batch, int h, int w, int C, int dtype,
                   sfvos_stream_t stream);

/* ---- ResNet-50 body (model.py:204, `maskrcnn_model.backbone(...)`: the `body` half of torchvision's BackboneWithFPN,
 * frozen in the reference at :176-177, so inference only; restated from torchvision's resnet50 + FrozenBatchNorm2d, parity
 * unpinned by the reference).  Activations are channels-last: [batch][h][w] positions x pitch, in the compute dtype
 * (SFVOS_F32: exact-f32 MFMA, SFVOS_BF16: bf16 operands, fp32 accumulation).  Bit-identical from run to run (no atomics).
 * ---- */

/* Every conv of the bottlenecks, with the frozen norm's affine, the residual and the ReLU in its epilogue:
 *   y[b][i][j][n] = act(scale[n] * sum_{dh,dw,c} x[b][s i + dh - p][s j + dw - p][c] W[n][c][dh][dw] + shift[n]
 *                       + residual[b][i][j][n])
 * taps = 1 (1x1, p = 0) or 9 (3x3, p = 1); stride s = 1 or 2; output sides (h - 1) / s + 1, (w - 1) / s + 1; pixels outside
 * the image are zero.  c_in, c_out: multiples of 64 up to 2048.  weight: [c_out][taps][c_in] in the compute dtype (the
 * state-dict weight permuted to (n, dh, dw, c) and cast; no packer).  scale, shift: fp32 [c_out], both required.
 * residual: NULL or [batch oh ow] positions x ld_res in the compute dtype.  acc * scale + shift in fp32, then the residual,
 * then ReLU (relu = 1), one rounding on the store.  Pitches are whole 16-byte chunks; every pointer 16-byte aligned.
 * workspace: sfvos_conv2d_workspace_bytes of the same shape (0 for most; the K splits of layer4's shapes need their fp32
 * slabs, summed in split order by a second launch); NULL is accepted where that is 0. */
int sfvos_conv2d(const void* x, int ld_x, const void* weight, const float* scale, const float* shift, const void* residual,
                 int ld_res, void* y, int ld_y, int batch, int h, int w, int c_in, int c_out, int taps, int stride, int relu,
                 int dtype, void* workspace, sfvos_stream_t stream);
size_t sfvos_conv2d_workspace_bytes(int dtype, int batch, int h, int w, int c_in, int c_out, int taps, int stride);
/* The configuration sfvos_conv2d picks for a shape on a device of `cus` compute units (0 = the current device's): 0 = 128
 * channels x 128 positions per workgroup, 1 = 64 x 128, 2 = 64 x 64, 5 = 64 x 64 with K split over *splits slabs (1
 * otherwise; splits may be NULL).  A pure function of its arguments; a refused shape returns SFVOS_E_ARG. */
int sfvos_conv2d_plan(int dtype, int batch, int h, int w, int c_in, int c_out, int taps, int stride, int cus, int* splits);

/* conv1 (7x7, stride 2, pad 3, 3 -> 64, no bias) + affine + ReLU: x planar fp32 [batch][3][h][w] through ELEMENT strides
 * (stride_w must be 1), rounded to the compute dtype in registers; y channels-last [batch oh ow] x ld_y, 64 channels.
 * weight: [64][176] in the compute dtype, k = (c * 7 + dh) * 8 + dw with zeros at dw = 7 and behind k = 168 (the
 * state-dict weight padded and cast; no packer). */
int sfvos_body_stem(const float* x, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w, int batch, int h,
                    int w, const void* weight, const float* scale, const float* shift, void* y, int ld_y, int dtype,
                    sfvos_stream_t stream);

/* max_pool2d(kernel 3, stride 2, padding 1) channels-last: dst[b][i][j][c] = max over the window's pixels inside the image
 * (the padding is -inf, not 0).  Layouts, pitches and alignment as sfvos_fpn_pool. */
int sfvos_maxpool3x3s2(const void* src, int ld_src, void* dst, int ld_dst, int batch, int h, int w, int C, int dtype,
                       sfvos_stream_t stream);

/* ---- image transform (model.py:283, :298: `maskrcnn_model.transform(images, targets)`, torchvision's
 * GeneralizedRCNNTransform; restated from its published sources and torch's upsample kernels, parity unpinned by the
 * reference).  The size rule (min_size / max_size -> oh x ow, size_divisible -> Hp x Wp) lives on the host. ---- */

/* normalize + resize (bilinear, align_corners = False, scale recomputed from the sizes) + batch_images' zero pad in one
 * launch: `batch` images of h x w pixels and 3 channels -> dst[b][c][0 .. Hp)[0 .. Wp), planar fp32, which sfvos_body_stem
 * reads.  The image occupies [0, oh) x [0, ow); every other element up to Hp x Wp is written as +0.0f (dst may be
 * uninitialised); nothing outside [0, Hp) x [0, Wp) of a plane is touched.
 * src: SFVOS_F32 (stride_w must be 1) or SFVOS_U8 through ELEMENT strides, so a decoded [batch][h][w][3] byte frame is
 *   read in place (stride_c = 1, stride_w = 3); a byte u enters as float(u) / 255.0f (IEEE division: ToTensor), after
 *   which both dtypes take the same arithmetic.  dst: 16-byte aligned, strides in elements, non-negative multiples of 4
 *   (16-byte rows), stride 1 along w, dst_stride_h >= Wp.  mean, std: by value; every std > 0.
 * Arithmetic of output pixel (i, j) of channel c, all in fp32, every operation rounded to nearest on its own (no fused
 * multiply-add), in this order -- the contract:
 *     scale = (float)in / (float)out                       (per axis: h / oh, w / ow)
 *     src   = max(scale * ((float)d + 0.5f) - 0.5f, 0)     (d = i resp. j)
 *     i0 = (int)src,  i1 = min(i0 + 1, in - 1),  l1 = src - (float)i0,  l0 = 1.0f - l1
 *     v(y, x) = (x[b][c][y][x] - mean[c]) / std[c]         (IEEE division) for the four taps
 *     left  = ly0 * v(y0, x0) + ly1 * v(y1, x0),  right = ly0 * v(y0, x1) + ly1 * v(y1, x1)     (vertically first)
 *     out   = lx0 * left + lx1 * right
 * Offsets are 64-bit (a sequence's batch exceeds 4 GB); a source plane and a padded plane hold fewer than 2^31
 * elements.  Bit-identical from run to run and between the two source dtypes on equal values. */
int sfvos_transform_image(const void* src, int src_dtype, int64_t stride_b, int64_t stride_c, int64_t stride_h,
                          int64_t stride_w, int batch, int h, int w, float mean0, float mean1, float mean2, float std0,
                          float std1, float std2, float* dst, int64_t dst_stride_b, int64_t dst_stride_c,
                          int64_t dst_stride_h, int oh, int ow, int Hp, int Wp, sfvos_stream_t stream);

/* The nearest resize of the target masks, F.interpolate(mask[:, None].float(), size = (oh, ow))[:, 0].byte():
 *     dst[g][i][j] = src[g][min((int)floorf((float)i * scale_h), h - 1)][min((int)floorf((float)j * scale_w), w - 1)],
 *     scale = (float)in / (float)out in fp32.
 * src: dense bytes [G][h][w]; dst: dense bytes [G][oh][ow], as sfvos_mask_targets takes them.  G = 0 returns 0 without a
 * launch (the pointers may be NULL then). */
int sfvos_transform_masks(const unsigned char* src, int G, int h, int w, unsigned char* dst, int oh, int ow,
                          sfvos_stream_t stream);

/* ---- evaluation-side reducer (reference code/helpers/davis_evaluate.py:40-42) ------------ */

/* out[i] = OR over the n predicted masks of (masks[k][i] >= threshold), i < hw: the per-frame union the reference
 * builds with numpy before writing the PNG.  masks: n contiguous fp32 planes of hw elements ([N,1,H,W]);
 * out: hw bytes (0/1).  n may be 0 (all zeros).  Comparison and OR only: bit-exact with the reference. */
int sfvos_mask_union(const float* masks, int n, int64_t hw, float threshold, unsigned char* out,
                     sfvos_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFVOS_H */

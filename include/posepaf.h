/*
 * posepaf.h -- C ABI of libposepaf.so: the MI355X (gfx950) post-processing path of the bottom-up pose
 * pipeline (flip-average -> heat-map NMS/peak refinement -> limb-map line-integral scoring -> greedy
 * limb matching -> person assembly), hand-written HIP behind plain pointers and sizes.
 *
 * Two groups of entry points:
 *
 *  (1) DROP-IN for the reference's native module `utils/pafprocess` -- the seven functions of
 *      /root/reference/utils/pafprocess/pafprocess.h:70-76, same names, argument order and meaning,
 *      exported with C linkage.  The SWIG interface (utils/pafprocess/pafprocess.i:14) or a ctypes stub
 *      binds them unchanged; see INTEGRATION.md.  Host arrays in, results held until the next call.
 *
 *  (2) NATIVE batched path -- takes the network output where it already lives (HBM) and returns
 *      fixed-size per-image records; this is what removes the reference's D2H copy
 *      (utils/parse_skeletons.py:80), the per-peak cv2.resize loop (:143-163) and the 31.5 MB limb-map
 *      upsample (evaluate.py:77-80).
 *
 * All functions return 0 (PP_OK) or a negative pp_status unless stated otherwise.  No function falls back
 * to a CPU implementation: without a usable HIP device every compute entry point returns PP_ERR_NO_DEVICE.
 */
#ifndef POSEPAF_H
#define POSEPAF_H

#include <stdint.h>

/* exported symbols (the library is built with -fvisibility=hidden) */
#define PP_API __attribute__((visibility("default")))

#ifdef __cplusplus
extern "C" {
#endif

#define PP_NUM_PART 18    /* pafprocess.h:11  NUM_PART */
#define PP_NUM_LIMB 30    /* pafprocess.h:20  COCOPAIRS_SIZE */
#define PP_NUM_HEAT 20    /* utils/parse_skeletons.py:17 */
#define PP_NUM_CH 50      /* config/config.py:127-129: [0,30) limb maps, [30,48) keypoints, [48,50) background */
#define PP_MAX_HUMANS 128 /* capacity of one pp_record */
#define PP_MAX_PEAKS_PER_PART_LIMIT 128

typedef enum {
    PP_OK = 0,
    PP_ERR_NO_DEVICE = -1,   /* no HIP device / runtime error at create */
    PP_ERR_BAD_ARG = -2,
    PP_ERR_TOO_LARGE = -3,   /* batch/h/w beyond what the context was created for; a map above 650x950; on the Python-rule
                                path (pp_process_batch_py) also a map that does not fit LDS */
    PP_ERR_HIP = -4,         /* a HIP call failed; pp_last_hip_error() has the code */
    PP_ERR_OVERFLOW = -5,    /* compat path only: a per-part / per-image capacity was exceeded */
    PP_ERR_UNSUPPORTED = -6  /* pp_conv_f16: this tile configuration / channel count is not available for the shape */
} pp_status;

typedef enum { PP_F32 = 0, PP_F16 = 1 } pp_dtype;

/* per-image status bits in pp_record.status */
#define PP_ST_PEAK_OVERFLOW 1u   /* a keypoint channel had more peaks than max_peaks_per_part: per part the first
                                    max_peaks_per_part peaks in row-major order of the map are kept, and peak ids are numbered
                                    over the KEPT peaks (parts in order, no gaps) -- the record is what the reference gives on
                                    that truncated joint list; n_peaks counts the kept peaks; pp_read_peaks refuses */
#define PP_ST_HUMAN_OVERFLOW 2u  /* more than PP_MAX_HUMANS people after pruning: the first PP_MAX_HUMANS in the reference's
                                    order are kept.  Never raised by the Python rules, whose table (next bit) is as large */
#define PP_ST_SKEL_OVERFLOW 4u   /* more live partial skeletons than the assembly table holds: 256 with the C++ rules,
                                    128 with the Python rules (pp_process_batch_py and the original path) */
#define PP_ST_SORT_UNDEFINED 8u  /* the reference's std::sort (non-strict comparator, pafprocess.cpp:333-335)
                                    would have read outside its array on this input: its result is undefined */
#define PP_ST_CAND_OVERFLOW 16u  /* more accepted limb candidates for one limb than the kernel holds */
#define PP_ST_FLOAT_COORDS 32u   /* original path: pp_human.x / .y hold float32 BIT PATTERNS (fractional coordinates) */
#define PP_ST_SYNC_TIMEOUT 64u   /* the image's assembly gave up waiting for a limb of its own launch (cannot happen on a healthy
                                    device: the record is incomplete and the context must be re-created) */
#define PP_ST_RECON_UNDEFINED 128u /* Python rules with remove_recon = 1: for a connection of this image the reference itself raises
                                    (utils/parse_skeletons.py:529-537: int(np.where(...)[0]) on zero or several matches, or
                                    the assert conn1_idx != conn2_idx); that connection changed nothing */

/* One person.  Mirrors what evaluate.py:111-127 pulls through the getters:
 * peak_id[p] = get_part_peak_id(h,p) (-1 = part absent); x/y/part_score = get_part_x/y/score(peak_id);
 * score = get_score(h) = total_score / part_count (pafprocess.cpp:295-297). */
typedef struct {
    int32_t peak_id[PP_NUM_PART];
    int32_t x[PP_NUM_PART];
    int32_t y[PP_NUM_PART];
    float part_score[PP_NUM_PART];
    float score;
    int32_t n_parts;
} pp_human;

typedef struct {
    int32_t n_humans;
    int32_t n_peaks;
    uint32_t status;
    int32_t n_connections;
    pp_human humans[PP_MAX_HUMANS];
} pp_record;

typedef struct pp_ctx pp_ctx;

/* ---------------------------------------------------------------- context */

/* Allocates all device workspace up front (no allocation or synchronisation happens in the per-batch
 * calls, so they can be captured into a hipGraph).  max_h/max_w are FEATURE-map sizes (image/4).
 * max_peaks_per_part in [1, 128]; 64 covers every synthetic scene up to 45 people. */
PP_API int pp_create(pp_ctx **out, int device, int max_batch, int max_h, int max_w, int max_peaks_per_part);
PP_API int pp_destroy(pp_ctx *ctx);
PP_API int pp_last_hip_error(const pp_ctx *ctx);
PP_API const char *pp_status_string(int status);
/* 1 if a HIP device is visible to this process, 0 otherwise (does not create a context) */
PP_API int pp_device_available(void);

/* ---------------------------------------------------------------- native batched path
 * net_out_dev: DEVICE pointer, (batch, n_samples, 50, h, w) planar, n_samples = 2 when flip (sample 1 is the
 * network's output for the W-mirrored image, utils/parse_skeletons.py:69-72) else 1; dtype PP_F16 or PP_F32.
 * With PP_F16 the flip-average is done in binary16 and then widened, exactly like numpy on the float16
 * array of utils/parse_skeletons.py:91-93,103.
 * min_img_size: the `img_h` argument of process_paf (evaluate.py:110), one value for the whole batch;
 * min_img_size_dev (optional DEVICE int[batch]) overrides it per image.
 * records_dev: DEVICE pp_record[batch].  stream: hipStream_t (NULL = default stream).  Asynchronous. */
PP_API int pp_process_batch(pp_ctx *ctx, int batch, const void *net_out_dev, int dtype, int h, int w, int flip,
                     int min_img_size, const int *min_img_size_dev, pp_record *records_dev, void *stream);

/* Where the kernels of pp_process_batch / pp_nms_batch / pp_nms_batch_ex / pp_time_kernels keep a feature map while they
 * work on it.  A channel that fits LDS (up to roughly 270x270 binary16, 190x190 float32) is staged there by each workgroup:
 * two launches.  A larger one -- up to 650x950, the reference's own cap (utils/parse_skeletons.py:46-49) -- stays in device
 * memory: a pre-pass writes the 48 flip-averaged channels into a workspace of the context and the same two kernels read it
 * through a global pointer (three launches, same results bit for bit, still nothing allocated or synchronised per call).
 * pp_create allocates that workspace (max_batch * 48 * plane * 4 bytes) only when a float32 max_h x max_w map would not fit LDS.
 * pp_set_map_residency(PP_MAPS_HBM) sends EVERY shape down the large-map path (A/B measurements, tests at small shapes) and
 * allocates the workspace if pp_create did not; PP_MAPS_AUTO restores the default.  A setter: never call it under stream capture.
 * pp_map_residency: PP_MAPS_LDS or PP_MAPS_HBM for the shape as pp_process_batch would run it, or PP_ERR_TOO_LARGE.
 * pp_map_workspace_bytes: size of the workspace (0: none allocated).
 * pp_process_batch_py (the Python rules) has no large-map kernels yet and keeps answering PP_ERR_TOO_LARGE beyond LDS. */
typedef enum { PP_MAPS_AUTO = 0, PP_MAPS_LDS = 1, PP_MAPS_HBM = 2 } pp_map_residency_mode;
PP_API int pp_set_map_residency(pp_ctx *ctx, int mode);
PP_API int pp_map_residency(const pp_ctx *ctx, int dtype, int h, int w);
PP_API long long pp_map_workspace_bytes(const pp_ctx *ctx);

/* The same batched path with the rules of the reference's PURE-PYTHON matching, find_connections + find_humans
 * (utils/parse_skeletons.py:324-600) -- what evaluate.py runs with --run_refactor but WITHOUT --run_cpp.  It differs
 * from the C++ rules in sampling (np.round(np.linspace)), float64 arithmetic, a stable sort, the merge conditions and the
 * score bookkeeping.  img_height is find_connections' `img_height` argument.  Thresholds are the
 * INI defaults (utils/config:17-25).  Needs max_peaks_per_part <= 64.
 * The map must fit LDS (PP_ERR_TOO_LARGE otherwise): the large-map kernels exist for the C++ rules only. */
PP_API int pp_process_batch_py(pp_ctx *ctx, int batch, const void *net_out_dev, int dtype, int h, int w, int flip,
                               int img_height, const int *img_height_dev, pp_record *records_dev, void *stream);

/* Config-2 path: flip-average + NMS + refinement of the 18 keypoint channels only
 * (utils/parse_skeletons.py:126-176).  peaks_dev: DEVICE float[batch][18][max_peaks_per_part][4] =
 * (x, y, score, unused); counts_dev: DEVICE int[batch][18] (true counts, may exceed the capacity).
 * refine = 0 reproduces bool_refine_center=False.  Either output may be NULL to use the context's own
 * workspace (read back with pp_read_peaks). */
PP_API int pp_nms_batch(pp_ctx *ctx, int batch, const void *net_out_dev, int dtype, int h, int w, int flip, int refine,
                 float *peaks_dev, int *counts_dev, void *stream);

/* Same kernel with the original (non-refactored) path's rules selectable:
 *   nms_mode    0: plus-shaped window, value >  threshold   (find_peaks_refactor, utils/parse_skeletons.py:115-116)
 *               1: full 3x3 window,    value >= threshold   (util.keypoint_heatmap_nms, utils/util.py:177-185)
 *   refine_mode 0: (p + 0.5) * 4 - 0.5, raw score            (heatmap_nms with bool_refine_center=False)
 *               1: x4 bicubic patch arg-max                   (heatmap_nms, :143-163)
 *               2: 5x5 weighted centroid, score = box mean    (util.refine_centroid, utils/util.py:188-213)
 *               3: integer map coordinates, raw score */
PP_API int pp_nms_batch_ex(pp_ctx *ctx, int batch, const void *net_out_dev, int dtype, int h, int w, int flip, int nms_mode,
                           float threshold, int refine_mode, float *peaks_dev, int *counts_dev, void *stream);

/* Measurement aid: runs the kernels of pp_process_batch `iters` times EACH on `stream`, bracketed by HIP
 * events on that stream, and returns the average duration of one launch in milliseconds:
 * ms_out[0] = k_heat_peaks (peaks + the image ordering), ms_out[1] = k_limb_connect (limb scoring, matching AND the
 * person assembly done by each image's last limb workgroup), ms_out[2] = k_assemble_wave (the assembly alone as its own
 * one-wave-per-image launch; diagnostic, not part of the chain), ms_out[3] = the whole chain as pp_process_batch enqueues it.
 * ms_out must hold 4 floats.  Blocking.  For a map kept in device memory (pp_map_residency) [0] and [1] are the _hbm instances
 * and [3] includes the pre-pass; pp_time_map_prepass times that pre-pass (k_flip_average_maps) alone the same way, *ms_out = 0
 * when the shape has none. */
PP_API int pp_time_kernels(pp_ctx *ctx, int batch, const void *net_out_dev, int dtype, int h, int w, int flip,
                           int min_img_size, int iters, float *ms_out, void *stream);
PP_API int pp_time_map_prepass(pp_ctx *ctx, int batch, const void *net_out_dev, int dtype, int h, int w, int flip, int iters,
                               float *ms_out, void *stream);

/* Forward-pass helpers (not part of the reference's interface), all on channels-last (NHWC) fp16 DEVICE tensors with
 * channels % 8 == 0 and 16-byte aligned pointers:
 *   pp_bias_act_f16 : in place  y = act(y + bias[c] (+ residual)) (+ post),  act = LeakyReLU(slope) if has_act;
 *                     n_elems = N*H*W*C; bias fp16[channels]; residual / post may be NULL
 *   pp_maxpool2_f16 : y[n][ho][wo][c] = max of the 2x2 window of x (x is (n, 2*h_out, 2*w_out, c)): the maximum of the window's
 *                     non-NaN elements (IEEE 754-2019 maximumNumber), so NaN only when all four are NaN, and +0 for a window that
 *                     holds +0 and -0 and nothing larger.  The pooled output of pp_pw_pool_f16 / pp_pw_cat_f16 follows the same rule
 *                     bit for bit: the tuner may take either kernel for one layer.  (torch's max_pool2d propagates NaN instead.)
 *   pp_upsample2_f16: nearest x2: y (n, 2*h_in, 2*w_in, c) from x (n, h_in, w_in, c) */
PP_API int pp_bias_act_f16(void *y, const void *bias, const void *residual, const void *post, long n_elems, int channels,
                           float slope, int has_act, void *stream);
PP_API int pp_maxpool2_f16(const void *x, void *y, long n, int h_out, int w_out, int channels, void *stream);
PP_API int pp_upsample2_f16(const void *x, void *y, long n, int h_in, int w_in, int channels, void *stream);
/* y = a + b (+ c) on fp16 tensors of n_elems elements (multiple of 8, 16-byte aligned), fp32 sum rounded once; c may be NULL. */
PP_API int pp_add3_f16(const void *a, const void *b, const void *c, void *y, long n_elems, void *stream);
/* SE squeeze (models/layers_transposed.py SELayer, AdaptiveAvgPool2d(1)): out[n][c] = mean over the h*w pixels of the NHWC fp16
 * activation x (n, hw, channels), fp32 accumulation.  partial_ws: DEVICE float[n][splits][channels] scratch; splits = number of
 * workgroups per image (pick n*splits >= ~1024).  channels % 8 == 0, channels <= 2048. */
PP_API int pp_channel_mean_f16(const void *x, void *partial_ws, void *out, int n, long hw, int channels, int splits, void *stream);
/* The SE squeeze without a pass of its own (round 3): the 3x3 / pad 1 halo-tile kernel writes y = act(conv + bias) AND, per image,
 * per-split partial sums of its binary16 outputs: sums_ws DEVICE float[n][splits][c_out], splits = pp_conv_own_sums_splits(h, w)
 * (0: the shape is not taken by that kernel); pp_channel_mean_finish_f16 adds the partials in split order and writes the fp16 mean
 * (= pp_channel_mean_f16's second kernel). */
PP_API int pp_conv_own_sums_splits(int h, int w);
PP_API int pp_conv_own_sums_f16(const void *x, const void *w, const void *bias, void *y, void *sums_ws, int n, int h, int wd, int c_in,
                                int c_out, float slope, void *stream);
/* The same with a residual: y = act(conv + bias + residual), residual DEVICE (n, h, w, c_out), and the partial sums of the binary16
 * values it stores, laid out and consumed as pp_conv_own_sums_f16's -- the last block of a level of the published variant's
 * hourglass (models/layers_transposed_final.py: `up1 += deconv2`, then the LeakyReLU), whose output the stage's SE block squeezes.
 * Also takes maps lower than a tile (16 x 16: whole images stacked in one tile; n must be a multiple of the images per tile).
 * splits = pp_conv_own_res_sums_splits(h, w) (0: the shape is not taken). */
PP_API int pp_conv_own_res_sums_splits(int h, int w);
PP_API int pp_conv_own_res_sums_f16(const void *x, const void *w, const void *bias, const void *residual, void *y, void *sums_ws, int n,
                                    int h, int wd, int c_in, int c_out, float slope, void *stream);
PP_API int pp_channel_mean_finish_f16(const void *partial_ws, void *out, int n, long hw, int channels, int splits, void *stream);
/* The SE block's excitation (models/layers_transposed.py:289-310) in one launch: gains (n, c) fp16 = sigmoid(W2 leaky(W1 mean + b1)
 * + b2), one workgroup per sample, roundings as the fp16 torch modules it replaces.  Input: partial_ws (n, splits, c) fp32 channel
 * sums over hw pixels (pp_conv_own_sums_f16 / the first pass of pp_channel_mean_f16) OR mean (n, c) fp16 -- the other NULL.
 * w1 (hidden, c), b1 (hidden), w2 (c, hidden), b2 (c): fp16 DEVICE. */
PP_API int pp_se_gains_f16(const void *partial_ws, const void *mean, const void *w1, const void *b1, const void *w2, const void *b2,
                           void *out, int n, long hw, int c, int hidden, int splits, float slope, void *stream);
/* The layout change between the forward and the post-processing: x DEVICE (n, hw, 64) fp16 -- the last head's pixel-major output,
 * 50 channels + zero padding -- to channel planes y DEVICE (n, c_out, hw), c_out <= 64: the (N, 50, h, w) tensor the reference's
 * network returns (models/posenet.py:193-202) and pp_process_batch reads.  One pass at streaming speed instead of a strided copy. */
PP_API int pp_nhwc64_to_planes_f16(const void *x, void *y, int n, long hw, int c_out, void *stream);
/* SE excitation: y[n][p][c] = x[n][p][c] * scale[n][c] on NHWC fp16 (x: (n, hw, channels), scale: fp16 (n, channels)); y may be x. */
PP_API int pp_channel_scale_f16(const void *x, const void *scale, void *y, int n, long hw, int channels, void *stream);

/* Fused point-wise (1x1) convolution on the matrix cores (v_mfma_f32_32x32x16_f16), fp16 in/out, fp32 accumulate:
 *   y[m][n] = act(sum_k x[m][k] * w[n][k] + bias[n] (+ residual[m][n])) (+ post[m][n])
 * x: DEVICE [M][K] (channels-last activation, M = batch*H*W), w: DEVICE [N][K] (a (Cout, Cin, 1, 1) conv weight),
 * bias fp16[N], residual / post optional [M][N], y [M][N]; all 16-byte aligned.  pp_pwconv_supported(K, N) tells whether
 * the shape is taken (K in {64,128,192,256}, N % 32 == 0, weights fit LDS); other shapes stay on PyTorch-ROCm. */
PP_API int pp_pwconv_supported(int K, int N);
PP_API int pp_pwconv_f16(const void *x, const void *w, const void *bias, const void *residual, const void *post, void *y,
                         long M, int K, int N, float slope, int has_act, void *stream);

/* A1 forward: one fused convolution on the matrix cores, stride 1, square kernel, fp16 in/out, fp32 accumulate:
 *   y = leaky(conv(x, w) + bias[k] (+ extra if extra_mode == 1)) (+ extra if extra_mode == 2)
 * i.e. Conv2d + folded BatchNorm + LeakyReLU of models/layers_transposed.py:Conv, with the residual add of
 * Residual.forward (extra_mode 1) or the hourglass's `up1 +` (extra_mode 2) applied to the fp32 accumulators.
 * x: DEVICE (n, h, w, c_in) NHWC; w: DEVICE (c_out, ksize, ksize, c_in) (= a channels-last (c_out, c_in, k, k) weight);
 * bias fp16[c_out]; extra: DEVICE (n, ho, wo, c_out) or NULL (extra_mode 0); y: DEVICE (n, ho, wo, c_out) with
 * ho = h + 2*pad - dilation*(ksize-1).  slope = LeakyReLU slope (1.0f = no activation).  c_in, c_out multiples of 8,
 * all pointers 16-byte aligned.  config in [0, pp_conv_num_configs()) picks the workgroup tile (M x N x K-step per block):
 * 0 128x256x32, 1 256x128x32, 2 128x128x32, 3 128x64x32 (128 threads), 4 128x64x32, 5 64x128x32, and the software-pipelined
 * variants 6 128x128x64 (v4), 7 128x128x64 (v3), 8 256x256x32 (v3), 9 256x256x64 (v3);
 * callers time the configurations once per layer shape and keep the fastest (posepaf/fused_model.py).
 * The GEMM main loop is ROCm composable_kernel's XDL implicit-GEMM template; the epilogue functor is this library's. */
PP_API int pp_conv_num_configs(void);
PP_API int pp_conv_f16(const void *x, const void *w, const void *bias, const void *extra, void *y, int n, int h, int wd,
                       int c_in, int c_out, int ksize, int pad, int dilation, int extra_mode, float slope, int config,
                       void *stream);

/* pp_conv_f16 with explicit pixel strides (elements, multiples of 8): x and / or y may be a channel slice of a wider NHWC tensor
 * (ldx >= c_in, ldy >= c_out) -- the two halves of the backbone's concatenation (models/layers_transposed.py:193-195) are
 * written in place by their producers and read in place by the dilated chain. */
PP_API int pp_conv_ld_f16(const void *x, const void *w, const void *bias, const void *extra, void *y, int n, int h, int wd,
                          int c_in, int c_out, int ksize, int pad, int dilation, int extra_mode, float slope, int config, int ldx,
                          int ldy, void *stream);

/* A1 forward: the same fused convolution as pp_conv_f16 -- identical arguments and semantics -- as a HAND-WRITTEN implicit-GEMM
 * kernel (csrc/posepaf_conv_own.hip: 256-pixel x bn-channel workgroup tiles, LDS-DMA staging, v_mfma_f32_16x16x32_f16, epilogue
 * from registers; no composable_kernel).  Needs c_in % 32 == 0 and c_out % 64 == 0 (pp_conv_own_supported).  bn = output
 * channels per workgroup: 256, 128 or 64 (must divide c_out), 0 = the largest that divides c_out; 512 = the 3x3 halo-tile
 * kernel; 576 = its instances for c_out = 64 mod 128 (3x3, pad = dilation = 1, packed pixels, extra_mode 0 / 1 / 2), which run the
 * half-empty last channel tile on all four SIMDs -- bit-equal to 512, PP_ERR_UNSUPPORTED for every other shape or form. */
PP_API int pp_conv_own_supported(int c_in, int c_out, int ksize);
/* Diagnostics (the diagnostics build only, `make -C csrc diag`: the product library compiles no ablated instance and ignores
 * POSEPAF_CONV_DBG): after a launch of the 3x3 halo kernel with POSEPAF_CONV_DBG bit 1024 set, the median over the first nwg
 * workgroups of the shader-clock cycles spent per section (summed over the workgroup's tiles): out6[0..4] = wait for the
 * first DMA and the previous stores / first fragment reads / main loop / next tile's decode + DMA issue / epilogue;
 * out6[5] = the main loop in 100 MHz ticks.  No reference counterpart. */
PP_API int pp_conv_debug_clock(double *out6, int nwg);
PP_API int pp_conv_own_f16(const void *x, const void *w, const void *bias, const void *extra, void *y, int n, int h, int wd,
                           int c_in, int c_out, int ksize, int pad, int dilation, int extra_mode, float slope, int bn,
                           void *stream);
/* The same on channel SLICES of wider NHWC tensors (ldx / ldy = elements between consecutive pixels of x / y, multiples of 8; `extra`
 * stays packed) -- the backbone's concatenation written and read in place (models/layers_transposed.py:193-195).  The 3x3
 * halo-tile kernel only (bn = 512): pad = dilation = 1, or the backbone's dilated convolutions pad = dilation = 3 / 4 / 5
 * (models/layers_transposed.py:125-157, :175-182), whose rows the kernel walks class by class (y mod dilation). */
PP_API int pp_conv_own_ld_f16(const void *x, const void *w, const void *bias, const void *extra, void *y, int n, int h, int wd,
                              int c_in, int c_out, int ksize, int pad, int dilation, int extra_mode, float slope, int bn, int ldx,
                              int ldy, void *stream);
/* The same with extensions.  For the 3x3 / pad 1 halo-tile kernel (bn = 512 only, PP_ERR_UNSUPPORTED otherwise):
 *  - upsampled_input = 1: x is (n, h/2, wd/2, c_in) and stands for its x2 nearest-neighbour upsample (h, wd even) -- the
 *    `self.upsample(down3)` of models/layers_transposed.py:272 (nn.Upsample, :212) without materialising the upsample;
 *  - extra_mode = 3: y = fp16(act(conv + bias)) + extra + extra2 (fp32 sum, rounded once) -- the hourglass' `up1 + up2`
 *    and the stage's feature-cache add (models/posenet.py:104-106) inside the convolution's epilogue.
 * For every kernel (bn = 0 / 256 / 128 / 64 / 512):
 *  - extra_mode = 4: y = act(conv + bias + extra) as in mode 1 and a SECOND OUTPUT y2 = y + extra2 (the sum of the two
 *    binary16 tensors, rounded once) -- `cache = merge_preds(...) + merge_features(...)` and `x = x + cache`
 *    (models/posenet.py:116-118) in one pass.  y2 is NULL in every other mode. */
PP_API int pp_conv_own_ex_f16(const void *x, const void *w, const void *bias, const void *extra, const void *extra2, void *y, void *y2,
                              int n, int h, int wd, int c_in, int c_out, int ksize, int pad, int dilation, int extra_mode, float slope,
                              int bn, int upsampled_input, void *stream);

/* A1, the hourglass' `hg[i][3](upsample(low))` (models/layers_transposed.py:270-275): a 3x3 / pad 1 convolution behind a x2
 * nearest upsample, evaluated as FOUR 2x2 convolutions of the half-resolution tensor (one per output phase): an output pixel
 * (2y + py, 2x + px) only sees a 2x2 neighbourhood of the input, each input pixel through the sum of the 3x3 taps landing on it --
 * 16 instead of 36 multiply-adds per input pixel, the same real-number result.  w4: DEVICE [4][c_out][2][2][c_in] fp16, phase
 * (py, px) = (0,0), (0,1), (1,0), (1,1); rows: py = 0 -> {w[0], w[1] + w[2]} on input rows {y - 1, y}; py = 1 -> {w[0] + w[1], w[2]}
 * on {y, y + 1}; columns alike (sums formed in fp32, rounded once).  x: (n, h_low, w_low, c_in); y / extra / extra2: (n, 2 h_low,
 * 2 w_low, c_out); extra_mode 0 / 2 / 3 as pp_conv_own_ex_f16; bn: output channels per workgroup (0, 256, 128, 64). */
PP_API int pp_conv_up2_collapsed_f16(const void *x, const void *w4, const void *bias, const void *extra, const void *extra2, void *y, int n,
                                     int h_low, int w_low, int c_in, int c_out, int extra_mode, float slope, int bn, void *stream);

/* A1, the 1x1 convolutions as an HBM-bound stream with the neighbouring element-wise passes folded in (csrc/posepaf_conv_own.hip
 * k_pw):   y = act(conv1x1(x * scale[n]) + bias (+ extra))   [and  y2 = y + extra2]
 * x: DEVICE (m, c_in) fp16 = an NHWC activation of m = n * h * w pixels; scale: DEVICE (m / hw, c_in) fp16 or NULL -- the SE
 * block's per-sample channel gains (models/layers_transposed.py:289-310), multiplied into the input in binary16 exactly as the
 * separate x * s pass would; w: DEVICE (c_out, c_in); bias fp16[c_out]; extra / extra2 / y2: DEVICE (m, c_out) or NULL;
 * y: DEVICE with ldy >= c_out elements between pixels (a channel slice of a wider tensor when larger); hw = h * w.
 * extra_mode 0 / 1 / 2 / 4 as pp_conv_own_ex_f16; 5 = the second output y2 = y + extra2 without a tensor added before the
 * activation (extra = NULL).  pp_pw_supported: c_in in {64, 128, 192, 256, 384, 448, 512, 640, 704, 768} (the sums of a two-input call included), c_out % 64 == 0;
 * with `scale`, hw % 64 == 0 (a group of pixels must not straddle two images). */
PP_API int pp_pw_supported(int c_in, int c_out);
PP_API int pp_pw_f16(const void *x, const void *scale, const void *w, const void *bias, const void *extra, const void *extra2, void *y,
                     void *y2, long m, int hw, int c_in, int c_out, int ldy, int extra_mode, float slope, void *stream);
/* An INPUT form of the same stream: y = act(conv1x1(x * scale[n] + pre_add) + bias) -- the compress convolution of the published
 * variant (models/posenet_final.py: before_regress[s][0] reads SE(h)_s + cache_s).  scale: DEVICE (m / hw, c_in) fp16; pre_add:
 * DEVICE (m, c_in) fp16 or NULL.  The product is rounded to binary16, then the sum is rounded to binary16, where the fp16 modules
 * round them; neither tensor is written to memory.  c_in in {256, 384, 512, 640, 768}, c_out % 64 == 0, hw % 64 == 0. */
PP_API int pp_pw_pre_f16(const void *x, const void *scale, const void *pre_add, const void *w, const void *bias, void *y, long m, int hw,
                         int c_in, int c_out, int ldy, float slope, void *stream);
/* The same with the 2x2 / stride-2 max-pool of the tensor it produces (y; y2 in mode 4) as one more output -- the hourglass pools
 * exactly these tensors (`low = hg[i][1](pool(x))`, models/layers_transposed.py:262-266), so its pooling passes disappear.
 * pool_out: DEVICE (n, h / 2, w / 2, c_out); width = w: a multiple of 32 (64 when c_in = 64); h even.  The pooled value is
 * pp_maxpool2_f16's, bit for bit: the maximum of the window's non-NaN elements, NaN only when all four are NaN, +0 above -0
 * (tests/test_gpu_helper_kernels.py runs both on one tensor).  y may be NULL: the
 * full-resolution tensor is then not written (a caller that reads only the pooled one); y = NULL without pool_out is
 * PP_ERR_BAD_ARG. */
PP_API int pp_pw_pool_f16(const void *x, const void *scale, const void *w, const void *bias, const void *extra, const void *extra2,
                          void *y, void *y2, void *pool_out, long m, int hw, int width, int c_in, int c_out, int ldy, int extra_mode,
                          float slope, void *stream);

/* pp_pw_f16 on TWO inputs whose channels continue each other along K: y = act(W [x ; x2] + bias (+ extra)), W: (c_out, c_in + c_in2).
 * A residual block's last 1x1 convolution and its 1x1 skip convolution (models/layers_transposed.py:12-48: conv3(t) + skip(x)) are one
 * product this way; the skip's output is never written.  pool_out (NULL: none) / width as pp_pw_pool_f16; with pool_out, y may be
 * NULL as there. */
PP_API int pp_pw_cat_f16(const void *x, const void *x2, const void *w, const void *bias, const void *extra, void *y, void *pool_out, long m,
                         int hw, int width, int c_in, int c_in2, int c_out, int ldy, int extra_mode, float slope, void *stream);

/* A1, the stem (models/layers_transposed.py:78-87 Backbone.conv1 + bn1 + LeakyReLU): y = leaky(conv(x, w, 7x7, stride 2, padding 3)
 * + bias) in one HBM-bound pass.  x: DEVICE (n, h, w, 3) NHWC fp16, h even, w % 4 == 0; w_prepared: DEVICE (64, 192) fp16,
 * w_prepared[k][(r * 8 + s1) * 3 + c] = weight[k][c][r][s1 - 1] (zeros for s1 = 0 and past 168); bias fp16[64];
 * y: DEVICE (n, h / 2, w / 2, 64) NHWC fp16. */
PP_API int pp_stem7x7_f16(const void *x, const void *w_prepared, const void *bias, void *y, int n, int h, int w, float slope,
                          void *stream);

/* A0 pre-processing (utils/parse_skeletons.py:52-73, utils/util.py:44-65) of a batch of equally sized BGR uint8 DEVICE
 * images (batch, h, w, 3): pad bottom/right to a multiple of pad_to with pad_value, divide by 255, and write each image
 * followed (flip != 0) by the W-mirror of the PADDED image.  out: DEVICE (batch*(flip?2:1), Hp, Wp, 3), PP_F16 or PP_F32. */
PP_API int pp_preprocess_u8(const void *images_u8, void *out, int dtype, int batch, int h, int w, int pad_to,
                            int pad_value, int flip, void *stream);
/* The same with the test-time rotation (utils/parse_skeletons.py:214-221): the padded image is warped with cv2.warpAffine(M,
 * (0, 0)) -- m_inv: HOST, 6 doubles, M inverted as warpAffine does it (posepaf/rotation.py) -- 0 outside the padded frame,
 * and the mirror written is that of the WARPED image. */
PP_API int pp_preprocess_u8_affine(const void *images_u8, void *out, int dtype, int batch, int h, int w, int pad_to,
                                   int pad_value, int flip, const double *m_inv, void *stream);
/* The same for a bucket of images of DIFFERENT sizes sharing one padded shape (hp, wp) -- the reference pads every image
 * alone (utils/parse_skeletons.py:54); the batched evaluation loop groups images by padded shape.  images_u8: DEVICE
 * (batch, hp, wp, 3), image b in the top-left (sizes[b], sizes[batch + b]) corner of its slot, the rest of the slot is never
 * read; sizes_dev: DEVICE int[2][batch] = heights, then widths (heights double as pp_process_batch's min_img_size_dev). */
PP_API int pp_preprocess_u8_ragged(const void *images_u8, const int *sizes_dev, void *out, int dtype, int batch, int hp,
                                   int wp, int pad_value, int flip, void *stream);

/* Demo rendering (reference demo_image.py:174-192, the refactored branch; utils/common.py:240-264 draw_humans with pixel
 * coordinates): every human of every record drawn on its image in ONE launch -- per human the present joints 0..17 as discs of
 * radius 4.5 in CocoColors[part] (utils/common.py:281-283), then CocoPairsRender (:285-289) as lines of thickness 3 in
 * CocoColors[pair], later over earlier -- bit-equal to the NumPy renderer utils/draw.py:draw_humans(canvas, humans) (parity with
 * cv2's own rasteriser stays unpinned, as for draw.py).  The ellipse / alpha-blend style of the original branch
 * (demo_image.py:218-240) is pp_draw_limbs_u8 below.
 * records_dev: DEVICE pp_record[batch]; n_humans is clamped to [0, PP_MAX_HUMANS], peak_id[p] < 0 = part absent, and with
 * PP_ST_FLOAT_COORDS the joint is drawn at the truncated coordinate, as int(bp.x) does.  src_u8 / dst_u8: DEVICE (batch, hp, wp, 3)
 * BGR; dst_u8 == src_u8 draws in place, any other overlap is the caller's error.  sizes_dev: DEVICE int[2][batch] = heights, then
 * widths (the layout of pp_preprocess_u8_ragged), NULL = every image is hp x wp.  Only the top-left (h, w) corner of a slot is
 * read or written: the rest of dst is left as it was, the rest of src is never read.  Bit-equality holds for coordinates within
 * +-32767; beyond that nothing outside the image's pixels is written.  Asynchronous, nothing allocated: capturable. */
PP_API int pp_draw_humans_u8(const pp_record *records_dev, const void *src_u8, void *dst_u8, const int *sizes_dev, int batch, int hp,
                             int wp, void *stream);

/* The demo's other style (reference demo_image.py:218-240, the original branch; what `python demo_image.py` draws without
 * flags): per limb type of DRAW_LIST (config/config.py:154) and per human a filled rotated ellipse between the two joints in
 * LimbColors[board[t]] and black rings on the joints, each such drawing blended 0.4 / 0.6 into the canvas so far -- bit-equal to
 * the NumPy renderer utils/draw.py:draw_limbs_original on the persons / candidates the record stands for
 * (posepaf/render.py:record_to_persons).  Per pixel: the fold, in draw order (limb types outside, humans inside), of
 * px = clip(rint(px * 0.4 + cur * 0.6), 0, 255) over the instances that hit it, cur = the ellipse colour where the ellipse hits
 * and black where only a ring does; the geometry is spelled out in csrc/posepaf_limbs.hip.  The ellipse's angle
 * k = int(degrees(atan2(dy, dx))) is found without a device libm (pp_limb_angle_deg), and cos / sin of k degrees come from
 * angle_table_dev: a DEVICE copy of the 361 x 2 doubles pp_limb_angle_table fills on the HOST with the C library.
 * Records, buffers, sizes_dev, the in-place form and the claim (coordinates within +-32767; a joint with a non-finite float32
 * coordinate skips its limbs) are pp_draw_humans_u8's.  Asynchronous, nothing allocated: capturable. */
PP_API int pp_draw_limbs_u8(const pp_record *records_dev, const void *src_u8, void *dst_u8, const int *sizes_dev, int batch, int hp,
                            int wp, const double *angle_table_dev, void *stream);
/* table_host[2 * (k + 180)] = cos, [2 * (k + 180) + 1] = sin of k * (pi / 180) for k = -180 .. 180, from the C library's cos / sin
 * at run time: the bits of Python's math.cos(math.radians(k)) / math.sin(math.radians(k)).  Host work only. */
PP_API int pp_limb_angle_table(double *table_host);
/* int(math.degrees(math.atan2(dy, dx))) for finite dy, dx that are differences of int or float32 coordinates: the host instance
 * of the function the kernel calls (no libm inside; exact directions by branches, a bisection on the table's signs elsewhere). */
PP_API int pp_limb_angle_deg(double dy, double dx);

/* COCO keypoint evaluation, the per-image half (reference evaluate.py:182-209 append_result and :274-279 COCOeval, here
 * posepaf/oks_eval.py evaluate_keypoints_ranges stage A), on the records where they already are.  Both entries are asynchronous,
 * allocate nothing, use no atomics and store every output word plainly on every launch: capturable.
 *
 * pp_coco_rows_f32: per record the humans with at least one peak_id >= 0, in record order, one row of PP_COCO_ROW = 52 floats
 *   each: 17 x (x, y, 1) in COCO keypoint order (posepaf/skeleton.py ORDER_COCO), zeros for absent parts, then pp_human.score --
 *   what coco.humans_from_record + coco.coco_results produce.  n_humans is clamped to [0, PP_MAX_HUMANS]; a PP_ST_FLOAT_COORDS
 *   record's coordinates are rounded half to even first (np.rint).  Coordinates are exact up to +-2^24 (float32).
 *   records_dev: DEVICE pp_record[batch]; rows_dev: DEVICE float[batch][PP_MAX_HUMANS][52], rows past the count are zero;
 *   counts_dev: DEVICE int[batch]. */
#define PP_COCO_ROW 52
#define PP_AP_MAX_DETS 20    /* COCOeval maxDets for keypoints */
#define PP_AP_MAX_GT 128     /* ground truths of one image the matching kernel holds (20 x 128 float64 OKS values in LDS) */
#define PP_AP_THRESHOLDS 10  /* OKS 0.50:0.05:0.95 */
#define PP_AP_RANGES 3       /* area ranges all, medium, large */
/* One ground-truth annotation as the evaluation reads it: keypoints (x, y, v) in COCO order, the annotation's area, its box
 * [x, y, w, h] (has_bbox = 0: the annotation has none, a ground truth without labelled keypoints then has OKS 0), the crowd
 * flag and num_keypoints (0 = ignored). */
typedef struct {
    double keypoints[17][3];
    double area;
    double bbox[4];
    int32_t iscrowd;
    int32_t num_keypoints;
    int32_t has_bbox;
    int32_t reserved;
} pp_gt_ann;
PP_API int pp_coco_rows_f32(const pp_record *records_dev, int batch, float *rows_dev, int *counts_dev, void *stream);
/* pp_oks_match: one wave per image.  rows_dev / counts_dev: pp_coco_rows_f32's outputs (counts clamped to [0, PP_MAX_HUMANS]).
 *   gt_dev: DEVICE pp_gt_ann[], the annotations of ground-truth slot s at [gt_offsets[s], gt_offsets[s + 1]); gt_offsets_dev /
 *   gt_offsets_host: int[n_slots + 1], the SAME values on the device (read by the kernel) and on the host (argument checks);
 *   slots_dev / slots_host: int[batch], the slot of image b, both NULL = image b uses slot b.  thresholds: HOST double[10],
 *   area_ranges: HOST double[3][2] (lo, hi; both ends belong to the range) -- the caller's own values, passed to the kernel by
 *   value and never recomputed.  Per image:
 *     order_dev  int[batch][20]          rows of the 20 best detections by score, ties in row order; -1 past n_det
 *     scores_dev float[batch][20]        their scores; 0 past n_det
 *     match_dev  int8[batch][3][10][20]  1 true positive, 0 false positive, -1 ignored (matched an ignored ground truth, or
 *                                        unmatched with the detection's own area outside the range); 0 past n_det
 *     n_det_dev  int[batch]              min(count, 20)
 *     n_gt_dev   int[batch][3]           ground truths that count in each range (not crowd, num_keypoints != 0, area in range)
 *     oks_dev    double[batch][20][128]  optional (NULL: not written): the OKS matrix, detections in score order, ground truths
 *                                        in annotation order, 0 outside [n_det][count]
 *   The OKS follows compute_oks one IEEE float64 operation at a time; exp is the device library's and the sum runs in keypoint
 *   order.  An image with more than PP_AP_MAX_GT ground truths: PP_ERR_TOO_LARGE before any launch, never truncated. */
PP_API int pp_oks_match(const float *rows_dev, const int *counts_dev, int batch, const pp_gt_ann *gt_dev, const int *gt_offsets_dev,
                        const int *gt_offsets_host, int n_slots, const int *slots_dev, const int *slots_host, const double *thresholds,
                        const double *area_ranges, int *order_dev, float *scores_dev, signed char *match_dev, int *n_det_dev,
                        int *n_gt_dev, double *oks_dev, void *stream);

/* Ground-truth-style scenes in the network-output layout, rendered on the device from joint lists (the reference's training-target
 * recipe, py_cocodata_server/py_data_heatmapper.py:105-257; csrc/posepaf_synth.hip spells out the arithmetic): what synthetic
 * evaluations inject into the network output.  Needs no context.
 *   joints_dev   DEVICE float[batch][max_people][18][3]: x, y in image pixels (stride 4: map cell i sits at 4 i + 1.5) and a flag,
 *                flag < 2 = annotated; n_people_dev: DEVICE int[batch], clamped to [0, max_people]; people past it are never read
 *   scene_id_dev DEVICE long long[batch], the noise identity of each image (NULL: the image's index); unused without noise
 *   out_dev      DEVICE (batch, n_samples, 50, h, w) planar, dtype PP_F16 or PP_F32; every word is stored on every launch.
 *                n_samples = 2 adds the mirrored sample, out1[c][y][x] = out0[flip_ord[c]][y][w - 1 - x] (config/config.py:150-152)
 *   flags        PP_SCENE_REVERSE_KP: channel 49 = max over the keypoint channels 30..47 (:86); other bits are reserved and ignored.
 *                Channel 48 (the segmentation mask of the reference) is always zero
 *   noise_sigma  > 0: sigma * N(0, 1) added after the clip to [0, 1], no second clip.  Counter-based (Philox4x32-10 keyed by seed,
 *                counter = scene id, sample, channel, pixel; Box-Muller in float32): an image gets the same noise in whichever
 *                batch, slot or launch geometry it is rendered
 * Deterministic (gather, no atomics; people are accumulated in index order).  PP_ERR_BAD_ARG: a null joints / n_people / out
 * pointer, n_samples outside {1, 2}, a dtype that is neither PP_F16 nor PP_F32, a non-positive batch / max_people / h / w, a
 * negative or NaN noise_sigma.  PP_ERR_UNSUPPORTED: max_people above PP_SCENE_MAX_PEOPLE (the joints and windows of one image are
 * staged in LDS and its people are compacted by one wave).  PP_ERR_TOO_LARGE: batch above 65535, a map side above 10^6, or 2^24 or
 * more 64 x 32 tiles in one map.
 * PP_ERR_NO_DEVICE without a HIP device.  Asynchronous, nothing allocated: capturable. */
#define PP_SCENE_REVERSE_KP 1
#define PP_SCENE_MAX_PEOPLE 64
PP_API int pp_render_scenes(const float *joints_dev, const int *n_people_dev, const long long *scene_id_dev, int batch,
                            int max_people, int h, int w, int n_samples, int dtype, int flags, float noise_sigma,
                            unsigned long long seed, void *out_dev, void *stream);

/* The reference's multi-scale focal-L2 validation loss (models/loss_model.py:23-81, :133-161) as per-image terms
 *   terms[t][s][b] = sum over c, y, x of (p - G)^2 * |1 - st| * M * cw[c]
 * for stack t, scale s, image b (csrc/posepaf_loss.hip spells out the arithmetic): G = the target pooled to the prediction's size by
 * adaptive_avg_pool2d's window formula (float64 sum, one rounding to float32; a window that holds nothing but 0.01f pools to exactly
 * 0.01f), st = p where G >= 0.01f (float32 comparison) else 1 - p, M = the mask resampled bilinearly (align_corners = False) in
 * float64 with values < 0.5 set to 0, cw = multi_task_weight for channel 48, keypoint_task_weight for channels 30..47, 1 otherwise;
 * everything behind G and M in float64.  PP_LOSS_PLAIN_L2 drops |1 - st| (l2_loss, :103-131).  Needs no context.
 *   pred_dev     HOST array of n_stacks * n_scales DEVICE pointers, [t * n_scales + s] -> the prediction of (batch, 50, hs[s], ws[s]);
 *                read during the call only (the table travels by value in the kernel arguments)
 *   pred_dtype   PP_F16 or PP_F32, of every prediction
 *   pred_pixel_stride   0: planes (batch, 50, h_s, w_s); >= 50: pixel-major (batch, h_s, w_s, stride), channels 0..49 of a pixel read,
 *                the rest never (64 = what the fused heads write, 50 = a channels-last tensor)
 *   target_dev   DEVICE planes (50, H, W) per image, PP_F16 or PP_F32, target_image_stride elements (>= 50 H W) from one image to the
 *                next: sample 0 of a (batch, 2, 50, H, W) buffer is read in place with 2 * 50 * H * W
 *   mask_dev     DEVICE float (batch, H, W), or NULL = all ones
 *   hs, ws       HOST int[n_scales], 1 <= hs[s] <= H, 1 <= ws[s] <= W (any sizes: the windows need not divide)
 *   workspace_dev  DEVICE, pp_focal_l2_workspace_bytes(batch, n_stacks, n_scales, hs, ws) bytes, 8-byte aligned
 *   terms_dev    DEVICE double[n_stacks][n_scales][batch]
 * Every word of terms_dev and every workspace word that is read is stored plainly on every launch (no memset, no atomics).
 * Deterministic: the order of an image's additions depends on the shapes alone -- its terms are bit-identical in every batch, slot
 * and run.  Predictions are read with 16-byte loads where their runs are 16-byte aligned and element by element elsewhere (same
 * order).  PP_ERR_BAD_ARG: a null pointer (but mask_dev), a pointer not aligned to its element (workspace / terms: 8 bytes), a dtype
 * that is neither PP_F16 nor PP_F32, batch / n_stacks / n_scales / H / W < 1, an hs / ws entry outside 1..H / 1..W,
 * pred_pixel_stride in 1..49 or negative, target_image_stride below 50 H W.  PP_ERR_UNSUPPORTED: n_stacks above 8, n_scales above 5.
 * PP_ERR_TOO_LARGE: batch above 65535, more than 2^30 pixels in a map, a pixel stride above 2^20, 2^31 or more workgroups (128-pixel
 * tiles of all scales x batch).  PP_ERR_NO_DEVICE without a HIP
 * device (after the argument checks).  Asynchronous, nothing allocated: capturable.
 * pp_focal_l2_workspace_bytes: the bytes, or the negative status of the same shape checks. */
#define PP_LOSS_PLAIN_L2 1
PP_API long long pp_focal_l2_workspace_bytes(int batch, int n_stacks, int n_scales, const int *hs, const int *ws);
PP_API int pp_focal_l2_terms(const void *const *pred_dev, int pred_dtype, int pred_pixel_stride, const void *target_dev, int target_dtype,
                             long long target_image_stride, const float *mask_dev, int batch, int H, int W, int n_stacks, int n_scales,
                             const int *hs, const int *ws, double multi_task_weight, double keypoint_task_weight, int flags,
                             void *workspace_dev, double *terms_dev, void *stream);

/* The derivative of pp_focal_l2_terms with respect to the predictions: for upstream weights tw[t][s][b] = dL / dterms[t][s][b]
 *   d = p - (double)G
 *   focal:  f = |1 - st|,  f' = -sgn(1 - p) where G >= 0.01f, sgn(p) elsewhere, sgn(0) = +0.0 (torch's abs backward)
 *           e = (2.0 d) f + (d d) f'
 *   plain (PP_LOSS_PLAIN_L2):  e = 2.0 d
 *   grad = tw[t][s][b] (cw[c] (M e))       float64 in exactly this association, no contraction
 * rounded to float32 (nearest even) and, for PP_F16 predictions, that float32 rounded to binary16.  G, M, cw and every argument up to
 * `flags` are pp_focal_l2_terms's.  There is no gradient with respect to the target or the mask (the foreground test and the mask
 * threshold are steps).
 *   term_weight_dev  DEVICE double[n_stacks][n_scales][batch], 8-byte aligned; a zero weight gives a zero gradient (a padded batch)
 *   grad_dev     HOST array of n_stacks * n_scales DEVICE pointers, [t * n_scales + s] -> a buffer with the geometry and dtype of
 *                pred_dev[t * n_scales + s] (planes, or pixel-major with the same stride); must not be the prediction itself
 * Every element of channels 0..49 is stored plainly on every launch (no memset, no atomics, no workspace); the padding channels
 * 50 .. stride - 1 of a pixel-major buffer and everything behind channel 49 of the last pixel are never written.  Stores are 16 bytes
 * wide where pp_focal_l2_terms's loads are and the gradient pointers of the scale are 16-byte aligned too, element by element
 * elsewhere.  Elementwise: an image's gradients do not depend on batch size, slot, alignment or launch geometry.
 * Refuses what pp_focal_l2_terms refuses, with the same codes, and with PP_ERR_BAD_ARG a null term_weight_dev / grad_dev / entry of
 * it, a gradient pointer not aligned to its element, term_weight_dev off an 8-byte boundary, and a gradient pointer equal to its
 * prediction's.  Nothing is launched on a refusal.  Asynchronous, nothing allocated, needs no context: capturable. */
PP_API int pp_focal_l2_grad(const void *const *pred_dev, int pred_dtype, int pred_pixel_stride, const void *target_dev, int target_dtype,
                            long long target_image_stride, const float *mask_dev, int batch, int H, int W, int n_stacks, int n_scales,
                            const int *hs, const int *ws, double multi_task_weight, double keypoint_task_weight, int flags,
                            const double *term_weight_dev, void *const *grad_dev, void *stream);

/* The reference's training-data transformer (py_cocodata_server/py_data_transformer.py:42-88, :111-183, py_data_iterator.py:54-74,
 * py_data_heatmapper.py:79-86) as one device stage: the uint8 image and both uint8 masks of every image of a batch warped with the
 * image's own affine matrix (cv2.warpAffine INTER_LINEAR, BORDER_CONSTANT, 8-bit fixed-point path), the masks reduced to stride 4
 * (INTER_AREA), the all-person mask eroded 3 x 3 into the foreground plane, and the joints mapped through the same matrix with the
 * left / right exchange after a flip.  The arithmetic is the contract of INTEGRATION section 17 (csrc/posepaf_augment.hip restates
 * it; tests/augment_reference.py is its NumPy form): it follows OpenCV 3.4, but OpenCV was not run against it.  Needs no context.
 *   images_u8      DEVICE uint8 (batch, slot_h, slot_w, 3), image b in the top-left (h_b, w_b) corner of its slot; the rest of a
 *                  slot is never read
 *   sizes_dev      DEVICE int[2][batch], heights then widths (the layout of pp_preprocess_u8_ragged), clamped to the slot; NULL =
 *                  every image fills its slot
 *   mask_miss_u8, mask_all_u8   DEVICE uint8 (batch, slot_h, slot_w), either may be NULL: constant 255 / constant 0
 *   m_inv_dev      DEVICE double[batch][6], the matrix as cv2.warpAffine inverts it (posepaf/rotation.py invert_affine): destination
 *                  (x, y) reads source (m0 x + m1 y + m2, m3 x + m4 y + m5).  The fixed-point coordinates are int32: the caller keeps
 *                  (|m0| out_w + |m1| out_h + |m2| + 1) 1024 and the same of the second row below 2^31 (posepaf/augment.py refuses
 *                  what is beyond); beyond it pixels are wrong, but no address leaves the slot
 *   m_fwd_dev      DEVICE double[batch][6], the forward matrix, for the joints;  flip_dev: DEVICE int[batch]
 *   joints_in_dev  DEVICE double[batch][max_people][18][3];  n_people_dev: DEVICE int[batch], clamped to [0, max_people]
 *   out_h, out_w   the output size, both multiples of 4;  border: HOST unsigned char[3], the image's border value
 *   image_out      DEVICE (batch, out_h, out_w, 3), PP_F32 or PP_F16, 16-byte aligned: float(u8) / 255.0f correctly rounded (and that
 *                  rounded to binary16)
 *   mask_miss_out  DEVICE float (batch, out_h / 4, out_w / 4): the mask pp_focal_l2_terms takes
 *   fg_out         DEVICE, PP_F16 or PP_F32: plane b (out_h / 4 x out_w / 4) at element b * fg_image_stride -- with the pointer at
 *                  channel 48 of a (batch, n, 50, h, w) target and the stride n * 50 * h * w the plane lands in place
 *   joints_out     DEVICE float[batch][max_people][18][3], the layout pp_render_scenes reads; persons at or beyond n_people[b] are
 *                  written as they were (rounded to float32)
 * Every output word is stored plainly on every launch; an image's outputs do not depend on the batch, the slot or the launch
 * geometry.  PP_ERR_BAD_ARG: a null pointer (but sizes_dev and the two masks), a non-positive batch / slot / max_people / output
 * size, out_h or out_w no multiple of 4, a dtype that is neither PP_F16 nor PP_F32, fg_image_stride below one plane, image_out off
 * a 16-byte boundary or another pointer off its element's.  PP_ERR_UNSUPPORTED: max_people above PP_SCENE_MAX_PEOPLE.
 * PP_ERR_TOO_LARGE: batch above 65535, a slot or output side above 32768.  PP_ERR_NO_DEVICE without a HIP device (after the argument
 * checks).  Nothing is launched on a refusal.  Asynchronous, nothing allocated, every per-image parameter read on the device:
 * capturable, and a captured graph replays with new draws. */
PP_API int pp_augment_batch(const void *images_u8, const int *sizes_dev, const void *mask_miss_u8, const void *mask_all_u8, int batch,
                            int slot_h, int slot_w, const double *m_inv_dev, const double *m_fwd_dev, const int *flip_dev,
                            const double *joints_in_dev, const int *n_people_dev, int max_people, int out_h, int out_w,
                            const unsigned char *border, void *image_out, int image_dtype, float *mask_miss_out, void *fg_out,
                            int fg_dtype, long long fg_image_stride, float *joints_out, void *stream);

/* The person masks of the reference's data/coco_masks_hdf5.py (make_mask over annToMask) from polygon vertices and at most one
 * uncompressed crowd run-length code per image: mask_miss (0 where a person is segmented without keypoints, or the crowd lies) and
 * mask_all (255 on every person), uint8, into the slots pp_augment_batch reads.  The arithmetic is the contract of INTEGRATION
 * section 19 (csrc/posepaf_segm.hip restates it; tests/coco_mask_reference.py is its NumPy form): it follows the published maskApi.c,
 * but pycocotools was not run against it.  Needs no context.
 *   verts_dev      DEVICE double[n_verts][2], every ring's (x, y) back to back
 *   rings_dev      DEVICE int[n_rings][4], 16-byte aligned: first vertex, vertices (>= 3), order index of the ring's annotation among
 *                  its image's, flags (bit 0: the annotation has num_keypoints <= 0 and counts for mask_miss).  An image's rings
 *                  are consecutive.  A ring pointing outside verts_dev is skipped
 *   images_dev     DEVICE long long[batch][5]: first ring, rings, first entry of the crowd in runs_dev, its runs (0: no crowd), the
 *                  crowd's order index -- rings with a smaller order index are taken out of the crowd (make_mask is order-dependent)
 *   runs_dev       DEVICE long long[n_runs]: per crowd the running sums c_0, c_0 + c_1, ... of its counts (the last is h_b w_b); pixel
 *                  p = x h_b + y is set iff it lies in an odd-indexed run
 *   sizes_dev      DEVICE int[2][batch], heights then widths (the layout of pp_augment_batch), clamped to the slot; NULL = every
 *                  image fills its slot
 *   workspace      DEVICE, 8-byte aligned, at least pp_coco_masks_workspace_bytes(n_verts) bytes: the vertices in rleFrPoly's
 *                  integer grid.  The boundary events are found per edge and column in closed form and never stored, so the
 *                  size does not depend on how many there are
 *   mask_miss_u8, mask_all_u8   DEVICE uint8 (batch, slot_h, slot_w), distinct: image b in the top-left (h_b, w_b) corner of its slot;
 *                  the rest of a slot is never written.  An image with no ring and no crowd gets 255 / 0
 * n_verts, n_rings and n_runs are the lengths of the arrays: everything read from the tables is clamped against them, so they may be
 * capacities above what a batch uses, and a captured graph replays with rewritten tables.  An image's masks do not depend on the
 * batch, the slot or the launch geometry; no atomics on mask bytes.  PP_ERR_BAD_ARG: a null pointer (but sizes_dev, and an array of
 * length 0), a non-positive batch or slot, a negative length, the two outputs being one, a pointer off its alignment, a workspace
 * that is too small.  PP_ERR_TOO_LARGE: batch above 65535, a slot side above 32768, more than 2^24 vertices or runs or 2^20 rings.
 * PP_ERR_NO_DEVICE without a HIP device (after the argument checks).  Nothing is launched on a refusal.  Asynchronous, nothing
 * allocated: capturable.  pp_coco_masks_workspace_bytes: the size, or PP_ERR_BAD_ARG / PP_ERR_TOO_LARGE (negative). */
PP_API long long pp_coco_masks_workspace_bytes(int n_verts);
PP_API int pp_coco_masks_u8(const double *verts_dev, int n_verts, const int *rings_dev, int n_rings, const long long *images_dev,
                            const long long *runs_dev, int n_runs, const int *sizes_dev, int batch, int slot_h, int slot_w,
                            void *workspace, long long workspace_bytes, void *mask_miss_u8, void *mask_all_u8, void *stream);

/* A2 standalone: the arrays predict_refactor returns (utils/parse_skeletons.py:82-103).  net_out_dev as for
 * pp_process_batch; heat_hwc_dev: DEVICE float[batch][h][w][20], paf_hwc_dev: DEVICE float[batch][h][w][30]. */
PP_API int pp_flip_average(const void *net_out_dev, int dtype, int batch, int h, int w, int flip, float *heat_hwc_dev,
                           float *paf_hwc_dev, void *stream);

/* Diagnostics: register a DEVICE buffer of 8 int64 per workgroup; K_A and K_B then store shader-clock stamps at
 * their phase boundaries (slot 0 start, 1 map in LDS, ...).  NULL (default) disables it. */
PP_API int pp_debug_set_stamps(long long *stamps_dev);
/* Diagnostics / A-B measurements of pp_process_batch's launch structure: 0 (default) two launches -- peaks, then limb matching
 * with the person assembly done by each image's last limb workgroup, images dispatched heaviest first; 1 = limb matching and
 * assembly as separate launches; 2 = as 0 without the load ordering.  Results are identical in every mode. */
PP_API int pp_debug_set_mode(pp_ctx *ctx, int mode);

/* Blocking read-backs of the context's workspace for the last batch (host pointers).
 * pp_read_peaks: joint_list rows [x, y, score, peak_id, part] (evaluate.py:99-103) of one image; returns
 * PP_ERR_OVERFLOW (rows still filled, truncated per part) when a part had more peaks than max_peaks_per_part. */
PP_API int pp_read_peaks(pp_ctx *ctx, int image, float *joint_list_host, int max_rows, int *n_rows);
/* connections of one limb of one image, rows {cid1, cid2, score, length} (pafprocess.h:60-67) */
PP_API int pp_read_connections(pp_ctx *ctx, int image, int limb, float *rows_host, int max_rows, int *n_rows);
/* number of peaks found in every keypoint channel of one image (counts[18]; may exceed max_peaks_per_part: the true count) */
PP_API int pp_read_part_counts(pp_ctx *ctx, int image, int *counts_host);
/* number of accepted connections of every limb of one image (counts[30]); valid after either rule set (C++ or Python twins) */
PP_API int pp_read_connection_counts(pp_ctx *ctx, int image, int *counts_host);
/* Diagnostics: the raw per-workgroup status words of one image, flags[48] = 18 part words (peak kernels) then 30 limb words
 * (limb kernels); pp_record.status is their OR plus the assembly's own flags.  Each word is plainly stored by its
 * workgroup on every launch; none is ever memset or accumulated. */
PP_API int pp_debug_read_flags(pp_ctx *ctx, int image, uint32_t *flags_host);
/* device -> host copy of `batch` records, then synchronises the stream */
PP_API int pp_read_records(pp_ctx *ctx, const pp_record *records_dev, pp_record *records_host, int batch, void *stream);

/* ---------------------------------------------------------------- drop-in, context form
 * Same contract as process_paf below but re-entrant: state lives in ctx. */
PP_API int pp_process_paf_host(pp_ctx *ctx, int p1, int p2, int p3, const float *peaks, int f1, int f2, int f3,
                        const float *pafmap, int min_img_size);
PP_API int pp_get_num_humans(const pp_ctx *ctx);
PP_API int pp_get_part_peak_id(const pp_ctx *ctx, int skeleton_id, int part_id);
PP_API float pp_get_score(const pp_ctx *ctx, int skeleton_id);
PP_API int pp_get_part_x(const pp_ctx *ctx, int cid);
PP_API int pp_get_part_y(const pp_ctx *ctx, int cid);
PP_API float pp_get_part_score(const pp_ctx *ctx, int cid);
PP_API uint32_t pp_get_status(const pp_ctx *ctx);

/* ---------------------------------------------------------------- original (non-refactored) path, SURVEY 8a row A10
 * predict (utils/parse_skeletons.py:180-283) + find_peaks (:286-321) + find_connections / find_humans at IMAGE
 * resolution, with a real scale search (BASELINE config 5).  All buffers are DEVICE memory owned by the caller:
 *   scratch_planar float[batch][50][h][w], scratch_up float[batch][50][4h][4w],
 *   heat_acc double[batch][20][img_h][img_w], paf_acc double[batch][30][img_h][img_w]  (zero them before the first scale),
 *   mask_scratch uchar[batch][18][img_h][img_w], peaks64_scratch 32 bytes x batch x 18 x max_peaks_per_part.
 * pp_original_accumulate adds ONE scale: flip-average, x4 bicubic, crop of (pad_down, pad_right) pixels, bicubic resize to
 * (img_h, img_w), += value / n_scales.  pp_original_finish: 3x3 / >= thre1 NMS + refine_centroid, Python-twin matching
 * on the float64 limb maps, records with PP_ST_FLOAT_COORDS (x / y are float32 bit patterns).
 * pp_resize_u8_cubic: cv2.resize(INTER_CUBIC) of a batch of interleaved 3-channel uint8 images (scale = src / dst). */
PP_API int pp_original_accumulate(pp_ctx *ctx, int batch, const void *net_out_dev, int dtype, int h, int w, int flip,
                                  int pad_down, int pad_right, int img_h, int img_w, int n_scales, float *scratch_planar,
                                  float *scratch_up, double *heat_acc, double *paf_acc, void *stream);
/* All scales of predict's loop in ONE launch: the accumulators are WRITTEN (not added to; no zeroing needed) with
 * ((0 + v_1 / n) + v_2 / n) + ... in float64, bit-identical to n_scales calls of pp_original_accumulate on zeroed accumulators,
 * without the scratch maps and without re-reading the accumulators per scale.  net_out_dev[i]: DEVICE (batch, 2|1, 50, h[i],
 * w[i]); h / w / pad_down / pad_right: HOST arrays of n_scales entries (n_scales <= 6).  PP_ERR_UNSUPPORTED when a scale is so
 * large that its tiles do not fit LDS (more than ~3x the image size): use the per-scale form then. */
PP_API int pp_original_accumulate_all(pp_ctx *ctx, int batch, int n_scales, const void *const *net_out_dev, int dtype, const int *h,
                                      const int *w, int flip, const int *pad_down, const int *pad_right, int img_h, int img_w,
                                      double *heat_acc, double *paf_acc, void *stream);
/* Test-time rotation search (utils/parse_skeletons.py:180-283 with rotation_search != [0]): every (scale, angle) entry is one
 * more accumulation, the x4 map of a rotated entry warped back with cv2.warpAffine(M_rev, (0, 0)) before the crop.  m_inv: HOST,
 * 6 doubles, the matrix INVERTED as warpAffine does it (posepaf/rotation.py); sampling is OpenCV's fixed-point INTER_LINEAR with
 * BORDER_CONSTANT 0 (posepaf_affine.h).  pp_original_accumulate_affine: one entry through the chain, += value / n_div; m_inv
 * NULL is pp_original_accumulate; scratch_warp float[batch][50][4h][4w].  pp_original_accumulate_all_affine: every entry in ONE
 * launch (written, not added to, as pp_original_accumulate_all), m_inv: HOST array of n_entries pointers, NULL = not rotated;
 * n_div = n_entries; bit-identical to the chain; PP_ERR_UNSUPPORTED beyond 6 entries or when an entry's tiles do not fit LDS. */
PP_API int pp_original_accumulate_affine(pp_ctx *ctx, int batch, const void *net_out_dev, int dtype, int h, int w, int flip,
                                         int pad_down, int pad_right, int img_h, int img_w, int n_div, const double *m_inv,
                                         float *scratch_planar, float *scratch_up, float *scratch_warp, double *heat_acc,
                                         double *paf_acc, void *stream);
PP_API int pp_original_accumulate_all_affine(pp_ctx *ctx, int batch, int n_entries, const void *const *net_out_dev, int dtype,
                                             const int *h, const int *w, int flip, const int *pad_down, const int *pad_right,
                                             const double *const *m_inv, int img_h, int img_w, double *heat_acc, double *paf_acc,
                                             void *stream);
/* cv2.warpAffine(src, M, (0, 0)) of DEVICE float32 maps, m_inv as above: hwc = 0: n planes (n, h, w); hwc = 1: (n, h, w,
 * channels) interleaved.  dst (same shape) must not alias src. */
PP_API int pp_warp_affine_f32(const float *src, float *dst, long n, int h, int w, int channels, int hwc, const double *m_inv,
                              void *stream);
PP_API int pp_original_finish(pp_ctx *ctx, int batch, int img_h, int img_w, float thre1, const double *heat_acc,
                              const double *paf_acc, unsigned char *mask_scratch, void *peaks64_scratch, pp_record *records_dev,
                              void *stream);
PP_API int pp_resize_u8_cubic(const void *src, void *dst, int batch, int sh, int sw, int dh, int dw, double scale_x,
                              double scale_y, void *stream);
/* The original path for a RAGGED bucket: images of different sizes whose scaled sizes pad to one shape at every scale, so that one
 * forward per scale serves them all (posepaf/original_path.py bucket_key).  Every image comes out bit for bit as it does alone
 * through the entries above.  Layout:
 *   uint8 images  (batch, slot_h, slot_w, 3), image b in the top-left (h_b, w_b) corner of its slot (as pp_preprocess_u8_ragged
 *                 reads them); the rest of a slot is never read and, on output, never written;
 *   sizes         int[2][batch], heights then widths, as a DEVICE array the kernels read and as a HOST array with the SAME values
 *                 for the argument checks, the grid and the LDS capacities;
 *   heat_acc      double[batch][20][slot_area], paf_acc double[batch][30][slot_area], mask_scratch uchar[batch][18][slot_area]:
 *                 plane (b, c) starts at (b * C + c) * slot_area and holds h_b x w_b values row-major with row length w_b (no
 *                 pitch); the tail of a slot is never read or written; slot_area >= h_b * w_b for every image.
 * pp_resize_u8_cubic_ragged: per image pp_resize_u8_cubic of the source corner into the destination corner; dst_sizes_dev holds
 *   what cv2.resize gives each image (round half to even, computed by the host); scale_x = scale_y = 1 / scale for all of them.
 * pp_original_accumulate_all_ragged: pp_original_accumulate_all with a per-image image size and crop.  pads: int[n_scales][2]
 *   [batch], per scale pad_down then pad_right of every image, HOST and DEVICE.  PP_ERR_UNSUPPORTED where
 *   pp_original_accumulate_all answers it for one of the images: run that bucket as exact-size groups then.  No allocation, no
 *   host synchronisation.
 * pp_original_finish_ragged: pp_original_finish with each image's own extent for the NMS borders, the refine_centroid window
 *   and the limb sampler's clamp, and its own height as find_connections' img_h. */
PP_API int pp_resize_u8_cubic_ragged(const void *src, void *dst, int batch, int src_slot_h, int src_slot_w, int dst_slot_h,
                                     int dst_slot_w, const int *src_sizes_dev, const int *dst_sizes_dev, double scale_x,
                                     double scale_y, void *stream);
PP_API int pp_original_accumulate_all_ragged(pp_ctx *ctx, int batch, int n_scales, const void *const *net_out_dev, int dtype,
                                             const int *h, const int *w, int flip, const int *sizes, const int *sizes_dev,
                                             const int *pads, const int *pads_dev, long slot_area, double *heat_acc,
                                             double *paf_acc, void *stream);
PP_API int pp_original_finish_ragged(pp_ctx *ctx, int batch, const int *sizes, const int *sizes_dev, long slot_area, float thre1,
                                     const double *heat_acc, const double *paf_acc, unsigned char *mask_scratch,
                                     void *peaks64_scratch, pp_record *records_dev, void *stream);

/* ---------------------------------------------------------------- run-time test configuration (Python rules)
 * The matching rules the reference's Python post-processing reads from test_cfg (utils/config:16-27,
 * utils/parse_skeletons.py:309, :328-329, :353, :429-431, :530).  thre1 is not here: it stays pp_original_finish's argument.
 * Read by pp_process_batch_py, pp_original_finish, pp_py_find_connections_host and pp_py_find_humans_host.
 * pp_process_batch (the C++ pafprocess rules) never looks at it: the reference compiles those constants in.
 * With the defaults the kernels with the literals run, exactly as before; a general instance of a kernel is launched only
 * when a value that kernel reads differs from its default. */
typedef struct {
    double thre2;           /* 0.1   limb-map threshold of a sample; compared as NumPy does: a float32 map in float32 with
                                      the value rounded once, a float64 map in double */
    double connect_ration;  /* 0.8   count(samples > thre2) > mid_num * connect_ration */
    double len_rate;        /* 16    a new limb may be at most len_rate times the person's longest so far */
    double connection_tole; /* 0.7   merge of two disjoint people: score >= connection_tole * min limb score */
    int mid_num;            /* 20    samples per candidate limb, 1..128.  128 is NumPy's pairwise-sum block: up to there mean()
                                      is the eight-accumulator loop the kernels restate, above it NumPy recurses */
    int offset_radius;      /* 2     refine_centroid's radius (original path), 0..7: the (2r+1)^2 box, at most 225 values, must
                                      fit one 64-lane wave four times over (up to four values per lane) */
    int remove_recon;       /* 0     0 / 1: take a joint shared by two people away from the weaker one (:526-564) */
} pp_test_cfg;
/* the INI defaults above */
PP_API int pp_default_test_cfg(pp_test_cfg *cfg);
/* A fresh context holds the defaults.  PP_ERR_UNSUPPORTED, context unchanged: mid_num outside 1..128, offset_radius outside
 * 0..7, remove_recon not 0 / 1, a non-finite or negative thre2 / connect_ration / len_rate / connection_tole. */
PP_API int pp_set_test_cfg(pp_ctx *ctx, const pp_test_cfg *cfg);
PP_API int pp_get_test_cfg(const pp_ctx *ctx, pp_test_cfg *cfg);

/* ---------------------------------------------------------------- 1 x 1 head: weight and bias gradient (training the heads)
 * dw[k][c] = fl32(inv_loss_scale * A[k][c]), A[k][c] the float32 accumulation over all m of the exact products g[m][k] * xs[m][c];
 * db[k] = fl32(inv_loss_scale * sum_m g[m][k]).  xs[m][c] = x[m][c] when scale is NULL, else the binary16 rounding (nearest even,
 * one rounding) of the exact product x[m][c] * scale[m / hw][c]: what pp_pw_f16 multiplies and pp_channel_scale_f16 stores.
 *   g      DEVICE binary16 (m, ldg): channels 0 .. c_out - 1 of a pixel are read, the rest never enter arithmetic; 16-byte loads
 *          where the rows are 16-byte aligned (g on a 16-byte boundary and ldg % 8 == 0), element loads elsewhere
 *   x      DEVICE binary16 (m, c_in), packed pixel-major (NHWC);  scale  DEVICE binary16 (m / hw, c_in) or NULL
 *   dw     DEVICE float32 (c_out, c_in);  db  DEVICE float32 (c_out): every element is stored on every call, nothing else is
 * Two plain launches on `stream`: per-workgroup partials into the workspace (never assumed zero, never needs clearing), then a
 * reduction in a fixed order that multiplies by inv_loss_scale once.  No floating-point atomics: the order of the float32 additions
 * follows from (m, c_in, c_out) alone, so the result is bit-equal from run to run, eager or replayed from a graph, at every pointer
 * alignment the entry accepts (g on any 2-byte boundary with any ldg >= c_out, x and scale on any 16-byte one).  Non-finite inputs
 * stay non-finite and stay where they belong: an infinite or NaN g[m][k] makes row k of dw and db[k] non-finite, a non-finite
 * xs[m][c] (an infinite or NaN x, or a product with the gain above 65504) makes column c of dw non-finite in all c_out rows, every
 * other element keeps the bits it has without that input; whether an affected element is an infinity or a NaN is unspecified.
 * Asynchronous, allocates nothing, needs no pp_ctx, capturable.
 * Refusals (nothing launched, outputs untouched), in this order:  PP_ERR_BAD_ARG: a null g, x, dw, db or workspace; m <= 0, hw <= 0,
 * m % hw != 0 with a scale; ldg < c_out; x or scale off a 16-byte boundary, g off a 2-byte one, dw, db or the workspace off a 4-byte
 * one; inv_loss_scale not finite and positive.  PP_ERR_UNSUPPORTED: pp_head_wgrad_supported is 0, or a scale with hw % 64 != 0 (the
 * forward's rule: materialise and pass NULL).  PP_ERR_TOO_LARGE: m > 2^31 - 1.  PP_ERR_BAD_ARG: a workspace smaller than
 * pp_head_wgrad_workspace_bytes.  PP_ERR_NO_DEVICE after those. */
PP_API int pp_head_wgrad_supported(int c_in, int c_out);   /* c_in % 64 == 0, 64..256; c_out 1..64 */
PP_API int pp_head_wgrad_chunk_pixels(void);               /* pixels one workgroup contracts per pass */
PP_API int pp_head_wgrad_max_workgroups(void);             /* upper bound of the first launch's grid */
/* bytes, or a negative pp_status for arguments pp_head_wgrad_f16 refuses */
PP_API long long pp_head_wgrad_workspace_bytes(long m, int c_in, int c_out);
PP_API int pp_head_wgrad_f16(const void *g, int ldg, const void *x, const void *scale, long m, int hw, int c_in, int c_out,
                             float inv_loss_scale, void *workspace, long long workspace_bytes, float *dw, float *db, void *stream);

/* Every head of a training step in one call.  A descriptor holds the per-head arguments of pp_head_wgrad_f16, and for every head dw
 * and db are BIT-EQUAL to what that entry stores for the same arguments, at every shape, alignment and row pitch it accepts: a head
 * keeps its own min(256, ceil(m / 64)) workgroups, their chunks, the four-run reduction order and the exact products; only the
 * launches are shared.  At most one accumulate launch per distinct (c_in, 16-byte / element load of g) pair among the heads, then
 * one finishing launch for all of them; the descriptors travel in the kernel arguments, so a graph capture freezes them.
 *   inv_loss_scale_dev  NULL: the finishing launch multiplies by the host's inv_loss_scale.  Else a DEVICE float the finishing
 *                       launch reads when it runs (the host value is ignored): a captured step whose loss scale moves
 *   workspace           DEVICE, at least pp_head_wgrad_multi_workspace_bytes (the sum of the heads' own sizes, a slice per head in
 *                       table order); never assumed zero, no memset, no atomics; nothing outside every dw and db is written
 * Asynchronous, allocates nothing, needs no pp_ctx, capturable.
 * Refusals (nothing launched, outputs untouched), in this order:  PP_ERR_BAD_ARG: a null table or n_heads <= 0.
 * PP_ERR_UNSUPPORTED: n_heads > pp_head_wgrad_multi_max_heads().  Then, head by head, the first refusal of pp_head_wgrad_f16's list
 * that concerns a descriptor's own fields (null g, x, dw, db; m, hw; ldg; alignment of g, x, scale, dw, db; unsupported; too large).
 * PP_ERR_BAD_ARG: a workspace that is null, off a 4-byte boundary or too small.  PP_ERR_BAD_ARG: inv_loss_scale_dev off a 4-byte
 * boundary; with a NULL inv_loss_scale_dev, an inv_loss_scale that is not finite and positive.  PP_ERR_NO_DEVICE after those. */
#define PP_HEAD_WGRAD_MULTI_MAX 40      /* the loss's 8 stacks x 5 scales */
typedef struct {
    const void *g;
    int ldg;
    const void *x;
    const void *scale;
    long m;
    int hw, c_in, c_out;
    float *dw;
    float *db;
} pp_head_wgrad_desc;
PP_API int pp_head_wgrad_multi_max_heads(void);
/* bytes, or the negative pp_status of the first refusal above up to the heads' own */
PP_API long long pp_head_wgrad_multi_workspace_bytes(int n_heads, const pp_head_wgrad_desc *heads);
PP_API int pp_head_wgrad_multi_f16(int n_heads, const pp_head_wgrad_desc *heads, float inv_loss_scale, const float *inv_loss_scale_dev,
                                   void *workspace, long long workspace_bytes, void *stream);

/* ---------------------------------------------------------------- one layer below a head (csrc/posepaf_convgrad.hip)
 * pp_head_dgrad_f16: the gradient through a 1 x 1 head and the LeakyReLU in front of it.
 *   s[m][c] = the float32 accumulation, k = 0, 1, ... c_out - 1 in this order, of the EXACT products g[m][k] * w[k][c];
 *   t = s where y[m][c] > 0, else fl32(slope * s);   dx[m][c] = half_rn(t)   (above 65504: an infinity, which the step's finite test
 *   then meets in the gradients formed from dx)
 *   g      DEVICE binary16 (m, ldg), pp_head_wgrad_f16's operand: channels at or behind c_out are never loaded; any 2-byte boundary
 *          and any ldg >= c_out
 *   w      DEVICE binary16 (c_out, c_in), the head's weight;  y  DEVICE binary16 (m, c_in) packed, the head's input, that is the
 *          OUTPUT of the LeakyReLU: slope > 0 keeps the sign of the pre-activation, y = +-0 takes the slope as torch's backward does
 *   dx     DEVICE binary16 (m, c_in) packed: every element is stored on every call, nothing else is
 * |dx - exact| <= E + max(2^-11 (|t| + E), 2^-25),  E = a 2^-24 (c_out sum_k |g w| + |s|),  a = 1 or slope: c_out float32 additions,
 * one float32 multiply, one binary16 rounding.  One launch, no workspace, no atomics; asynchronous, allocates nothing, needs no
 * pp_ctx, capturable.  Refusals (nothing launched, dx untouched), in this order:  PP_ERR_BAD_ARG: a null g, w, y or dx; m <= 0;
 * ldg < c_out; g off a 2-byte boundary, w, y or dx off a 16-byte one; slope not finite and positive.  PP_ERR_UNSUPPORTED:
 * pp_head_dgrad_supported is 0.  PP_ERR_TOO_LARGE: m > 2^31 - 1.  PP_ERR_NO_DEVICE after those. */
PP_API int pp_head_dgrad_supported(int c_in, int c_out);   /* c_in % 64 == 0, 64..256; c_out 1..64 */
PP_API int pp_head_dgrad_f16(const void *g, int ldg, const void *w, const void *y, long m, int c_in, int c_out, float slope, void *dx,
                             void *stream);

/* pp_conv3x3_wgrad_f16: the weight and bias gradient of a 3 x 3 / pad 1 / stride 1 convolution.
 *   dw[k][r][s][c] = fl32(inv * A),  A the float32 accumulation of the EXACT products dy[b, i, j, k] * x[b, i + r - 1, j + s - 1, c] over
 *   all pixels whose neighbour lies inside image b (a neighbour outside is not loaded: nothing next to the tensor is ever read);
 *   db[k] = fl32(inv * sum dy[.][k]);   inv = *inv_loss_scale_dev when that is non-NULL (read when the launch runs), else inv_loss_scale
 *   dy     DEVICE binary16 (n h w, c_out) packed;  x  DEVICE binary16 NHWC (n, h, w, c_in) packed, the convolution's input
 *   dw     DEVICE float32 (c_out, 3, 3, c_in): the memory order of a channels-last (c_out, c_in, 3, 3) weight;  db  DEVICE float32
 *          (c_out): every element is stored on every call, nothing else is
 * Two plain launches: 9 c_out / 64 sub-problems (tap, 64 output channels) of min(pp_conv3x3_wgrad_max_workgroups(), ceil(n h w / 64))
 * workgroups each run the head gradient's pass with 64 x c_in + 64 partials per workgroup in the workspace (never assumed zero, no
 * memset), then a reduction in a fixed order multiplies by inv once.  No floating-point atomics: (n, h, w, c_in, c_out) fixes the
 * order of the additions, so the bits are equal from run to run, eager or replayed.  A non-finite dy[.][k] makes row k of dw and
 * db[k] non-finite and leaves every other row its bits.  Asynchronous, allocates nothing, needs no pp_ctx, capturable.
 * Refusals (nothing launched, outputs untouched), in this order:  PP_ERR_BAD_ARG: a null dy, x, dw, db or workspace; n, h or w <= 0;
 * dy or x off a 16-byte boundary, dw, db, the workspace or inv_loss_scale_dev off a 4-byte one; with a NULL inv_loss_scale_dev an
 * inv_loss_scale that is not finite and positive.  PP_ERR_UNSUPPORTED: pp_conv3x3_wgrad_supported is 0.  PP_ERR_TOO_LARGE:
 * n h w > 2^31 - 1.  PP_ERR_BAD_ARG: a workspace smaller than pp_conv3x3_wgrad_workspace_bytes.  PP_ERR_NO_DEVICE after those. */
PP_API int pp_conv3x3_wgrad_supported(int c_in, int c_out);   /* c_in % 64 == 0, 64..256; c_out % 64 == 0, 64..256 */
PP_API int pp_conv3x3_wgrad_max_workgroups(void);             /* per sub-problem */
/* bytes, or a negative pp_status for arguments pp_conv3x3_wgrad_f16 refuses */
PP_API long long pp_conv3x3_wgrad_workspace_bytes(int n, int h, int w, int c_in, int c_out);
PP_API int pp_conv3x3_wgrad_f16(const void *dy, const void *x, int n, int h, int w, int c_in, int c_out, float inv_loss_scale,
                                const float *inv_loss_scale_dev, void *workspace, long long workspace_bytes, float *dw, float *db,
                                void *stream);

/* pp_conv3x3_dgrad_f16: the data gradient of a 3 x 3 / pad 1 / stride 1 convolution and the LeakyReLU in front of it.
 *   s[b, i, j, c] = the float32 accumulation of the EXACT products dy[b, i + 1 - r, j + 1 - q, k] * w[k][r][q][c] over the (r, q, k)
 *   whose dy pixel lies inside image b (a pixel outside is not loaded: nothing next to the tensor and nothing of image b +- 1 is read);
 *   t = s where y > 0 or y == NULL, else fl32(slope * s) (y = +-0 takes the slope, as in pp_head_dgrad_f16);   dx = half_rn(t)
 *   (above 65504: an infinity, which the step's finite test then meets)
 *   dy     DEVICE binary16 (n h w, c_out) packed: what pp_head_dgrad_f16 writes
 *   w      DEVICE binary16 (c_out, 3, 3, c_in): the memory of a channels-last (c_out, c_in, 3, 3) weight, as it is -- no rotated or
 *          transposed copy
 *   y      DEVICE binary16 NHWC (n, h, w, c_in) packed, or NULL: the OUTPUT of the LeakyReLU that produced this convolution's input
 *   dx     DEVICE binary16 NHWC (n, h, w, c_in) packed: every element is stored on every call, nothing else is
 * One launch: a workgroup owns an 8 x 8 pixel tile of one image, all c_in channels and the whole reduction of 9 c_out; products on
 * the matrix unit from operands split into bfloat16 hi + lo (four MFMAs per pair, every product exact, subnormals included), taps
 * 0 .. 8 and k ascending.  (n, h, w, c_in, c_out) alone fixes the order of the additions: equal bits from call to call, eager or
 * replayed.  No atomics, no split of the reduction across workgroups, no workspace.  For any order and an accumulate that may
 * truncate:  |dx - exact| <= E + max(2^-11 (|t| + E), 2^-25),  E = a (9 c_out 2^-23 sum |dy w| + 2^-24 |s|),  a = 1 or slope.
 * Asynchronous, allocates nothing, needs no pp_ctx, capturable once a call of that c_in has run eagerly on the device: the
 * first one raises the kernel's LDS limit (once per device) and is refused with PP_ERR_UNSUPPORTED inside a stream capture.  Refusals (nothing launched, dx untouched), in this order:  PP_ERR_BAD_ARG: a null dy, w or
 * dx; n, h or wd <= 0; dy, w, y or dx off a 16-byte boundary; a non-NULL y with a slope that is not finite and positive.
 * PP_ERR_UNSUPPORTED: pp_conv3x3_dgrad_supported is 0.  PP_ERR_TOO_LARGE: n h wd > 2^31 - 1.  PP_ERR_NO_DEVICE after those. */
PP_API int pp_conv3x3_dgrad_supported(int c_in, int c_out);   /* both % 64 == 0, 64..256: pp_conv3x3_wgrad_supported's set */
PP_API int pp_conv3x3_dgrad_f16(const void *dy, const void *w, const void *y, int n, int h, int wd, int c_in, int c_out, float slope,
                                void *dx, void *stream);

/* ---------------------------------------------------------------- the heads' optimiser step on the device (csrc/posepaf_headopt.hip)
 * One chain of two launches: the finite test of all n gradients, then -- when every one is finite -- torch.optim.SGD's update
 * (dampening 0, no Nesterov) of the float32 masters, their binary16 copies, and the loss-scale state machine.
 *   g' = fma(wd, p, g)  (wd = 0: g' = g);   buf' = fl(mu * buf) + g'  (mu = 0: no buffer is read or written, buf' = g');
 *   p' = fma(-lr, buf', p)                  -- each operation rounded where this torch build's SGD kernels round it
 *   masters, momentum   DEVICE float32 (n), updated in place;  grads  DEVICE float32 (n), read only
 *   table      DEVICE pp_head_update_desc[n_heads]: where a head's weight and bias lie in the flat tensors and the four binary16
 *              destinations of their nearest-even roundings: weight and wpad receive w_len elements from w_off, bias and bpad b_len
 *              from b_off (the first rows of the zero-padded copies; the rows behind are never touched).  Ranges in ascending
 *              order, disjoint, inside [0, n); an element of no range is updated and copied nowhere.  A layer without padded copies
 *              (a 3 x 3 convolution) names its weight as wpad and its bias as bpad too: the second store repeats the first
 *   hyper      DEVICE float[3] = lr, momentum, weight_decay (read when the launch runs: a schedule needs no new capture)
 *   state      DEVICE pp_head_update_state.  A non-finite gradient: masters, momentum and every binary16 copy keep their bits,
 *              skipped += 1, scale = max(scale / 2, min_scale), good_steps = 0.  A finite step: good_steps += 1, and when it reaches
 *              growth_interval: scale = min(2 scale, max_scale), good_steps = 0.  inv_scale = 1 / scale.  growth_interval = 0: static,
 *              scale, inv_scale and good_steps never move (skipped still counts)
 *   workspace  DEVICE, pp_head_update_workspace_bytes(n): one flag word per workgroup of the first launch, stored with plain
 *              stores on every call and OR-ed by the second; no memset, no atomics
 * Asynchronous, allocates nothing, needs no pp_ctx, capturable.  Refusals before any launch: PP_ERR_BAD_ARG for a null pointer,
 * n <= 0, n_heads < 0, masters / grads / momentum / hyper / workspace off a 4-byte boundary, table / state off an 8-byte one;
 * PP_ERR_UNSUPPORTED for n_heads > pp_head_wgrad_multi_max_heads(); PP_ERR_TOO_LARGE for n > 2^31 - 1; PP_ERR_NO_DEVICE last. */
typedef struct {
    long long w_off, w_len, b_off, b_len;
    void *weight, *bias, *wpad, *bpad;
} pp_head_update_desc;
typedef struct {
    float scale, inv_scale;
    int good_steps, growth_interval;
    float min_scale, max_scale;
    long long skipped;
} pp_head_update_state;
PP_API long long pp_head_update_workspace_bytes(long n);
PP_API int pp_head_update_f32(float *masters, const float *grads, float *momentum, long n, const pp_head_update_desc *table, int n_heads,
                              const float *hyper, pp_head_update_state *state, void *workspace, void *stream);

/* pp_layer_update_f32: pp_head_update_f32 -- the same two launches, finite test over all n, three SGD roundings, loss-scale state
 * machine and workspace (pp_head_update_workspace_bytes(n)) -- for more layers than 40 heads: the table is a DEVICE array of single
 * segments, ascending, disjoint, inside [0, n).  Elements off .. off + len - 1 of the masters are rounded to binary16 (nearest
 * even) into dst and dst2, which may be equal (a layer without a padded copy).  One copy of the device arithmetic serves both
 * entries.  Refusals before any launch: PP_ERR_BAD_ARG for a null pointer, n <= 0, n_segments < 0, masters / grads / momentum /
 * hyper / workspace off a 4-byte boundary, segments / state off an 8-byte one; PP_ERR_UNSUPPORTED for n_segments >
 * PP_LAYER_UPDATE_MAX_SEGMENTS; PP_ERR_TOO_LARGE for n > 2^31 - 1; PP_ERR_NO_DEVICE last. */
#define PP_LAYER_UPDATE_MAX_SEGMENTS 256     /* 8 stacks x 5 scales x 3 layers x (weight, bias) = 240 */
typedef struct {
    long long off, len;
    void *dst, *dst2;
} pp_update_segment;
PP_API int pp_layer_update_max_segments(void);
PP_API int pp_layer_update_f32(float *masters, const float *grads, float *momentum, long n, const pp_update_segment *segments,
                               int n_segments, const float *hyper, pp_head_update_state *state, void *workspace, void *stream);

/* ---------------------------------------------------------------- Python twins, host form
 * utils.parse_skeletons.find_connections / find_humans (:324-600) with host arrays, for callers of the non --run_cpp
 * branch of evaluate.py (:88-89).  peaks: joint-list rows [x, y, score, id, part] (n of them); paf: (H, W, C) float32.
 * conns: double[30][max_peaks_per_part][6] rows {src_id, dst_id, score, i, j, limb_len}; counts: int[30];
 * special: int[30] (1 where neither part has a peak); persons: rows of 40 doubles = person_to_joint_assoc (20, 2). */
PP_API int pp_py_find_connections_host(pp_ctx *ctx, const float *peaks, int n, const float *paf, int H, int W, int C,
                                       int img_height, double *conns_out, int *counts_out, int *special_out);
PP_API int pp_py_find_humans_host(pp_ctx *ctx, const double *conns, const int *counts, const float *peaks, int n,
                                  double *persons_out, int cap, int *n_out);

/* ---------------------------------------------------------------- drop-in, reference names
 * Replaces /root/reference/utils/pafprocess/pafprocess.h:70-76 one for one.
 *   peaks  : host float[p1][p2][p3], rows [x, y, score, peak_id, part]   (evaluate.py:99-107, p3 = 5)
 *   pafmap : host float[f1][f2][f3] = (H, W, 30) up-sampled limb maps     (evaluate.py:77-80, :109)
 * Results stay in one process-wide context until the next call (the reference keeps them in file-scope
 * globals, pafprocess.cpp:16-17); like the reference this group is not re-entrant.
 * process_paf returns 0 on success like the reference (pafprocess.cpp:284); unlike the reference it can
 * fail, and then returns a negative pp_status (no device, capacity exceeded) instead of computing on the CPU. */
PP_API int process_paf(int p1, int p2, int p3, float *peaks, int f1, int f2, int f3, float *pafmap, int min_img_size);
PP_API int get_num_humans(void);
PP_API int get_part_peak_id(int skeleton_id, int part_id);
PP_API float get_score(int skeleton_id);
PP_API int get_part_x(int cid);
PP_API int get_part_y(int cid);
PP_API float get_part_score(int cid);

#ifdef __cplusplus
}
#endif
#endif /* POSEPAF_H */

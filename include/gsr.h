/*
 * gsr.h -- C ABI of libgsr.so: the MI355X (gfx950) articulated Gaussian-splat hot path.
 *
 * Drop-in boundary.  Every entry point replaces one interface of the reference
 * (paths relative to the reference tree; DGR = submodules/diff-gaussian-rasterization,
 * CR = DGR/cuda_rasterizer, SK = submodules/simple-knn):
 *
 *   gsr_rasterize_forward   <- CudaRasterizer::Rasterizer::forward      CR/rasterizer.h:32-56, CR/rasterizer_impl.cu:198-341
 *   gsr_rasterize_backward  <- CudaRasterizer::Rasterizer::backward     CR/rasterizer.h:58-89, CR/rasterizer_impl.cu:345-447
 *   gsr_mark_visible        <- CudaRasterizer::Rasterizer::markVisible  CR/rasterizer.h:25-30, CR/rasterizer_impl.cu:141-153
 *   gsr_dist2               <- SimpleKNN::knn                           SK/simple_knn.h:17, SK/simple_knn.cu:185-221
 *   gsr_lbs_*               <- GaussianModel.coarse_deform_c2source     scene/gaussian_model.py:768-872
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless named host_*;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); all work is enqueued on it;
 *   - the three growable scratch buffers of the reference (geometry / binning / image state,
 *     std::function<char*(size_t)> callbacks in CR/rasterizer.h:33-35) are requested through
 *     gsr_alloc_fn callbacks: the library calls alloc(user, bytes) once per buffer per forward call
 *     and the caller returns a device pointer that stays valid until the matching backward;
 *     the contents are private to the library;
 *   - a null `shs` / `colors_precomp` / `scales` / `rotations` / `cov3D_precomp` pointer selects the
 *     other input mode exactly like the reference (CR/forward.cu:205,241);
 *   - every function returns GSR_OK (0) or a negative GSR_E* code; gsr_last_error() returns a
 *     thread-local message for the last failure on the calling thread.  With debug != 0 the
 *     library synchronises and checks after every kernel (CR/auxiliary.h:166-173).
 */
#ifndef GSR_H_INCLUDED
#define GSR_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_OK 0
#define GSR_EINVAL (-1)  /* bad argument (shape/size/null) */
#define GSR_EHIP (-2)    /* a HIP runtime call or kernel failed */
#define GSR_ENOMEM (-3)  /* an allocation callback returned null / workspace too small */

typedef void *gsr_stream_t;
typedef char *(*gsr_alloc_fn)(void *user, size_t bytes);

/* Library version (major*10000 + minor*100 + patch) and the gfx target it was built for ("gfx950"). */
int gsr_version(void);
/* 1 if the library was built with GSR_BUILD_EXPERIMENTS (python -m mygauhuman_amd.build --experiments): the kernels that were built,
 * measured and NOT adopted (the MFMA reductions, the global -> LDS DMA forward, the 4x4-block forward, round 3's
 * backward, the "render the longest lists alone" measurement) are then compiled in and selectable through gsr_set_tuning.  The
 * default build does not contain them, and their knob values are refused. */
int gsr_has_experiments(void);
const char *gsr_target_arch(void);
const char *gsr_last_error(void);

/* Binning back-ends (gsr_set_binning_mode; default GSR_BINNING_TILE_BUCKET):
 *   GSR_BINNING_GLOBAL_RADIX: duplicate keys + device-wide stable LSD radix sort on the low 32+bit key bits +
 *                             identifyTileRanges -- the reference's structure (CR/rasterizer_impl.cu:291-320);
 *   GSR_BINNING_TILE_BUCKET : per-tile counting + per-tile register / LDS sort on (depth bits, Gaussian id).
 * With the tuning knob "tile_cull" = 0 both produce the reference's point lists and tile ranges bit for bit.  With
 * "tile_cull" = 1 (default, tile-bucket only) instances whose tile the Gaussian cannot reach with alpha >= 1/255 are dropped:
 * images, radii and gradients are unchanged, the per-tile lists are sublists of the reference's. */
#define GSR_BINNING_GLOBAL_RADIX 0
#define GSR_BINNING_TILE_BUCKET 1
int gsr_set_binning_mode(int mode);
int gsr_get_binning_mode(void);

/* Knobs (images, radii and gradients never change beyond summation order):
 *   "binning_mode" (= gsr_set_binning_mode);
 *   "blend_fwd_waves" / "blend_bwd_waves" in {1, 2, 4}: waves that cooperate on one 16x16 tile (a lane owns 4 / waves pixels);
 *   "blend_bwd_reduce" in {0, 3}: cross-lane reduction of the backward: 3 = two hops through LDS (default: the per-Gaussian
 *       sums of a quadrant are formed by reader lanes from transposed (r, w) planes; plain-pass only, other configurations use 0),
 *       0 = v_permlane swaps + DPP on the VALU.  Experiment builds only (gsr_has_experiments): 1 = MFMA on the folded rows,
 *       2 = transposed MFMA contraction, 4 = round 3's kernel of the LDS design (all slower on gfx950);
 *   "bucket_hist" in {0, 1}: tile-bucket counting without global atomics (per-workgroup LDS histograms + a dense prefix table,
 *       default) or with one returning global atomic per instance (also taken for tile grids beyond 8192 tiles);
 *   "bucket_cstride" in {1, 2, 4, 8, 16}: spacing (in 4-byte words) of the per-tile counters of the atomic variant;
 *   "bucket_sort_merged" in {0, 1}: histogram path -- the sort of the short lists (a wave per tile) and of the long ones (a
 *       workgroup per list, from a work list) in one launch (default) or in two;
 *   "blend_sort" in {0, 1}: histogram path with the plain four-wave forward (no extra channels): lists of up to 512 entries are
 *       sorted by the forward workgroup that walks them (default 1), not by a binning launch; longer lists keep their own launch;
 *   "tile_order" in {0, 1, 2, 3}: the order in which the blend kernels visit the tiles (tile-bucket back-end, histogram path): 1 =
 *       longest list first, dealt round-robin to the XCDs (default), 0 = the natural order (a contiguous band of tile rows per
 *       XCD), 2 / 3 = blocks of 2 x 2 / 4 x 2 tiles by summed length, a block per XCD; results do not depend on it;
 *   "blend_segments" in 0 .. 64: 0 = every list is walked whole by the backward; v > 0 (default 8) = a list of at least v / 4 times
 *       the frame's mean list is walked in up to four segments by different waves, each started from a checkpoint of the blend
 *       state the forward writes at the segment boundary (gradients agree with the whole walk to rounding; needs tile_order 1);
 *   "blend_tail_cut" in 0 .. 16 (default 0), "blend_prio" in {0, 1} (default 1); experiment builds only: "blend_prio" 2..4
 *       (MEASUREMENT ONLY, renders wrong images), "blend_layout" = 1 (forward with a wave per 4x4 pixel block), "blend_fwd_dma" = 1
 *       (see DESIGN.md section 4);
 *   "tile_cull" in {0, 1}: exact ellipse-vs-tile culling of instances in the tile-bucket back-end (see above);
 *   "deterministic" in {0, 1}: the backward reduces its per-(Gaussian, tile-quadrant) partial sums in a fixed order instead of
 *       with float atomics: run-to-run bit-identical gradients (for tests; costs a 256-byte slot per instance quadrant).
 *       PLAIN PASS ONLY, by design: the mode exists so that tests can demand bit equality where two code paths must produce the same
 *       sums (the fused alpha-mask loss against loss kernel + backward; a knob against its default).  The fused 18-channel backward
 *       (gsr_rasterize_backward_ex with extra features) returns GSR_EINVAL under it: a slot would be 27 columns wide (432 bytes per
 *       instance quadrant, ~1 GB for a render() frame of 200k Gaussians), and what that pass has to be checked against -- seven
 *       plain passes and the oracle, at 1e-4 -- differs from it in summation order anyway (tests/test_gpu_multi.py,
 *       tests/test_gpu_render.py).
 * gsr_set_tuning sets the PROCESS DEFAULTS.  gsr_set_stream_tuning gives one stream its own set (initialised from the
 * defaults at its first call); every API call resolves its knobs once, at entry, from the stream it is given, so calls on
 * different streams are independent of each other whatever threads they come from (no mutable global state is consulted
 * below the API layer).  gsr_clear_stream_tuning returns a stream to the defaults. */
int gsr_set_tuning(const char *key, int value);
int gsr_set_stream_tuning(gsr_stream_t stream, const char *key, int value);
int gsr_clear_stream_tuning(gsr_stream_t stream);

/* Optional stage timing with HIP events recorded on the caller's stream around the selected stages' kernels
 * (no synchronisation until gsr_profile_read).  Stage ids: 0 forward preprocess, 1 scan, 2 binning (duplicate+sort+
 * ranges or the tile-bucket kernels), 3 blend forward, 4 blend backward, 5 backward preprocess, 6 blend backward, colours
 * only (gsr_rasterize_backward_colors, its zero fills included).  stage_mask bit i enables stage i; 0 disables.
 * gsr_profile_read returns the accumulated milliseconds and launch count of a stage. */
int gsr_profile_enable(unsigned stage_mask);
/* Measurement only: while a zero-filled device buffer is registered here, every wave of the blend kernels (default variants)
 * leaves {start, end} in 100 MHz ticks + its list length: forward waves in the first half of the buffer (4 words per wave,
 * wave index = workgroup * 4 + wave), backward waves in the second half.  words >= 2 * 16 * visiting slots of the image (32 * (4 * tiles
 * + 64) always suffices; a rasterizer call that finds the buffer too small fails with GSR_EINVAL); NULL switches it off. */
int gsr_debug_wave_trace(unsigned long long *device_buffer, size_t words);
/* Measurement only: the shader clock the device runs at right now.  `workgroups` (1 .. 2048) single-wave workgroups each run a
 * dependent chain of `fmas` v_fma_f32 bracketed by the constant 100 MHz counter and by s_memtime (which ticks with the shader
 * clock on gfx950): device_out[2 i] = 10 ns ticks, device_out[2 i + 1] = shader cycles of workgroup i;
 * clock = cycles / (ticks x 10 ns).  bench.py prints it next to every figure that scales with the clock and runs the probe until
 * the clock has settled before its warm-up steps (a freshly leased MI355X needs ~20 ms of load to go from 2.26 to 2.39 GHz). */
int gsr_debug_clock_probe(int workgroups, int fmas, unsigned long long *device_out, gsr_stream_t stream);
int gsr_profile_reset(void);
int gsr_profile_read(int stage, double *total_ms, long *launches);

/* present[i] = (view-space z of means3D[i]) > 0.2          (CR/rasterizer_impl.cu:54-66, CR/auxiliary.h:139-164) */
int gsr_mark_visible(int P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                     uint8_t *present, gsr_stream_t stream);

/* Forward rasterisation.  Argument meaning and order follow Rasterizer::forward (CR/rasterizer.h:32-56):
 *   P Gaussians, D active SH degree, M SH coefficients per Gaussian (shs is [P][M][3]);
 *   background[3]; means3D[P][3]; colors_precomp[P][3]; opacities[P]; scales[P][3]; rotations[P][4] (r,x,y,z);
 *   cov3D_precomp[P][6]; viewmatrix/projmatrix[16] (row-vector convention); cam_pos[3];
 *   scale_modifier: the covariance is built from the float32 product scale_modifier * scales (CR/forward.cu:122-124), and the
 *   backward's dL_dscale is the gradient with respect to THAT product -- it carries no factor of scale_modifier
 *   (CR/backward.cu:295,323-325).  So a call with (scale_modifier, scales) equals the call with (1, scale_modifier * scales) in
 *   every output, dL_dscale included.  D and scale_modifier are by-value kernel arguments: a captured graph keeps them;
 *   D < the stored degree reads only the first (D + 1)^2 of the M coefficients of a row (the others may hold anything) and
 *   the backward writes exact zeros into the rest of dL_dsh's row;
 *   out_color[3][H][W], out_depth[H][W], out_alpha[H][W] (alpha = sum of blending weights), radii[P] (may be null).
 * Every element of the outputs is written when P > 0 (the reference binding zero-fills them first,
 * DGR/rasterize_points.cu:69-72; callers only need that for P == 0);
 * *host_num_rendered receives the number of (Gaussian, tile) instances (the reference's return value). */
int gsr_rasterize_forward(gsr_alloc_fn geometry_alloc, void *geometry_user, gsr_alloc_fn binning_alloc,
                          void *binning_user, gsr_alloc_fn image_alloc, void *image_user, int P, int D, int M,
                          const float *background, int width, int height, const float *means3D, const float *shs,
                          const float *colors_precomp, const float *opacities, const float *scales,
                          float scale_modifier, const float *rotations, const float *cov3D_precomp,
                          const float *viewmatrix, const float *projmatrix, const float *cam_pos, float tan_fovx,
                          float tan_fovy, int prefiltered, float *out_color, float *out_depth, float *out_alpha,
                          int *radii, int debug, int *host_num_rendered, gsr_stream_t stream);

/* Asynchronous forward (extension: no counterpart in the reference, which blocks on a device->host copy of R every
 * call, CR/rasterizer_impl.cu:283).  The caller owns the three scratch buffers (gsr_geometry_bytes(P),
 * gsr_binning_bytes(capacity, w, h), gsr_image_bytes(w, h)) and picks `binning_capacity` = the number of
 * (Gaussian, tile) instances the binning buffer can hold; nothing is read back and the host never waits.
 * dev_status is device uint32[2]: [0] = R, [1] = flags: bit 0 = R > capacity, in which case NOTHING was rendered (outputs
 * hold the background) and the call must be repeated with a larger capacity; bit 1 = a point was filtered although
 * `prefiltered` was set (the reference traps the device there, CR/auxiliary.h:156-160; here the point is culled and the call is
 * flagged -- the blocking entry points return GSR_EINVAL with the reference's message).  Always uses the tile-bucket binning.
 * The matching backward is gsr_rasterize_backward with R = binning_capacity. */
size_t gsr_geometry_bytes(int P);
size_t gsr_image_bytes(int width, int height);
size_t gsr_binning_bytes(size_t binning_capacity, int width, int height);
int gsr_rasterize_forward_async(char *geom_buffer, char *binning_buffer, size_t binning_capacity, char *image_buffer, int P,
                                int D, int M, const float *background, int width, int height, const float *means3D,
                                const float *shs, const float *colors_precomp, const float *opacities, const float *scales,
                                float scale_modifier, const float *rotations, const float *cov3D_precomp,
                                const float *viewmatrix, const float *projmatrix, const float *cam_pos, float tan_fovx,
                                float tan_fovy, int prefiltered, float *out_color, float *out_depth, float *out_alpha,
                                int *radii, int debug, uint32_t *dev_status, gsr_stream_t stream);

/* Backward rasterisation, Rasterizer::backward (CR/rasterizer.h:58-89).  R = num_rendered of the forward call;
 * geom/binning/image buffers are the ones the forward call filled.  The library writes every element of the dL_d*
 * outputs it owns, zeros for culled Gaussians (the reference relies on zero-filled tensors,
 * DGR/rasterize_points.cu:159-167); dL_dsh / dL_dscale / dL_drot are only touched when shs / scales are given:
 * dL_dmean2D[P][3], dL_dconic[P][4], dL_dopacity[P], dL_dcolor[P][3],
 * dL_dmean3D[P][3], dL_dcov3D[P][6], dL_dsh[P][M][3], dL_dscale[P][3], dL_drot[P][4].
 * `alphas` is accepted and ignored like in the reference kernel (CR/backward.cu:410). */
int gsr_rasterize_backward(int P, int D, int M, int R, const float *background, int width, int height,
                           const float *means3D, const float *shs, const float *colors_precomp,
                           const float *alphas, const float *scales, float scale_modifier, const float *rotations,
                           const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
                           const float *campos, float tan_fovx, float tan_fovy, const int *radii,
                           char *geom_buffer, char *binning_buffer, char *image_buffer, const float *dL_dpix,
                           const float *dL_ddepths, const float *dL_dalphas, float *dL_dmean2D, float *dL_dconic,
                           float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D, float *dL_dcov3D,
                           float *dL_dsh, float *dL_dscale, float *dL_drot, int debug, gsr_stream_t stream);

/* Fused multi-feature variants (extension).  The reference's render() rasterises the same geometry
 * seven times per frame with different colours (gaussian_renderer/__init__.py:203-272).  The _ex entry points blend
 * n_extra extra colour channels (extra_features[P][n_extra], n_extra == 18 = six RGB triples, each triple composited
 * over `background` like the main colour) in the SAME pass: out_extra[n_extra][H][W]; the backward takes
 * dL_dout_extra = HOST array of n_extra / 3 device pointers, one [3][H][W] gradient image per colour triple, and returns
 * dL_dextra[P][n_extra], every geometric gradient being the sum over all images.  A null entry = that image received no
 * gradient: it is treated as zero and costs no work -- a training loss typically touches two or three of the six feature
 * images (train.py:256-286).  sh_dtype: GSR_SH_F32 or GSR_SH_F16 (how the `shs` pointer is to be read).
 * With extra_features == NULL / n_extra == 0 and GSR_SH_F32 the _ex entry points are
 * identical to the plain ones. */
#define GSR_SH_F32 0 /* shs: float32 [P][M][3] */
#define GSR_SH_F16 1 /* shs: IEEE half [P][16][3] (extension: fp16 SH storage, BASELINE configs[4]); M must be 16, the array
                      * 16-byte aligned; coefficients are widened exactly on load, dL_dsh stays float32 */
/* Flag for the `debug` argument of the backward entry points (bit 0 = the reference's debug mode: synchronise and check after
 * every kernel).  GSR_BWD_ROWS_ZEROED: the caller guarantees that the gradient accumulation rows inside geom_buffer are all zero
 * on entry -- true for a geometry buffer that was zero-filled once and has since only been used by backward calls carrying this
 * flag -- and the call leaves them zero again (the backward preprocess clears every row it consumes): no 64-byte-per-Gaussian
 * memset per backward.  Without the flag the rows are zeroed by the call, as before. */
#define GSR_BWD_ROWS_ZEROED 2
/* Flag for the `debug` argument of the FORWARD entry points (bit 0 = debug mode as above): the forward preprocess also zeroes the
 * gradient accumulation rows inside geom_buffer (128 B per Gaussian, written by the thread that writes the Gaussian's record
 * anyway), so that the backward of this frame may carry GSR_BWD_ROWS_ZEROED whatever the buffer held before -- for callers that
 * know a backward will follow (the autograd wrappers) and allocate a fresh geometry buffer per frame. */
#define GSR_FWD_ZERO_ROWS 2

int gsr_rasterize_forward_ex(gsr_alloc_fn geometry_alloc, void *geometry_user, gsr_alloc_fn binning_alloc, void *binning_user,
                             gsr_alloc_fn image_alloc, void *image_user, int P, int D, int M, const float *background, int width,
                             int height, const float *means3D, const float *shs, const float *colors_precomp,
                             const float *opacities, const float *scales, float scale_modifier, const float *rotations,
                             const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, const float *cam_pos,
                             float tan_fovx, float tan_fovy, int prefiltered, float *out_color, float *out_depth,
                             float *out_alpha, int *radii, int debug, int *host_num_rendered, const float *extra_features,
                             int n_extra, float *out_extra, int sh_dtype, gsr_stream_t stream);
int gsr_rasterize_forward_async_ex(char *geom_buffer, char *binning_buffer, size_t binning_capacity, char *image_buffer, int P,
                                   int D, int M, const float *background, int width, int height, const float *means3D,
                                   const float *shs, const float *colors_precomp, const float *opacities, const float *scales,
                                   float scale_modifier, const float *rotations, const float *cov3D_precomp,
                                   const float *viewmatrix, const float *projmatrix, const float *cam_pos, float tan_fovx,
                                   float tan_fovy, int prefiltered, float *out_color, float *out_depth, float *out_alpha,
                                   int *radii, int debug, uint32_t *dev_status, const float *extra_features, int n_extra,
                                   float *out_extra, int sh_dtype, gsr_stream_t stream);
int gsr_rasterize_backward_ex(int P, int D, int M, int R, const float *background, int width, int height, const float *means3D,
                              const float *shs, const float *colors_precomp, const float *alphas, const float *scales,
                              float scale_modifier, const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                              const float *projmatrix, const float *campos, float tan_fovx, float tan_fovy, const int *radii,
                              char *geom_buffer, char *binning_buffer, char *image_buffer, const float *dL_dpix,
                              const float *dL_ddepths, const float *dL_dalphas, float *dL_dmean2D, float *dL_dconic,
                              float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D, float *dL_dcov3D, float *dL_dsh,
                              float *dL_dscale, float *dL_drot, int debug, const float *extra_features, int n_extra,
                              const float *const *dL_dout_extra, float *dL_dextra, int sh_dtype, gsr_stream_t stream);

/* The colour columns of the backward alone (extension), for a phase that trains nothing but colours: after pbr_iteration the
 * reference freezes positions, SH, opacity, scales, rotations and the pose networks (scene/gaussian_model.py:296-306) and its loss
 * reaches the Gaussians only through the feature images (train.py:294-363), so all a frame needs is
 *     dL_dcolor[i][c] = sum over pixels of w_i(pixel) dL_dpix[c](pixel),   dL_dextra[i][3 t + c] likewise from dL_dout_extra[t],
 * with w_i = T_i alpha_i the forward's own blending weight.  The call replays the forward's front-to-back walk (same contributors,
 * same weights) and forms nothing else: no geometric gradient, no backward preprocess.
 *   geom / binning / image buffers: as the forward left them (R = its num_rendered, or the capacity of the async forward); they are
 *     only read -- the gradient accumulation rows inside geom_buffer are not touched, so a gsr_rasterize_backward* call on the same
 *     buffers before or after it is unaffected, with or without GSR_BWD_ROWS_ZEROED;
 *   dL_dpix [3][H][W] or null; dL_dcolor [P][3], required when dL_dpix is given (null otherwise allowed);
 *   n_extra = 0 or 18; dL_dout_extra = HOST array of six device pointers as in gsr_rasterize_backward_ex (a null entry = no
 *     gradient on that image: no work, its three columns come back exactly zero); dL_dextra [P][18]; both required when n_extra = 18.
 * Every element of the outputs given is written: the call zero-fills them and accumulates with float atomics (sums agree with
 * gsr_rasterize_backward_ex to summation order); rows of culled Gaussians stay zero.  "deterministic" = 1 returns GSR_EINVAL, as the
 * fused 18-channel backward does.  debug bit 0 as elsewhere.  Results do not depend on the binning back-end or on "tile_order" /
 * "blend_segments" / "tile_cull" (long lists are walked whole, like the forward's). */
int gsr_rasterize_backward_colors(int P, int R, int width, int height, char *geom_buffer, char *binning_buffer, char *image_buffer,
                                  const float *dL_dpix, float *dL_dcolor, int n_extra, const float *const *dL_dout_extra,
                                  float *dL_dextra, int debug, gsr_stream_t stream);

/* The training loss render() feeds before the PBR phase (train.py:261-265 with utils/loss_utils.py:20-24), fused:
 *     L = w_image L1_b(image, gt_image) + w_alpha L2_b(alpha, alpha_target) + w_normal L1_b(normal, gt_normal) + w_axis L1_b(axis, gt_normal)
 * where L1_b / L2_b are the MEANS over the pixels with bound != 0 (the reference indexes with bound_mask == 1; a mean over n_bound x 3
 * colour values resp. n_bound alphas).  gsr_phase1_loss_forward reduces the forward's images to the loss value and leaves
 * (loss, n_bound, 1 / (3 n_bound), 1 / n_bound, the four unweighted terms) in stats[8] on the device -- no host read.
 * gsr_rasterize_backward_phase1_loss is gsr_rasterize_backward_ex whose blend-backward prologue FORMS this loss's per-pixel
 * gradient from the same images (bound . w sign(image - gt) / (3 n_bound) etc., times *upstream, the incoming dL/dL: null = 1)
 * instead of reading it: dL_dpix / dL_ddepths / dL_dalphas and the entries of dL_dout_extra may each be null there (no further
 * gradient on that image) or carry the gradient of OTHER loss terms (SSIM, LPIPS, ...), which is added.  What it saves per frame
 * against the same loss in torch ops: four masked reductions, their expand / divide / sign backward kernels and four full-image
 * gradient tensors written and read (~125 us of a 790 us render() frame at 1024^2, profiles/r3h_render_kernels.txt). */
typedef struct gsr_phase1_loss {
  const float *gt_image;      /* [3][H][W] */
  const float *gt_normal;     /* [3][H][W]: the target of BOTH the normal and the axis image (train.py:263-264) */
  const float *alpha_target;  /* [H][W]    (bkgd_mask[0]) */
  const float *bound;         /* [H][W]    != 0 inside bound_mask */
  float w_image, w_alpha, w_normal, w_axis;
  int normal_triple, axis_triple; /* which of the six extra colour triples are the normal / the axis image (render(): 0 and 5) */
  const float *color;         /* the forward's images: [3][H][W] */
  const float *alpha;         /* [H][W] */
  const float *extra_images;  /* [18][H][W] */
  float *stats;               /* device [8], written by gsr_phase1_loss_forward, read by the backward */
  const float *upstream;      /* device [1]: dL/dloss arriving from autograd (null = 1) */
} gsr_phase1_loss;
/* partials: device workspace of at least gsr_phase1_loss_partials() floats */
size_t gsr_phase1_loss_partials(void);
int gsr_phase1_loss_forward(int width, int height, const gsr_phase1_loss *loss, float *partials, gsr_stream_t stream);
int gsr_rasterize_backward_phase1_loss(int P, int D, int M, int R, const float *background, int width, int height, const float *means3D,
                                       const float *shs, const float *colors_precomp, const float *alphas, const float *scales,
                                       float scale_modifier, const float *rotations, const float *cov3D_precomp,
                                       const float *viewmatrix, const float *projmatrix, const float *campos, float tan_fovx,
                                       float tan_fovy, const int *radii, char *geom_buffer, char *binning_buffer,
                                       char *image_buffer, const float *dL_dpix, const float *dL_ddepths, const float *dL_dalphas,
                                       float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolor,
                                       float *dL_dmean3D, float *dL_dcov3D, float *dL_dsh, float *dL_dscale, float *dL_drot,
                                       int debug, const float *extra_features, int n_extra, const float *const *dL_dout_extra,
                                       float *dL_dextra, int sh_dtype, const gsr_phase1_loss *loss, gsr_stream_t stream);

/* Fused gradient of L = mean|color - gt| + lambda_alpha * mean (alpha - mask)^2 (train.py:261-262 with the masks set to
 * the whole image): dL_dcolor[3][H][W] = sign(color - gt) / (3 H W), dL_dalpha[H][W] = 2 lambda (alpha - mask) / (H W). */
int gsr_alpha_mask_loss_backward(int width, int height, const float *color, const float *alpha, const float *gt,
                                 const float *mask, float lambda_alpha, float *dL_dcolor, float *dL_dalpha,
                                 gsr_stream_t stream);

/* gsr_rasterize_backward_ex with the image gradients of THAT loss formed inside the blend-backward kernel (per pixel, the same
 * expressions) instead of read from three gradient images: out_color / out_alpha are the forward's images, gt [3][H][W],
 * mask [1][H][W]; dL_ddepth = 0.  One launch and 48 B per pixel of traffic less than gsr_alpha_mask_loss_backward +
 * gsr_rasterize_backward_ex; gradients bit-identical to that pair.  (No extra feature channels in this entry.) */
int gsr_rasterize_backward_alpha_mask_loss(int P, int D, int M, int R, const float *background, int width, int height,
                                           const float *means3D, const float *shs, const float *colors_precomp,
                                           const float *out_alpha, const float *scales, float scale_modifier,
                                           const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                                           const float *projmatrix, const float *campos, float tan_fovx, float tan_fovy,
                                           const int *radii, char *geom_buffer, char *binning_buffer, char *image_buffer,
                                           const float *out_color, const float *gt, const float *mask, float lambda_alpha,
                                           float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolor,
                                           float *dL_dmean3D, float *dL_dcov3D, float *dL_dsh, float *dL_dscale, float *dL_drot,
                                           int debug, int sh_dtype, gsr_stream_t stream);

/* Introspection of the private scratch buffers, for the parity tests only (copies device -> device):
 * what = one of GSR_Q_*; dst must hold the documented element count. */
#define GSR_Q_DEPTHS 0        /* float[P]            geom  */
#define GSR_Q_MEANS2D 1       /* float[P][2]         geom  */
#define GSR_Q_CONIC_OPACITY 2 /* float[P][4]         geom  */
#define GSR_Q_RGB 3           /* float[P][3]         geom  */
#define GSR_Q_COV3D 4         /* float[P][6]         geom  (only valid if computed from scales/rotations) */
#define GSR_Q_TILES_TOUCHED 5 /* uint32[P]           geom  */
#define GSR_Q_POINT_OFFSETS 6 /* uint32[P]           geom  (inclusive scan) */
#define GSR_Q_CLAMPED 7       /* uint8[P][3]         geom  */
#define GSR_Q_POINT_LIST 8    /* uint32[R]           binning (sorted Gaussian ids) */
#define GSR_Q_KEYS_SORTED 9   /* uint64[R]           binning (tile << 32 | depth bits) */
#define GSR_Q_RANGES 10       /* uint32[tiles][2]    image */
#define GSR_Q_FINAL_T 11      /* float[H][W]         image */
#define GSR_Q_N_CONTRIB 12    /* uint32[H][W]        image */
#define GSR_Q_ORDER 13        /* uint32[4 tiles + 66] image: [0] visiting mode | longest list << 8, [1] slots in use (mode 1),
                               * [2 ..] one entry per visiting slot: tile | segment << 22 | (segments - 1) << 25 */
int gsr_query_state(int what, int P, int R, int width, int height, const char *geom_buffer,
                    const char *binning_buffer, const char *image_buffer, void *dst, gsr_stream_t stream);

/* simple-knn: mean_dists[i] = mean of the 3 smallest squared distances from points[i] to the other points
 * (SK/simple_knn.cu:185-221).  workspace must hold gsr_dist2_workspace_bytes(P) bytes. */
size_t gsr_dist2_workspace_bytes(int P);
int gsr_dist2(int P, const float *points, float *mean_dists, char *workspace, size_t workspace_bytes,
              gsr_stream_t stream);

/* Stand-alone stable LSD radix sort of (key, value) pairs on key bits [0, end_bit), the replacement of
 * cub::DeviceRadixSort::SortPairs at CR/rasterizer_impl.cu:305-310 (u64 keys) and SK/simple_knn.cu:213 (u32 keys).
 * workspace: gsr_sort_workspace_bytes(n). Results land in keys_out / vals_out; inputs are preserved. */
size_t gsr_sort_workspace_bytes(size_t n);
int gsr_sort_pairs_u64(size_t n, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *vals_in,
                       uint32_t *vals_out, int end_bit, char *workspace, size_t workspace_bytes,
                       gsr_stream_t stream);
int gsr_sort_pairs_u32(size_t n, const uint32_t *keys_in, uint32_t *keys_out, const uint32_t *vals_in,
                       uint32_t *vals_out, int end_bit, char *workspace, size_t workspace_bytes,
                       gsr_stream_t stream);

/* SMPL linear-blend skinning of P canonical points (the per-point part of coarse_deform_c2source,
 * scene/gaussian_model.py:776-872, batch size 1).
 *   query[P][3], normals[P][3] (may be null); smpl_verts[V][3] = big-pose vertices searched for the nearest
 *   vertex (k = 1, lowest index wins ties); weights[V][24]; lbs_offsets[P][24] or null
 *   (softmax(log(w + 1e-9) + offset)); A_big / A_pose [24][16] joint transforms; off_big / off_shape / off_pose
 *   [V][3] per-vertex offset tables (PoseOff(theta_big), ShapeOff(beta), PoseOff(theta, dR)); R[9], Th[3].
 * Outputs (any may be null except world_pts): vert_ids int32[P], bweights[P][24], smpl_pts[P][3],
 *   world_pts[P][3], transforms[P][9], translation[P][3], world_normals[P][3]. */
int gsr_lbs_forward(int P, int V, const float *query, const float *normals, const float *smpl_verts,
                    const float *weights, const float *lbs_offsets, const float *A_big, const float *A_pose,
                    const float *off_big, const float *off_shape, const float *off_pose, const float *R,
                    const float *Th, int *vert_ids, float *bweights, float *smpl_pts, float *world_pts,
                    float *transforms, float *translation, float *world_normals, gsr_stream_t stream);

/* Same results as gsr_lbs_forward, bit for bit, with the nearest-vertex search run through a uniform grid over the V
 * reference vertices (rebuilt on every call by one workgroup) instead of the brute-force scan: ~30x fewer distance
 * evaluations when the query points lie near the vertex cloud, as canonical Gaussians do.  `workspace` must hold
 * gsr_lbs_workspace_bytes(V) bytes, 16-byte aligned.  grid_is_built != 0: the workspace already holds the grid of exactly
 * these vertices (gsr_lbs_grid_build, or an earlier call) and the rebuild is skipped -- the big-pose vertices of a subject
 * never change between frames.  A query point with no finite distance to any vertex (NaN, infinite, or a squared distance
 * that overflows) takes vertex 0, as in the brute-force scan. */
size_t gsr_lbs_workspace_bytes(int V);
int gsr_lbs_grid_build(int V, const float *smpl_verts, char *workspace, size_t workspace_bytes, gsr_stream_t stream);
int gsr_lbs_forward_grid(int P, int V, const float *query, const float *normals, const float *smpl_verts,
                         const float *weights, const float *lbs_offsets, const float *A_big, const float *A_pose,
                         const float *off_big, const float *off_shape, const float *off_pose, const float *R,
                         const float *Th, int *vert_ids, float *bweights, float *smpl_pts, float *world_pts,
                         float *transforms, float *translation, float *world_normals, char *workspace,
                         size_t workspace_bytes, int grid_is_built, gsr_stream_t stream);

/* gsr_lbs_forward_grid with an EXACT temporal cache of the nearest vertex (the reference searches every
 * frame, scene/gaussian_model.py:775).  The canonical points move by an optimizer step per iteration, the vertices not at all.
 * nn_cache (gsr_lbs_nn_cache_bytes(P) bytes, 16-byte aligned, caller-owned, tied to ONE vertex grid) holds per point slot
 * (x0, id, rho): vertex id is the strict nearest vertex of every point within rho of x0 -- rho = 0.49 x (lower bound on the
 * distance of every other vertex - distance of id), minus a guard for rounding -- which is a statement about the vertex set, so
 * it stays true whatever point sits in the slot.  cache_is_valid = 0: full grid search that also makes the entries.
 * cache_is_valid != 0: one kernel checks every point against its entry and searches (and re-centres) the misses, the
 * skinning takes the ids as given: results bit-identical to the search.  `workspace` must hold the BUILT grid
 * (gsr_lbs_grid_build).  The last 64 bytes of nn_cache are counters: word 1 = searches since the cache was made, word 2 = misses
 * of the last cached call.  A point with no finite distance to any vertex takes vertex 0.  A NaN or infinite point misses and is
 * searched again every frame; a finite point whose squared distances overflow gets the unbounded radius of a single-vertex cloud
 * (no other vertex was seen at a finite distance), keeps vertex 0 while its squared displacement stays finite and is searched
 * again once that overflows: the result equals the search's either way. */
size_t gsr_lbs_nn_cache_bytes(int P);
int gsr_lbs_forward_cached(int P, int V, const float *query, const float *normals, const float *smpl_verts,
                           const float *weights, const float *lbs_offsets, const float *A_big, const float *A_pose,
                           const float *off_big, const float *off_shape, const float *off_pose, const float *R,
                           const float *Th, int *vert_ids, float *bweights, float *smpl_pts, float *world_pts,
                           float *transforms, float *translation, float *world_normals, char *workspace,
                           size_t workspace_bytes, char *nn_cache, size_t nn_cache_bytes, int cache_is_valid,
                           gsr_stream_t stream);

/* Backward of gsr_lbs_forward w.r.t. query, normals, lbs_offsets, A_pose, off_pose (A_big/off_big/off_shape
 * belong to the constant big pose / shape and get no gradient in the reference training loop).
 * Incoming: dL_dworld_pts[P][3], dL_dtransforms[P][9], dL_dworld_normals[P][3] (each may be null = zero).
 * Outgoing (zero-filled by the caller, accumulated into): dL_dquery[P][3], dL_dnormals[P][3] (or null),
 *   dL_dlbs_offsets[P][24] (or null), dL_dA_pose[24][16] (or null), dL_doff_pose[V][3] (or null).
 * dA_pose_partials (optional): [gsr_lbs_backward_workgroups(P)][24 * 12] floats.  When given (and dL_dA_pose is non-null)
 *   every workgroup stores its own sum there instead of issuing 288 atomics onto dL_dA_pose; the caller adds the rows up
 *   (entry j * 12 + k belongs to dL_dA_pose[j][k / 4][k % 4]) -- dL_dA_pose itself is then left untouched. */
int gsr_lbs_backward_workgroups(int P);
int gsr_lbs_backward(int P, int V, const float *query, const float *normals, const int *vert_ids,
                     const float *weights, const float *lbs_offsets, const float *A_big, const float *A_pose,
                     const float *off_big, const float *off_shape, const float *off_pose, const float *R,
                     const float *dL_dworld_pts, const float *dL_dtransforms, const float *dL_dworld_normals,
                     float *dL_dquery, float *dL_dnormals, float *dL_dlbs_offsets, float *dL_dA_pose,
                     float *dL_doff_pose, float *dA_pose_partials, gsr_stream_t stream);

/* Joint-count variants of the four LBS entry points above: the same signatures with a leading J, and [24] becomes [J] in every
 * shape -- weights[V][J], lbs_offsets[P][J], A_big / A_pose [J][16], bweights[P][J], dL_dlbs_offsets[P][J], dL_dA_pose[J][16],
 * dA_pose_partials [gsr_lbs_backward_workgroups(P)][J * 12].  Compiled for J = 24 (SMPL; bit-identical to the entry points
 * without _nj) and J = 55 (SMPL-X); any other J returns GSR_EINVAL before anything runs on the device. */
int gsr_lbs_forward_nj(int J, int P, int V, const float *query, const float *normals, const float *smpl_verts,
                       const float *weights, const float *lbs_offsets, const float *A_big, const float *A_pose,
                       const float *off_big, const float *off_shape, const float *off_pose, const float *R,
                       const float *Th, int *vert_ids, float *bweights, float *smpl_pts, float *world_pts,
                       float *transforms, float *translation, float *world_normals, gsr_stream_t stream);
int gsr_lbs_forward_grid_nj(int J, int P, int V, const float *query, const float *normals, const float *smpl_verts,
                            const float *weights, const float *lbs_offsets, const float *A_big, const float *A_pose,
                            const float *off_big, const float *off_shape, const float *off_pose, const float *R,
                            const float *Th, int *vert_ids, float *bweights, float *smpl_pts, float *world_pts,
                            float *transforms, float *translation, float *world_normals, char *workspace,
                            size_t workspace_bytes, int grid_is_built, gsr_stream_t stream);
int gsr_lbs_forward_cached_nj(int J, int P, int V, const float *query, const float *normals, const float *smpl_verts,
                              const float *weights, const float *lbs_offsets, const float *A_big, const float *A_pose,
                              const float *off_big, const float *off_shape, const float *off_pose, const float *R,
                              const float *Th, int *vert_ids, float *bweights, float *smpl_pts, float *world_pts,
                              float *transforms, float *translation, float *world_normals, char *workspace,
                              size_t workspace_bytes, char *nn_cache, size_t nn_cache_bytes, int cache_is_valid,
                              gsr_stream_t stream);
int gsr_lbs_backward_nj(int J, int P, int V, const float *query, const float *normals, const int *vert_ids,
                        const float *weights, const float *lbs_offsets, const float *A_big, const float *A_pose,
                        const float *off_big, const float *off_shape, const float *off_pose, const float *R,
                        const float *dL_dworld_pts, const float *dL_dtransforms, const float *dL_dworld_normals,
                        float *dL_dquery, float *dL_dnormals, float *dL_dlbs_offsets, float *dL_dA_pose,
                        float *dL_doff_pose, float *dA_pose_partials, gsr_stream_t stream);

/* Fused SSIM (extension): utils/loss_utils.py:25-66 -- 11x11 Gaussian window (sigma 1.5), zero
 * padding, C1 = 0.01^2, C2 = 0.03^2 -- over `planes` independent H x W planes (batch x channels of the reference's grouped
 * conv2d).  forward: ssim_map[planes][H][W] (may be null) and the three derivative maps dA, dB, dC (all three or none) that
 * the backward consumes.  backward: dL_dimg1 from dL_dmap[planes][H][W], or from the constant dL_dmap_scalar when dL_dmap is
 * null (the mean reduction of the reference: scalar = upstream / (planes * H * W)).  img2 is the ground truth: no gradient.
 * dL_dmap weights the map, so it is applied under the window (at the pixel whose map value it scales), not at the output pixel.
 * The eleven window weights are the reference's float32 values bit for bit: the unnormalised float32 values divided by their sum
 * rounded ONCE to float32 (what torch's sum returns; a running float32 sum is one ulp lower and scales every weight by 1 + 6e-8).
 * The same weights serve gsr_ssim_crop_* and the SSIM of gsr_eval_view_finish.  All three round once per operation (built
 * without FMA contraction), like the reference's elementwise kernels: img1 == img2 gives a map of exactly 1, and the A / B / C
 * planes of gsr_ssim_crop_forward under the full-frame rectangle are gsr_ssim_forward's bit for bit. */
int gsr_ssim_forward(int planes, int height, int width, const float *img1, const float *img2, float *ssim_map, float *dA,
                     float *dB, float *dC, gsr_stream_t stream);
int gsr_ssim_backward(int planes, int height, int width, const float *img1, const float *img2, const float *dL_dmap,
                      float dL_dmap_scalar, const float *dA, const float *dB, const float *dC, float *dL_dimg1,
                      gsr_stream_t stream);

/* Fused row gather over a structure of arrays (extension): the data movement of the reference's
 * prune_points / cat_tensors_to_optimizer / densification_postfix (scene/gaussian_model.py:421-512) for ALL parameter
 * tensors, both Adam moments of each and the statistics in one launch.  For every array a < n_arrays (<= 32; src / dst /
 * row_floats / zero_new are HOST arrays, the pointers in them device pointers):
 *   dst[a][j][:] = src[a][index[j] & 0x3FFFFFFF][:]          for j < n_out, rows of row_floats[a] floats,
 *   dst[a][j][:] = 0   if index[j] < 0, or if bit 30 of index[j] is set ("new Gaussian") and zero_new[a] != 0
 * (the Adam moments of cloned / split Gaussians start at zero, their parameters are copies of the parent's row).
 * index is a device array; dst must not alias src. */
int gsr_gather_rows(int n_arrays, const float *const *src, float *const *dst, const int *row_floats, const int *zero_new,
                    int n_out, const int *index, gsr_stream_t stream);

/* The decisions and the new rows of a densification step on the device (extension; csrc/densify.hip): what surrounds
 * gsr_gather_rows in densify_and_clone / densify_and_split / kl_densify_and_clone / kl_densify_and_split / kl_merge /
 * prune_points (scene/gaussian_model.py:443-461,514-708,740-762) without a host read.  All arrays are device arrays unless
 * stated otherwise; none may alias an output.
 *
 *   gsr_kl_pairs: kl[i] = KL( N(mu_a, S_a) || N(mu_b, S_b) ), (a, b) = pairs[i], S = R diag(s^2) R^T with R of the normalised
 *     quaternion rotation[.] (w, x, y, z) and s = exp(log_scaling[.]) -- kl_div (:740-762) evaluated in the frame of b, where
 *     every summand of the trace and of the Mahalanobis term is non-negative and the log-determinant is 2 sum(l_b - l_a).
 *     A pair index outside [0, P) gives NaN and reads nothing.
 *   gsr_densify_select: flags[i] = 1 where Gaussian i is selected, else 0.  `scaling` is the ACTIVATED scaling [P][3], grads
 *     [n_grads] (n_grads <= P; rows beyond it count as 0):
 *       GSR_DENSIFY_CLONE  |grads[i]| >= grad_threshold and max(scaling[i]) <= size_threshold   [and kl[i] > kl_threshold]
 *       GSR_DENSIFY_SPLIT   grads[i]  >= grad_threshold and max(scaling[i]) >  size_threshold   [and kl[i] > kl_threshold]
 *       GSR_DENSIFY_MERGE   grads[i]  >= grad_threshold and max(scaling[i]) <= size_threshold   [and kl[i] < kl_threshold]
 *     (the KL term only with kl != null).  A NaN on either side of a comparison makes it false.
 *   gsr_densify_plan: the row plan (the `index` of gsr_gather_rows, bit 30 = new row) of an operation from its flags, by a
 *     stable compaction; header = (n_keep, n_new, n_out, 0), n_out = n_keep + n_new plan entries are written:
 *       GSR_PLAN_PRUNE  the rows with flag 0, in order                                              plan capacity P
 *       GSR_PLAN_CLONE  all P rows, then the flagged rows (new)                                                   2 P
 *       GSR_PLAN_SPLIT  the rows with flag 0, then N times the flagged rows in order (new)                  (N + 1) P
 *       GSR_PLAN_MERGE  the rows that are neither flagged nor pairs[i][1] of a flagged i, then pairs[i][0]        2 P
 *                       (new) for every flagged i in order; plan[P + c] = pairs[i][1] of the c-th of them (n_out <= P)
 *     The same input gives the same plan on every call (positions come from prefix sums).  (N + 1) P < 2^30.  Workspace:
 *     gsr_densify_plan_workspace_bytes(P), 4-byte aligned.
 *   gsr_build_rows: gsr_gather_rows (same host tables; n_src = rows of the source arrays, an index beyond it gives NaN)
 *     that also computes the new rows, i.e. the output rows j >= first, of the arrays whose role[] (host array) is not
 *     GSR_ROW_COPY; s = index[j] & 0x3FFFFFFF, c = j - first, `scaling` = the activated scaling [n_src][3]:
 *       GSR_BUILD_MOVE      nothing is computed (role, first, scaling, unit, partner are ignored)
 *       GSR_BUILD_CHILDREN  GSR_ROW_XYZ: R(rotation[s]) (scaling[s] * unit[c]) + xyz[s];  GSR_ROW_LOG_SCALING: log(scaling[s]
 *                           / divisor).  xyz / rotation are the source arrays with role GSR_ROW_XYZ / GSR_ROW_ROTATION and
 *                           zero_new = 0 (the parameters, not their moments); unit [n_out - first][3].
 *       GSR_BUILD_MERGE     GSR_ROW_XYZ and GSR_ROW_MEAN: 0.5 (src[s] + src[partner[c]]);  GSR_ROW_LOG_SCALING: log(scaling[s]
 *                           / 0.8); partner [n_out - first] (a row outside [0, n_src) gives NaN).
 *     Rows below `first`, arrays with role GSR_ROW_COPY / GSR_ROW_ROTATION and zeroed rows are as in gsr_gather_rows. */
enum { GSR_DENSIFY_CLONE = 0, GSR_DENSIFY_SPLIT = 1, GSR_DENSIFY_MERGE = 2 };
enum { GSR_PLAN_PRUNE = 0, GSR_PLAN_CLONE = 1, GSR_PLAN_SPLIT = 2, GSR_PLAN_MERGE = 3 };
enum { GSR_BUILD_MOVE = 0, GSR_BUILD_CHILDREN = 1, GSR_BUILD_MERGE = 2 };
enum { GSR_ROW_COPY = 0, GSR_ROW_XYZ = 1, GSR_ROW_LOG_SCALING = 2, GSR_ROW_ROTATION = 3, GSR_ROW_MEAN = 4 };
int gsr_kl_pairs(int P, const float *xyz, const float *rotation, const float *log_scaling, const int *pairs, float *kl,
                 gsr_stream_t stream);
int gsr_densify_select(int P, int mode, const float *grads, int n_grads, const float *scaling, const float *kl,
                       float grad_threshold, float size_threshold, float kl_threshold, unsigned char *flags,
                       gsr_stream_t stream);
size_t gsr_densify_plan_workspace_bytes(int P);
int gsr_densify_plan(int P, int kind, int N, const unsigned char *flags, const int *pairs, int *plan, int *header,
                     char *workspace, size_t workspace_bytes, gsr_stream_t stream);
int gsr_build_rows(int n_arrays, const float *const *src, float *const *dst, const int *row_floats, const int *zero_new,
                   const int *role, int n_out, const int *index, int n_src, int first, int mode, const float *scaling,
                   const float *unit, float divisor, const int *partner, gsr_stream_t stream);

/* k-NN service replacing the un-vendored KNN_CUDA dependency (scene/gaussian_model.py:87-89).
 * Semantics assumed for KNN_CUDA 0.2 (parity unpinned): exact brute-force k-NN, Euclidean distances in ascending order;
 * here ties resolve to the lowest index.
 *   gsr_knn_self: the k <= 3 nearest of every point among the SAME P points, the point itself included (what
 *     knn(xyz, xyz) returns; :176,573,621,671): idx[P][k] int32, dist[P][k].  Workspace: gsr_dist2_workspace_bytes(P).
 *   gsr_knn_nearest: nearest of N reference points for each of M queries (:727, distance of the Gaussians to the SMPL
 *     vertices; :775 is fused into gsr_lbs_forward_grid): idx[M] and/or dist[M] (either may be null).
 *     Workspace: gsr_lbs_workspace_bytes(N), 16-byte aligned.  A query with no finite distance to any reference point
 *     (NaN, infinite, overflowing square) gets index 0 and dist = sqrt(FLT_MAX). */
int gsr_knn_self(int P, const float *points, int k, int *idx, float *dist, char *workspace, size_t workspace_bytes,
                 gsr_stream_t stream);
int gsr_knn_nearest(int M, const float *query, int N, const float *ref, int *idx, float *dist, char *workspace,
                    size_t workspace_bytes, gsr_stream_t stream);

/* Compact exchange of the SH-coefficient gradient between view-parallel ranks (extension).  For one view
 * dL_dsh[i][k][c] = w_k(dir_i) * dL_dRGB[i][c] (dir = normalise(mean - campos); dL_dRGB zeroed on clamped channels,
 * CR/backward.cu:40-116): ranks all-gather 12 B per Gaussian instead of all-reducing 12 M B.
 *   gsr_sh_view_pack: packed[P][3] = dL_dcolor (the backward's dL_dcolor output of an SH-mode call) with the channels the
 *     forward clamped set to zero; geom_buffer is that call's geometry buffer.
 *   gsr_sh_grad_from_views: dL_dsh[P][M][3] = scale * sum_v w_k(normalise(means3D - campos_v)) * packed_v, v in fixed
 *     order; `views` holds n_views blocks of view_stride floats: [P*3 packed | campos xyz | padding].  dev_scale (device
 *     pointer to one float, or null) multiplies `scale`: the view-parallel step passes 0 there for a step some rank could not
 *     render (binning overflow), so that every replica skips it, without a host read.  A view whose three packed values for a
 *     Gaussian are all zero (culled or invisible there) contributes nothing to that Gaussian, whatever its direction would be:
 *     a position equal to the view's camera, or a non-finite one, does not reach the sum -- as in the all-reduced path. */
int gsr_sh_view_pack(int P, const char *geom_buffer, const float *dL_dcolor, float *packed, gsr_stream_t stream);
int gsr_sh_grad_from_views(int P, int sh_degree, int M, int n_views, const float *means3D, const float *views,
                           size_t view_stride, float scale, const float *dev_scale, float *dL_dsh, gsr_stream_t stream);

/* The same exchange for ARTICULATED Gaussians (render(): colours come from the per-frame attribute kernel, and every view poses
 * the Gaussians differently, so the positions travel with the view).  A view block is [P*3 masked dL_dRGB | ... ] with the
 * posed positions at means_offset (>= 3 P, floats) and the camera position at cam_offset (>= means_offset + 3 P):
 *   gsr_sh_view_pack_posed: fills the three parts of this rank's block in one launch; `colors` = the forward's colours
 *     max(SH + 0.5, 0) (a channel that came out 0 was clamped: its gradient is dropped, gaussian_renderer/__init__.py:195),
 *     dL_dcolors = the rasterizer's gradient with respect to them, means3D_view = the view's posed positions, campos device [3].
 *   gsr_sh_grad_from_views_posed: the mean SH gradient written in the model's two parameter layouts, dL_dsh_dc [P][1][3] and
 *     dL_dsh_rest [P][15][3] (16-byte aligned); scale / dev_scale as above, and so is the rule for an all-zero packed triple: the
 *     view contributes nothing to that Gaussian, whatever position rides in its block. */
int gsr_sh_view_pack_posed(int P, const float *colors, const float *dL_dcolors, const float *means3D_view, const float *campos,
                           float *view_block, size_t means_offset, size_t cam_offset, gsr_stream_t stream);
int gsr_sh_grad_from_views_posed(int P, int sh_degree, int n_views, const float *views, size_t view_stride, size_t means_offset,
                                 size_t cam_offset, float scale, const float *dev_scale, float *dL_dsh_dc, float *dL_dsh_rest,
                                 gsr_stream_t stream);

/* Bookkeeping of one view-parallel step around its gradient all-reduce, one single-thread launch, no host read
 * (extension).  status = dev_status of the step's gsr_rasterize_forward_async (R, overflow flag); overflow_slot = one float
 * inside the all-reduced gradient bucket.
 *   phase 0 (before the reduction): overflow_slot[0] = overflow flag as 0/1
 *   phase 1 (after the SUM reduction): scale[0] = overflow_slot[0] > 0 ? 0 : inv_world  (a step some rank could not render
 *            is skipped by every replica); report[0..2] = {ranks that overflowed, R, own flag} -- `report` may be pinned,
 *            device-mapped host memory, examined by the host after an event
 *   phase 2: both (single process). */
int gsr_step_status(int phase, const uint32_t *status, float *overflow_slot, float inv_world, float *scale, uint32_t *report,
                    gsr_stream_t stream);
/* gsr_step_status phase 1 AND the division of the reduced bucket in ONE launch: bucket[0 .. n_floats) is the flat fp32 buffer
 * that was SUM all-reduced (16-byte aligned), bucket[overflow_index] the number of ranks whose binning overflowed; every other
 * element is multiplied by scale = (that count > 0 ? 0 : inv_world); scale[0] (optional) and report[0..2] (optional; status may
 * be null: words 1, 2 are then 0) as in phase 1. */
int gsr_step_finish(const uint32_t *status, float *bucket, size_t n_floats, size_t overflow_index, float inv_world, float *scale,
                    uint32_t *report, gsr_stream_t stream);

/* SMPL pose -> joint transforms (batch size 1): rodrigues of the 24 axis-angle vectors (angle = |theta + 1e-8|), the
 * optional pose-refinement product R_j <- R_j correct_Rs[j-1] (j >= 1), the kinematic chain and the removal of the rest
 * pose -- scene/gaussian_model.py:894-980 (batch_rodrigues_torch, get_rigid_transformation_torch,
 * get_transform_params_torch) and :822-825 -- in one single-wave launch.
 *   poses[72], correct_Rs[23][9] or null, joints[24][3] (device); parents_host[24]: HOST array, parents[i] < i, entry 0
 *   ignored.  Outputs (device): rot_mats[24][9] (may be null), A[24][16] row-major 4x4. */
int gsr_smpl_pose_forward(const float *poses, const float *correct_Rs, const float *joints, const int *parents_host,
                          float *rot_mats, float *A, gsr_stream_t stream);

/* Adjoint of gsr_smpl_pose_forward: dL_dA[24][16] (row 3 ignored), dL_drot_mats[24][9] or null (the pose blend shapes'
 * use of rot_mats) -> dL_dposes[72], dL_dcorrect_Rs[23][9] (null if correct_Rs is null), dL_djoints[24][3]; each output
 * may be null and is fully written otherwise. */
int gsr_smpl_pose_backward(const float *poses, const float *correct_Rs, const float *joints, const int *parents_host,
                           const float *dL_dA, const float *dL_drot_mats, float *dL_dposes, float *dL_dcorrect_Rs,
                           float *dL_djoints, gsr_stream_t stream);

/* The same chain for any body model with 2 <= J <= 64 joints (one lane per joint): poses[3J], correct_Rs[J-1][9] or null,
 * joints[J][3], parents_host[J]; rot_mats[J][9], A[J][16]; dL_dA[J][16], dL_drot_mats[J][9] -> dL_dposes[3J],
 * dL_dcorrect_Rs[J-1][9], dL_djoints[J][3].  J = 24 is gsr_smpl_pose_forward / _backward bit for bit; SMPL-X is J = 55.
 * Any other J returns GSR_EINVAL before anything runs on the device. */
int gsr_body_pose_forward(int J, const float *poses, const float *correct_Rs, const float *joints, const int *parents_host,
                          float *rot_mats, float *A, gsr_stream_t stream);
int gsr_body_pose_backward(int J, const float *poses, const float *correct_Rs, const float *joints, const int *parents_host,
                           const float *dL_dA, const float *dL_drot_mats, float *dL_dposes, float *dL_dcorrect_Rs,
                           float *dL_djoints, gsr_stream_t stream);

/* Row-major matrix-vector products for the SMPL pose blend shapes (scene/gaussian_model.py:805-811,827-839):
 *   gsr_gemv_rows:   out[r] = sum_k mat[r][k] * vec[k]          (offsets[V*3] = posedirs[V*3][207] . pose_feature[207])
 *   gsr_gemv_rows_t: dvec[k] = sum_r dout[r] * mat[r][k]        (its backward w.r.t. the pose feature; dvec is overwritten)
 * cols <= 512 (SMPL-X: posedirs[10475*3][486]); up to 256 columns run the 4-columns-per-lane kernel, above it 8 per lane. */
int gsr_gemv_rows(int rows, int cols, const float *mat, const float *vec, float *out, gsr_stream_t stream);
int gsr_gemv_rows_t(int rows, int cols, const float *mat, const float *dout, float *dvec, gsr_stream_t stream);

/* The parameter activations render() applies every frame (the reference's property getters, scene/gaussian_model.py:157-199,
 * and the occlusion placeholder of gaussian_renderer/__init__.py:141), P rows each, one kernel:
 *   opacity[1] = sigmoid(opacity_raw)   albedo[3] = sigmoid(albedo_raw)   scaling[3] = exp(scaling_raw)
 *   rotation[4] = rotation_raw / max(|rotation_raw|, 1e-12)   normal[3] = normal_raw / |normal_raw|   occlusion[3] = opacity x3
 * (get_roughness reads _albedo as well in the reference, :197-199: callers alias the albedo output for it). */
int gsr_model_activations_forward(int P, const float *opacity_raw, const float *albedo_raw, const float *scaling_raw,
                                  const float *rotation_raw, const float *normal_raw, float *opacity, float *albedo,
                                  float *scaling, float *rotation, float *normal, float *occlusion, gsr_stream_t stream);

/* Backward of gsr_model_activations_forward: opacity / albedo / scaling are the forward's outputs, g_* the gradients of the six
 * outputs (a null g_* = that output did not reach the loss), d_*_raw are fully written. */
int gsr_model_activations_backward(int P, const float *rotation_raw, const float *normal_raw, const float *opacity,
                                   const float *albedo, const float *scaling, const float *g_opacity, const float *g_albedo,
                                   const float *g_scaling, const float *g_rotation, const float *g_normal,
                                   const float *g_occlusion, float *d_opacity_raw, float *d_albedo_raw, float *d_scaling_raw,
                                   float *d_rotation_raw, float *d_normal_raw, gsr_stream_t stream);
/* The same with acc_drotation_raw [P][4] (or null) ADDED to d_rotation_raw: a gradient of the raw quaternion that already exists
 * (render() hands the raw quaternion to the covariance as well, gaussian_renderer/__init__.py:128-131 / scene/gaussian_model.py:35-42:
 * the leaf would otherwise receive two gradients and autograd an add kernel per frame). */
int gsr_model_activations_backward_acc(int P, const float *rotation_raw, const float *normal_raw, const float *opacity,
                                       const float *albedo, const float *scaling, const float *g_opacity, const float *g_albedo,
                                       const float *g_scaling, const float *g_rotation, const float *g_normal,
                                       const float *g_occlusion, float *d_opacity_raw, float *d_albedo_raw, float *d_scaling_raw,
                                       float *d_rotation_raw, float *d_normal_raw, const float *acc_drotation_raw,
                                       gsr_stream_t stream);

/* Per-frame, per-Gaussian attributes render() derives between the LBS deform and the rasterizer
 * (gaussian_renderer/__init__.py:128-198; scene/gaussian_model.py:35-42,186-190; utils/general_utils.py:64-157;
 * utils/sh_utils.py:57-117; transform.py:9-17) -- one kernel instead of the reference's torch op chain.
 * Inputs, P rows each: means3D[3] (world), transforms[9] (row-major LBS rotation), world_normals[3] (LBS-rotated canonical
 *   normal, any length), scales[3] (activated), rot_cov[4] (raw quaternion of get_covariance, normalised inside),
 *   rot_axis[4] (quaternion of get_minimum_axis, normalised inside), albedo[3], roughness[3], occlusion[3],
 *   shs[M][3] or null (null: no colours), campos[3], viewmatrix[16] (row-vector convention, as the rasterizer's).
 * Outputs: cov3D[P][6] (upper triangle of T R S S R^T T^T, S = scale_modifier*scales), colors[P][3] =
 *   max(SH_sh_degree(dir) + 0.5, 0) (needs shs), features[P][18] = normal | world_normal | albedo | occlusion |
 *   roughness mean x3 | minimum axis, i.e. the `extra_features` array of gsr_rasterize_forward_ex.
 * Equal scales: the minimum-axis order is the stable one (lowest index first); torch.argsort leaves it unspecified. */
int gsr_frame_attributes_forward(int P, int sh_degree, int M, const float *means3D, const float *transforms,
                                 const float *world_normals, const float *scales, float scale_modifier,
                                 const float *rot_cov, const float *rot_axis, const float *albedo,
                                 const float *roughness, const float *occlusion, const float *shs,
                                 const float *campos, const float *viewmatrix, float *cov3D, float *colors,
                                 float *features, gsr_stream_t stream);

/* Backward of gsr_frame_attributes_forward (what autograd derives for the reference's op chain).  Incoming gradients
 * dL_dcov3D[P][6], dL_dcolors[P][3], dL_dfeatures[P][18] may each be null (= zero).  Every outgoing array is fully
 * written (no accumulation): dL_dmeans3D[P][3] (view-direction dependence of the colours), dL_dtransforms[P][9],
 * dL_dworld_normals[P][3], dL_dscales[P][3], dL_drot_cov[P][4], dL_drot_axis[P][4], dL_dalbedo / dL_droughness /
 * dL_docclusion [P][3], dL_dshs[P][M][3] (needs shs; may be null for M = 16 when the caller does not want the SH gradient -- the
 * view-parallel compact exchange rebuilds it from dL_dcolors, gsr_sh_grad_from_views_posed). */
int gsr_frame_attributes_backward(int P, int sh_degree, int M, const float *means3D, const float *transforms,
                                  const float *world_normals, const float *scales, float scale_modifier,
                                  const float *rot_cov, const float *rot_axis, const float *albedo,
                                  const float *roughness, const float *occlusion, const float *shs,
                                  const float *campos, const float *viewmatrix, const float *dL_dcov3D,
                                  const float *dL_dcolors, const float *dL_dfeatures, float *dL_dmeans3D,
                                  float *dL_dtransforms, float *dL_dworld_normals, float *dL_dscales,
                                  float *dL_drot_cov, float *dL_drot_axis, float *dL_dalbedo, float *dL_droughness,
                                  float *dL_docclusion, float *dL_dshs, gsr_stream_t stream);

/* The same two operations reading the SH coefficients from the model's TWO parameter tensors in place -- shs = the DC
 * coefficient [P][1][3], shs_rest = the other 15 [P][15][3] (16-byte aligned), M = 16 -- instead of through the torch.cat of
 * get_features (scene/gaussian_model.py:167-171; 38 MB copied per frame at 200k Gaussians, and split again in backward); the
 * backward writes dL_dshs [P][1][3] and dL_dshs_rest [P][15][3].  shs_rest = null: exactly the functions above. */
int gsr_frame_attributes_forward_split(int P, int sh_degree, int M, const float *means3D, const float *transforms,
                                       const float *world_normals, const float *scales, float scale_modifier,
                                       const float *rot_cov, const float *rot_axis, const float *albedo, const float *roughness,
                                       const float *occlusion, const float *shs, const float *shs_rest, const float *campos,
                                       const float *viewmatrix, float *cov3D, float *colors, float *features, gsr_stream_t stream);
int gsr_frame_attributes_backward_split(int P, int sh_degree, int M, const float *means3D, const float *transforms,
                                        const float *world_normals, const float *scales, float scale_modifier,
                                        const float *rot_cov, const float *rot_axis, const float *albedo, const float *roughness,
                                        const float *occlusion, const float *shs, const float *shs_rest, const float *campos,
                                        const float *viewmatrix, const float *dL_dcov3D, const float *dL_dcolors,
                                        const float *dL_dfeatures, float *dL_dmeans3D, float *dL_dtransforms,
                                        float *dL_dworld_normals, float *dL_dscales, float *dL_drot_cov, float *dL_drot_axis,
                                        float *dL_dalbedo, float *dL_droughness, float *dL_docclusion, float *dL_dshs,
                                        float *dL_dshs_rest, gsr_stream_t stream);
/* gsr_frame_attributes_backward_split with two accumulations that save autograd an add kernel each in render()'s frame:
 * acc_dmeans3D [P][3] (or null) -- the rasterizer's dL_dmeans3D of the same frame -- is ADDED to dL_dmeans3D; and
 * dL_droughness == dL_dalbedo (the same pointer: albedo and roughness are one tensor, scene/gaussian_model.py:197-199) makes the
 * kernel write their SUM there.  (Both also hold for the function above: it passes acc_dmeans3D = null.) */
int gsr_frame_attributes_backward_acc(int P, int sh_degree, int M, const float *means3D, const float *transforms,
                                      const float *world_normals, const float *scales, float scale_modifier,
                                      const float *rot_cov, const float *rot_axis, const float *albedo, const float *roughness,
                                      const float *occlusion, const float *shs, const float *shs_rest, const float *campos,
                                      const float *viewmatrix, const float *dL_dcov3D, const float *dL_dcolors,
                                      const float *dL_dfeatures, float *dL_dmeans3D, float *dL_dtransforms,
                                      float *dL_dworld_normals, float *dL_dscales, float *dL_drot_cov, float *dL_drot_axis,
                                      float *dL_dalbedo, float *dL_droughness, float *dL_docclusion, float *dL_dshs,
                                      float *dL_dshs_rest, const float *acc_dmeans3D, gsr_stream_t stream);

/* The per-Gaussian skinning-weight offset network of render() (nets/mlp_delta_weight_lbs.py:5-32: a 63-d positional embedding of
 * the canonical position through 63-128-128-128-(63+128)-128-24 with ReLU; gaussian_renderer/__init__.py:100-106 runs it every frame
 * when motion_offset_flag is set) on the matrix cores (csrc/mlp.hip: f32 MFMA, activations in registers): forward = one kernel.
 *   gsr_lbs_offset_mlp_pack: weights[5] / biases[5] = the module's tensors in its own layout -- bw_linears.0..3 ([128][63],
 *     [128][128], [128][128], [128][191]: Conv1d weight [out][in][1]) and bw_fc ([24][128]), biases [128] x 4 and [24] -- host arrays
 *     of DEVICE pointers; packed: gsr_lbs_offset_mlp_packed_floats() floats, 16-byte aligned (re-pack after every parameter update);
 *   gsr_lbs_offset_mlp_forward: xyz [P][3] -> out [P][24] (the module returns [1][24][P]: the transposed view of this). */
size_t gsr_lbs_offset_mlp_packed_floats(void);
int gsr_lbs_offset_mlp_pack(const float *const *weights, const float *const *biases, float *packed, gsr_stream_t stream);
int gsr_lbs_offset_mlp_forward(int P, const float *xyz, const float *packed, float *out, gsr_stream_t stream);
/* Which matrix instruction the three kernels run on (process-wide): 1 (default) = v_mfma_f32_32x32x16_bf16 with BOTH
 * operands split in two bf16 terms, three products per step (error 2^-16 of a product: 7e-6 of the output's scale against float64,
 * 16 x the rate of the f32 instruction); 0 = v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain, 6e-7). */
int gsr_lbs_offset_mlp_set_precision(int mode);
/* The forward on the bf16 instruction whatever the mode (comparisons: tools/mlp_bench.py). */
int gsr_debug_lbs_offset_mlp_forward_bf16x3(int P, const float *xyz, const float *packed, float *out, gsr_stream_t stream);
/* Backward w.r.t. the parameters (the positions arrive detached, gaussian_renderer/__init__.py:104: no input gradient).  The forward
 * is run again inside (no activation was kept), dL_dout is [P][24]; the gradients are ADDED into dL_dweights[5] / dL_dbiases[5] (host
 * arrays of device pointers, the module's own layouts: zero them first); workspace: gsr_lbs_offset_mlp_backward_workspace_floats(P)
 * floats, 16-byte aligned (every layer's activations and pre-activation gradients, feature-major, for the weight-gradient products). */
size_t gsr_lbs_offset_mlp_backward_workspace_floats(int P);
int gsr_lbs_offset_mlp_backward(int P, const float *xyz, const float *packed, const float *dL_dout, float *workspace,
                                float *const *dL_dweights, float *const *dL_dbiases, gsr_stream_t stream);
/* Bone-count variants of the six entry points above: the same arguments after a leading nb, the output width of bw_fc -- 24 (SMPL:
 * exactly the entry points without _nb) or 55 (SMPL-X: bw_fc [55][128] and [55], out and dL_dout [P][55]).  Any other nb is refused
 * (GSR_EINVAL, or 0 from the two size queries; gsr_last_error() names it) before any other argument or the device is looked at.  A
 * packed buffer holds one bone count: gsr_lbs_offset_mlp_packed_floats_nb(55) is larger than (24), and the two are not
 * interchangeable.  gsr_lbs_offset_mlp_set_precision covers both counts. */
size_t gsr_lbs_offset_mlp_packed_floats_nb(int nb);
int gsr_lbs_offset_mlp_pack_nb(int nb, const float *const *weights, const float *const *biases, float *packed, gsr_stream_t stream);
int gsr_lbs_offset_mlp_forward_nb(int nb, int P, const float *xyz, const float *packed, float *out, gsr_stream_t stream);
int gsr_debug_lbs_offset_mlp_forward_bf16x3_nb(int nb, int P, const float *xyz, const float *packed, float *out, gsr_stream_t stream);
size_t gsr_lbs_offset_mlp_backward_workspace_floats_nb(int nb, int P);
int gsr_lbs_offset_mlp_backward_nb(int nb, int P, const float *xyz, const float *packed, const float *dL_dout, float *workspace,
                                   float *const *dL_dweights, float *const *dL_dbiases, gsr_stream_t stream);

/* The pose-correction network of render() (nets/mlp_delta_body_pose.py: BodyPoseRefiner as scene/gaussian_model.py:95 builds it --
 * total_bones = J, embedding_size = 3(J-1), mlp_width = 128, mlp_depth = 2 -- followed by its RodriguesModule), one single-workgroup
 * launch each way (csrc/pose_refiner.hip).  J = 24 or 55, width = 128, 1 <= B <= 16 pose rows; anything else returns GSR_EINVAL
 * (gsr_last_error() names it) before any other argument or the device is looked at.
 *   x: [B][3(J-1)] float32 with element strides x_row_stride / x_col_stride (a view such as poses[:, 3:] is read in place);
 *   weights[3] / biases[3]: host arrays of DEVICE pointers to block_mlps.0 / .2 / .4 in the module's own layout (Linear weight
 *     [out][in] row-major: [128][3(J-1)], [128][128], [3(J-1)][128]; biases [128], [128], [3(J-1)]);
 *   gsr_pose_refiner_forward: Rs [B][J-1][3][3] = Rodrigues(r) per 3-vector of r = W4 relu(W2 relu(W0 x + b0) + b2) + b4, with
 *     theta = sqrt(1e-5 + |r|^2) (NOT the 1e-8 rule of gsr_body_pose_forward);
 *   gsr_pose_refiner_backward: the forward again, then dL_dRs [B][J-1][3][3] -> dL_dweights[3] / dL_dbiases[3] (host arrays of
 *     device pointers, the module's layouts) and dL_dx [B][3(J-1)] contiguous (or null: not wanted).  Every output is written whole
 *     (no zero fill needed), every sum has a fixed order: two calls give the same bits. */
int gsr_pose_refiner_forward(int J, int B, int width, const float *x, long long x_row_stride, long long x_col_stride,
                             const float *const *weights, const float *const *biases, float *Rs, gsr_stream_t stream);
int gsr_pose_refiner_backward(int J, int B, int width, const float *x, long long x_row_stride, long long x_col_stride,
                              const float *const *weights, const float *const *biases, const float *dL_dRs,
                              float *const *dL_dweights, float *const *dL_dbiases, float *dL_dx, gsr_stream_t stream);

/* ---- Image-based lighting (pbr/light.py, pbr/shade.py; csrc/pbr.hip; the sampling rules are in DESIGN.md "PBR stage") ----
 * A texture is one 2-D image [h][w][C] looked up by uv with the clamp boundary, or a cube map [6][n][n][C] (face order +x -x +y
 * -y +z -z, face-local axes of pbr/light.py cube_to_dir) looked up by direction with bilinear filtering across face edges, each
 * with a list of `levels` mip levels selected by a per-lookup level (mip_level_bias, clamped to [0, levels-1], trilinear).
 * grad[l] (backward only; null = not wanted) is ADDED into: zero it first. */
#define GSR_PBR_MAX_LEVELS 16
typedef struct gsr_pbr_texture {
  int cube;     /* 1: cube map (coords [n][3] directions), 0: 2-D image (coords [n][2] uv) */
  int channels; /* 1..4 */
  int levels;   /* 1..GSR_PBR_MAX_LEVELS */
  int width[GSR_PBR_MAX_LEVELS], height[GSR_PBR_MAX_LEVELS]; /* cube: width == height == the face size */
  const float *data[GSR_PBR_MAX_LEVELS];
  float *grad[GSR_PBR_MAX_LEVELS];
} gsr_pbr_texture;

/* nvdiffrast.torch.texture for the reference's call shapes: out[n][C]; mip_bias [n] may be null (level 0).  The backward writes
 * d_coords ([n][2], 2-D textures only; may be null) and d_bias ([n]; may be null) and adds into tex->grad[]. */
int gsr_pbr_texture_forward(const gsr_pbr_texture *tex, int n, const float *coords, const float *mip_bias, float *out,
                            gsr_stream_t stream);
int gsr_pbr_texture_backward(const gsr_pbr_texture *tex, int n, const float *coords, const float *mip_bias, const float *d_out,
                             float *d_coords, float *d_bias, gsr_stream_t stream);

/* CubemapLight.build_mips: fine [6][n][n][C] (n even) -> coarse [6][n/2][n/2][C], the 2x2 average; its backward is the
 * reference's own (pbr/light.py cubemap_mip.backward, not the adjoint): d_fine at each fine texel-centre direction is the cube
 * lookup of 0.25 * d_coarse.  d_fine is written. */
int gsr_pbr_cube_mip_forward(int n, int channels, const float *fine, float *coarse, gsr_stream_t stream);
int gsr_pbr_cube_mip_backward(int n, int channels, const float *d_coarse, float *d_fine, gsr_stream_t stream);
/* diffuse_cubemap / specular_cubemap (3 channels, [6][n][n][3] -> same size), brute force over every input texel.  The specular
 * forward writes out = rgb / wsum and wsum [6][n][n] (the backward needs it); backward outputs are written. */
int gsr_pbr_diffuse_forward(int n, const float *cube, float *out, gsr_stream_t stream);
int gsr_pbr_diffuse_backward(int n, const float *d_out, float *d_cube, gsr_stream_t stream);
int gsr_pbr_specular_forward(int n, float roughness, float costheta_cutoff, const float *cube, float *out, float *wsum,
                             gsr_stream_t stream);
int gsr_pbr_specular_backward(int n, float roughness, float costheta_cutoff, const float *wsum, const float *d_out,
                              float *d_cube, gsr_stream_t stream);

/* pbr_shading (pbr/shade.py:105-213) over n pixels, one kernel forward and one backward.  diffuse: light.diffuse (the raw cube;
 * the kernel applies pow(1/2.2) and the clamp per tap), specular: light.specular[0..L-1], lut: the BRDF LUT (2-D, 2 channels,
 * channel 0 is read).  Normals and view directions take no gradient. */
typedef struct gsr_pbr_shade {
  int n;
  int tone, gamma;
  const float *normals, *view_dirs, *albedo;   /* [n][3] */
  const float *roughness, *mask;               /* [n] */
  const float *occlusion, *metallic;           /* [n] or null */
  const float *background;                     /* [n][3] or null (zeros) */
  gsr_pbr_texture diffuse, specular, lut;
  float *render_rgb, *diffuse_rgb, *specular_rgb, *diffuse_light;                  /* forward outputs [n][3] */
  const float *d_render_rgb, *d_diffuse_rgb, *d_specular_rgb, *d_diffuse_light;  /* backward inputs [n][3], each may be null */
  float *d_albedo, *d_roughness, *d_occlusion, *d_metallic;                      /* backward outputs (written), each may be null */
} gsr_pbr_shade;
int gsr_pbr_shade_forward(const gsr_pbr_shade *s, gsr_stream_t stream);
int gsr_pbr_shade_backward(const gsr_pbr_shade *s, gsr_stream_t stream);

/* The environment light's own share of a PBR step.  base is a 3-channel cube [6][base_n][base_n][3], looked up
 * exactly as gsr_pbr_texture_forward looks it up (one level, no bias); a zero direction samples 0.  No call reads the device.
 * gsr_pbr_env_grey (train.py:195-198): out[n] = 0.2989 r + 0.587 g + 0.114 b of clamp(lookup(dirs[n][3]), 0, 1); one launch.
 * gsr_pbr_env_tv_* (train.py:352-363): loss[0] = mean((e[1:] - e[:-1])^2) + mean((e[:, 1:] - e[:, :-1])^2), e[h][w][3] the lookup
 *   at dirs[h][w][3], h, w >= 2.  The forward (two launches: per-workgroup partial sums, then one workgroup adds them in a fixed
 *   order) writes e and its partial sums into workspace (gsr_pbr_env_tv_workspace_floats(h, w) floats, e first); the backward (one
 *   launch) reads them and ADDS upstream[0] * d loss / d base into d_base: zero it first.  reduce selects how the backward
 *   splits the samples over workgroups that each sum into an LDS window of d_base and add its non-zero entries to memory once. */
#define GSR_PBR_ENV_TV_AUTO 0   /* the faster of the two where both apply, else WINDOW */
#define GSR_PBR_ENV_TV_WINDOW 1 /* the split of gsr_pbr_texture_backward: any base size, few large workgroup shares */
#define GSR_PBR_ENV_TV_WHOLE 2  /* d_base whole in LDS (it must fit); workgroups of 1,024 samples, at most 256 of them (beyond that a thread takes several samples) */
int gsr_pbr_env_grey(int base_n, const float *base, int n, const float *dirs, float *out, gsr_stream_t stream);
size_t gsr_pbr_env_tv_workspace_floats(int h, int w);
int gsr_pbr_env_tv_forward(int base_n, const float *base, int h, int w, const float *dirs, float *workspace, float *loss,
                           gsr_stream_t stream);
int gsr_pbr_env_tv_backward(int base_n, int h, int w, const float *dirs, const float *workspace, const float *upstream,
                            float *d_base, int reduce, gsr_stream_t stream);
/* render.py:215-222: out[n][3] = -(R rays[n] / max(|rays[n]|, 1e-12)), R the upper-left 3 x 3 block of
 * inverse(world_view_transform^T) ([4][4] row-major on the device, inverted in the kernel by cofactors: a singular matrix gives
 * non-finite directions where torch.inverse raises).  One launch. */
int gsr_pbr_view_dirs(int n, const float *rays, const float *world_view_transform, float *out, gsr_stream_t stream);

/* ---- Occlusion bake (baking.py bake_set; csrc/bake.hip; DESIGN.md "Occlusion bake") ----
 * gsr_bake_grid is pc_to_grid(points, 10): cell[P] = the compact cell id of each point, the occupied cells numbered in (ix, iy, iz)
 * lexicographic order (torch.unique's), centres[n][3] and cell_idx[n][3] (may be null) for the first *n_cells of 1000 rows, size[3]
 * (may be null).  A zero-extent axis puts every point at index 0 there.  *n_cells is read to the host (the call blocks).
 * gsr_bake_plan computes the view-independent cov3D, the needed cube texels (dir_texel: face * 1024 + y * 32 + x per direction)
 * and every (cell, face, tile) instance count into `plan` (kept for gsr_bake_visibility), and returns instances[0] = all of
 * them, instances[1] = the largest cell's (blocks).  gsr_bake_visibility writes vis[C][ndir] = 1 - the rasterizer's alpha (sum of
 * alpha T) at each direction's texel of cell c's cube, rendered without cell c's Gaussians; it processes cells in batches that fit
 * the workspace (20 bytes per instance beside gsr_bake_visibility_workspace_bytes(C, 0); tuning key "bake_batch_cells" caps a
 * batch) and fills stats[4] (may be null): instances, largest batch, batches, capacity.
 * Rule: a direction whose dir_texel is outside [0, 6144) (baking.cube_nearest_texel gives -1 for a zero or non-finite direction)
 * needs no texel and gets NaN in vis, in every row; the other columns do not depend on it.  bake_set never produces such a
 * direction (its 16 x 32 equirect directions all have a texel); the fused=False composition (baking.cube_nearest) reads alpha 0
 * there, which gives 1.0. */
typedef struct gsr_bake_scene {
  int P, C;                                            /* Gaussians, occupied cells */
  const float *means3D, *scales, *rotations, *opacities; /* [P][3] posed means, [P][3] / [P][4] canonical scales / rotations, [P] */
  const int *cell;                                     /* [P] from gsr_bake_grid */
  const float *views, *projs;                          /* [C][6][16] world-view and full projection matrices (the rasterizer's) */
  const int *dir_texel;                                /* [ndir] */
  int ndir;
} gsr_bake_scene;
size_t gsr_bake_grid_workspace_bytes(void);
int gsr_bake_grid(int P, const float *points, int *cell, float *centres, float *size, int *cell_idx, int *n_cells, void *workspace,
                  size_t workspace_bytes, gsr_stream_t stream);
size_t gsr_bake_plan_bytes(int P, int C);
int gsr_bake_plan(const gsr_bake_scene *scene, void *plan, size_t plan_bytes, unsigned long long *instances, gsr_stream_t stream);
size_t gsr_bake_visibility_workspace_bytes(int C, size_t capacity);
int gsr_bake_visibility(const gsr_bake_scene *scene, const void *plan, float *vis, void *workspace, size_t workspace_bytes,
                        unsigned long long *stats, gsr_stream_t stream);
/* occ[P][ndir] = (dirs[d] . normals[p] > 0) * vis[cell[p]][d], the dot summed left to right without contraction */
int gsr_bake_expand(int P, int ndir, const int *cell, const float *normals, const float *dirs, const float *vis, float *occ,
                    gsr_stream_t stream);
/* out[P][3] = clamp(sum_d clamp(occ[p][d], 0, 1) * env[d], 0, 1) over 512 directions (16-byte aligned occ and env) */
int gsr_bake_env_reduce(int P, const float *occ, const float *env, float *out, gsr_stream_t stream);

/* ---- PBR-phase training loss (train.py:296-363 less SSIM, LPIPS and the env-map TV; csrc/pbr_loss.hip) ----
 * Every image is [C][H][W] float32, contiguous, except rgb, which is read (and d_rgb written) at the element strides rgb_stride.
 * Each term is optional: its inputs null (or its flag 0) turn it off, its unweighted value is then 0 and it adds nothing.
 *   terms[0] L1:      mean |rgb - gt| over the 3 * n_b values whose pixel has bound == 1 (n_b = 0: NaN, gradient 0)
 *   terms[1] TV:      masked TV of [a; b] (ca + cb channels) under mask, masked-out entries in the denominators; mask takes a gradient
 *   terms[2] entropy: gaussian_entropy of a ([ca * H][W] view, entropy[0]) plus that of b (entropy[1]): columns 0..2 only, sigma =
 *                     the unbiased variance, a column whose histogram sum is not > 1e-6 adds 0 and gets a zero gradient; W >= 3
 *   terms[3] smooth:  sum over t of mean_{P, gc[t]} |g[t][k1] - g[t][k2]| / (g[t][k2] + 1e-6)
 *   terms[4] prior:   mean of 1 - b[0] over the n_a pixels with mask > 0 (n_a = 0: NaN, gradient 0); mask takes no gradient
 * loss = sum of w * term.  The forward writes loss, terms and, in `workspace` (gsr_pbr_loss_workspace_floats() floats), the
 * per-workgroup partials and the coefficients the backward reads; nothing is read to the host and no float atomics are used, so
 * two calls give the same bits.  The backward multiplies by *upstream (null: 1) read on the device and writes each non-null d_*
 * in full; the smoothness gradient gathers each row's contributions through inv_off / inv_idx (the entries p sorted stably by
 * k1[p], and by k2[p]: offsets [P + 1], entry ids [P]). */
typedef struct gsr_pbr_loss {
  int width, height;
  const float *rgb;                   /* [3][H][W] at rgb_stride (channel, row, column; elements) */
  long long rgb_stride[3];
  const float *gt, *bound;            /* [3][H][W], [H][W] */
  const float *a, *b, *mask;          /* [ca][H][W], [cb][H][W] (or null), [H][W] */
  int ca, cb;
  int tv, entropy[2], prior;          /* term flags */
  int bins;                           /* histogram bins, 1..32, centres lo + (k + 0.5) * (hi - lo) / bins */
  float lo, hi;
  int P;                              /* smoothness: P rows, k1 / k2 [P] in [0, P) */
  const int *k1, *k2;
  const float *g[2];                  /* [P][gc[t]] or null */
  int gc[2];
  const int *inv_off[2], *inv_idx[2]; /* [0]: by k1, [1]: by k2 (backward only) */
  float w_l1, w_tv, w_entropy, w_smooth, w_prior;
  float *loss, *terms;                /* [1], [5] */
  const float *upstream;              /* backward: [1] or null */
  float *d_rgb, *d_a, *d_b, *d_mask;  /* backward outputs, each may be null */
  float *d_g[2];
} gsr_pbr_loss;
size_t gsr_pbr_loss_workspace_floats(void);
int gsr_pbr_loss_forward(const gsr_pbr_loss *loss, float *workspace, gsr_stream_t stream);
int gsr_pbr_loss_backward(const gsr_pbr_loss *loss, const float *workspace, gsr_stream_t stream);

/* ---- SSIM on the bound-mask crop without a host read (train.py:269-281, :318-321; csrc/ssim_crop.hip) ----
 * gsr_bounding_rect: rect[4] = (x, y, w, h) of the nonzero pixels of mask[H][W] with OpenCV's boundingRect meaning -- x, y the
 * smallest column and row that hold a nonzero pixel, w = largest column - x + 1, h likewise, (0, 0, 0, 0) for an all-zero mask.
 * mask_dtype: GSR_MASK_F32 (nonzero = != 0.0f) or GSR_MASK_U8 (uint8 / bool bytes).  Two launches (per-workgroup boxes into
 * `workspace`, gsr_bounding_rect_workspace_ints() ints, then one workgroup folds them); every workspace word that is read has
 * been written by the same call, so the workspace needs no initialisation and none between calls.  No memset, no host read. */
enum { GSR_MASK_F32 = 0, GSR_MASK_U8 = 1 };
size_t gsr_bounding_rect_workspace_ints(void);
int gsr_bounding_rect(int height, int width, const void *mask, int mask_dtype, int *rect, int *workspace, gsr_stream_t stream);

/* SSIM of the crop img[:, y:y+h, x:x+w] for up to GSR_SSIM_CROP_MAX_GROUPS (img1, img2) pairs that share H, W and the device
 * rectangle `rect` (int32 (x, y, w, h); clipped to the frame on the device).  The reference's ssim() pads with zeros, so the crop's
 * SSIM is the full-frame SSIM map of the two images zeroed outside the rectangle, averaged over the rectangle: the kernels launch
 * over the whole frame and take the rectangle from device memory.
 *   forward:  value[g][0] = sum over the rectangle of the map / (planes[g] * w * h); dA / dB / dC[g] ([planes][H][W], all three or
 *             none) get the derivative maps inside the rectangle only (the rest is left as it was and never read).  Per-workgroup
 *             sums go to `workspace` (gsr_ssim_crop_workspace_floats() floats) and are added in a fixed order: two calls on the
 *             same inputs give the same bits.
 *   backward: d_img1[g] ([planes][H][W] contiguous, null = skip the group) = the SSIM backward with the upstream gradient
 *             upstream[g][0] / (planes[g] * w * h) (upstream[g] null: 1) inside the rectangle and 0 outside, written in full.
 * img1 is read at the element strides img1_stride[g] (plane, row, pixel); img2 is contiguous and takes no gradient.
 * An empty rectangle (w == 0 or h == 0) gives value 0 and an all-zero gradient (the reference raises there: conv2d refuses an
 * empty crop). */
#define GSR_SSIM_CROP_MAX_GROUPS 4
typedef struct gsr_ssim_crop {
  int groups, height, width;
  const int *rect;                                    /* device int32[4] */
  int planes[GSR_SSIM_CROP_MAX_GROUPS];               /* 1..65535 in total */
  const float *img1[GSR_SSIM_CROP_MAX_GROUPS];
  long long img1_stride[GSR_SSIM_CROP_MAX_GROUPS][3];
  const float *img2[GSR_SSIM_CROP_MAX_GROUPS];
  float *dA[GSR_SSIM_CROP_MAX_GROUPS], *dB[GSR_SSIM_CROP_MAX_GROUPS], *dC[GSR_SSIM_CROP_MAX_GROUPS];
  float *value[GSR_SSIM_CROP_MAX_GROUPS];             /* forward: [1] each */
  const float *upstream[GSR_SSIM_CROP_MAX_GROUPS];    /* backward: [1] each, or null */
  float *d_img1[GSR_SSIM_CROP_MAX_GROUPS];            /* backward */
} gsr_ssim_crop;
size_t gsr_ssim_crop_workspace_floats(int total_planes, int height, int width);
int gsr_ssim_crop_forward(const gsr_ssim_crop *crop, float *workspace, gsr_stream_t stream);
int gsr_ssim_crop_backward(const gsr_ssim_crop *crop, gsr_stream_t stream);

/* ---- fused Adam step with the densification statistics (train.py:401-423; csrc/adam.hip) ----
 * The update rule of torch.optim.Adam(betas, eps, weight_decay = 0, amsgrad = False, maximize = False) for up to
 * GSR_ADAM_MAX_ARRAYS tensors of up to GSR_ADAM_MAX_GROUPS parameter groups in two launches: one that advances the step counters,
 * one that streams every tensor once.  `arrays` and `groups` are HOST arrays (the pointers in them device pointers):
 *   array:  param, grad, exp_avg, exp_avg_sq of `count` floats (count == 0: nothing is moved, the counter still advances; the
 *           pointers may then be null), `group` its entry of `groups`, `step_slot` its counter steps[step_slot] (float32, one
 *           slot per array: a slot may appear once per call);
 *   group:  beta1, beta2 in [0, 1), eps > 0, clamp_min (-inf = none; applied to the parameter after the update), and the
 *           learning rate: lr_table[lr_slot] when the device table lr_table is not null (the form a captured graph needs: the caller
 *           rewrites the table in place between replays), else the by-value lr.
 * Accesses are 16 bytes wide for an array whose four pointers are all 16-byte aligned and 4 bytes wide otherwise.
 * stats (may be null; P == 0 = nothing): rows i < P with filter[i] != 0 get
 *   grad_accum[i] += sqrt(gx^2 + gy^2) with (gx, gy) = grad[i * grad_stride + 0 / 1],  denom[i] += 1,
 *   max_radii[i] = max(max_radii[i], radii[i]);          (scene/gaussian_model.py:764-766, train.py:403)
 * the other rows are not written.  Every element is owned by one lane (no atomics): a call gives the same bits every time.
 * No host read, no allocation, no memset; debug != 0 synchronises the stream and reports what the kernels raised.
 * gsr_stats_update is the statistics block alone (one launch); gsr_adam_chunk_floats() the floats one workgroup takes at a
 * time (an array of n floats occupies ceil(n / chunk) consecutive entries of the launch's flattened work list). */
#define GSR_ADAM_MAX_ARRAYS 64
#define GSR_ADAM_MAX_GROUPS 16
typedef struct gsr_adam_array {
  float *param;
  const float *grad;
  float *exp_avg, *exp_avg_sq;
  long long count;
  int group, step_slot;
} gsr_adam_array;
typedef struct gsr_adam_group {
  double beta1, beta2;
  float lr, eps, clamp_min;
  int lr_slot;
} gsr_adam_group;
typedef struct gsr_adam_stats {
  int P, grad_stride;          /* rows; floats between two rows of grad (>= 2) */
  const float *grad;           /* screen-space gradient, columns 0 and 1 are read */
  const unsigned char *filter; /* [P] uint8 / bool bytes */
  const int *radii;            /* [P] */
  float *grad_accum, *denom, *max_radii; /* [P] each */
} gsr_adam_stats;
int gsr_adam_chunk_floats(void);
int gsr_adam_step(int n_arrays, const gsr_adam_array *arrays, int n_groups, const gsr_adam_group *groups, const float *lr_table,
                  float *steps, const gsr_adam_stats *stats, int debug, gsr_stream_t stream);
int gsr_stats_update(const gsr_adam_stats *stats, int debug, gsr_stream_t stream);

/* ---- evaluation "view finish" without a host read (render.py:186-350, train.py:480-540; csrc/eval.hip) ----
 * Everything the reference's evaluation loop does to one view's images after render() / pbr_shading return, in three launches:
 *   finish:  one pass over the pixels for all slots.  Per slot and pixel, in the reference's order: GSR_EVAL_FLIP_Z (the ground-truth
 *            normal of render.py:190-193: n = n * 2 - 1, channel 2 negated, n = (n + 1) / 2, the same operations in the same order);
 *            GSR_EVAL_FILL: where the bound mask is 0 the value becomes fill = (bg[0] + bg[1] + bg[2] == 0) ? 0 : 1, evaluated on the
 *            device (render.py:250-253, :264-270); clamp to [0, 1] (NaN stays NaN, as torch.clamp); the float result is written to
 *            dst, or over src when dst is null; u8 (may be null) gets uint8(min(max(x * 255 + 0.5, 0), 255)), truncating
 *            (torchvision.utils.save_image), as [H][W][channels] bytes.  For the metric pair the per-channel sums of squared
 *            differences of the finished values go to per-workgroup partials (double, no atomics).
 *   ssim:    forward-only SSIM (11 x 11 window, zero padding; utils/loss_utils.py:36-66) of the finished metric pair: no map is written,
 *            one partial per 16 x 16 tile and plane.
 *   metrics: one workgroup adds the partials in a fixed order (double) and writes table[counter] = (psnr, ssim) with
 *            psnr = mean_c 20 log10(1 / sqrt(mse_c)) (utils/image_utils.py:19-21; mse_c == 0 gives +inf) and ssim = sum / (3 H W),
 *            then stores counter + 1.  counter < 0 or >= capacity: nothing is written to the table and overflow[0] = 1 (sticky).
 * A slot is read at its element strides (plane, row, pixel), so [C][H][W] images and permuted [H][W][C] ones are taken in place;
 * dst, when given, has the same strides.  Slots must not overlap one another.  metric_image = metric_gt = -1: no metrics (the
 * second and third launch are skipped; workspace, counter, table and overflow may then be null).  The workspace
 * (gsr_eval_workspace_floats() floats, 8-byte aligned) needs no initialisation.  No memset, no host read, no allocation: two calls
 * on the same inputs write the same bits. */
#define GSR_EVAL_MAX_SLOTS 16
enum { GSR_EVAL_FILL = 1, GSR_EVAL_FLIP_Z = 2 };
typedef struct gsr_eval_slot {
  float *src;             /* read; finished in place when dst is null */
  float *dst;             /* or null */
  unsigned char *u8;      /* [H][W][channels], or null */
  long long stride[3];    /* elements between planes, rows, pixels of src (and dst) */
  int channels, flags;    /* 1 or 3; GSR_EVAL_FILL | GSR_EVAL_FLIP_Z (FLIP_Z needs 3 channels) */
} gsr_eval_slot;
typedef struct gsr_eval_view {
  int slots, height, width;
  gsr_eval_slot slot[GSR_EVAL_MAX_SLOTS];
  const void *mask;        /* [H][W], device; required when a slot has GSR_EVAL_FILL */
  int mask_dtype;          /* GSR_MASK_F32 or GSR_MASK_U8 */
  const float *background; /* device float[3]; required when a slot has GSR_EVAL_FILL */
  int metric_image, metric_gt; /* slot indices (both 3-channel), or both -1 */
  int *counter;            /* device int[1]: the row of this view */
  double *table;           /* device double[capacity][2]: (psnr, ssim) */
  int capacity;
  int *overflow;           /* device int[1] */
} gsr_eval_view;
size_t gsr_eval_workspace_floats(int height, int width);
int gsr_eval_view_finish(const gsr_eval_view *view, float *workspace, gsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H_INCLUDED */

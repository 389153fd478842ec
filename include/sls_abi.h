/*
 * sls_abi.h — C-ABI of libsls_hip.so, the MI355X (gfx950) implementation of
 * the hot path behind Splat-LOAM's renderer.
 *
 * Every entry point replaces one native call the reference makes through
 * its (un-vendored) CUDA extensions; the Python binding a maintainer adds is
 * shown in INTEGRATION.md and shipped in splat_loam_amd/_abi.py.
 *
 *   reference call site (file:line under /root/reference)      replaced by
 *   ----------------------------------------------------------  -------------------------
 *   GaussianRasterizer.forward, native forward                  sls_forward_stage1/2
 *     gaussian_renderer/__init__.py:26,40-47
 *   loss.backward() -> native backward  slam/mapper.py:201      sls_backward
 *   optimizer.step() (Adam, 4 groups)   slam/mapper.py:204,     sls_adam_step
 *     scene/gaussian_model.py:97-121
 *   distCUDA2(points)  slam/mapper.py:113-115,                  sls_knn_dist2
 *     scene/gaussian_model.py:77-81
 *   GaussianRasterizer.markVisible (lineage API, unused in tree) sls_mark_visible
 *   one iteration of Mapper.optimize  slam/mapper.py:150-204     sls_mapping_step
 *   GSAligner.set_query/set_reference/align                      sls_aligner_normals/_align
 *     slam/tracker.py:141-197 ("next" row 3)
 *   render() post-processing + depth_to_normal + mapper loss     sls_consumer_fwd_bwd
 *     gaussian_renderer/__init__.py:48-93,                       ("next" row 1)
 *     utils/graphic_utils.py:26-88, slam/mapper.py:158-187
 *
 * Conventions
 *   - plain C, no torch types; all pointers are DEVICE pointers to
 *     contiguous float32/int32/uint32/uint64 arrays unless named *_host;
 *   - the CALLER owns every buffer (torch's caching allocator stays the only
 *     device allocator); the library never allocates device memory;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it,
 *     nothing synchronises unless stated;
 *   - return 0 on success, a negative SLS_E_* code on failure; the message
 *     is available from sls_last_error() (thread-local); nothing throws.
 */
#ifndef SLS_ABI_H
#define SLS_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLS_OK 0
#define SLS_E_ARG (-1)      /* bad argument (null pointer, negative size, ...) */
#define SLS_E_HIP (-2)      /* a HIP runtime call or kernel launch failed      */
#define SLS_E_SCRATCH (-3)  /* scratch buffer too small                         */
#define SLS_E_UNSUPPORTED (-4) /* this entry point does not serve the configuration: use the one it names */

/* Camera of one LiDAR keyframe.  Filled by sls_camera_from_matrices from the
 * two matrices the reference passes in GaussianRasterizationSettings
 * (gaussian_renderer/__init__.py:16-24; conventions scene/cameras.py:43-50). */
typedef struct SlsCamera {
    int32_t H, W;           /* image_height, image_width                        */
    int32_t wrap;           /* 1: azimuth wraps (360 deg image), D5             */
    int32_t tile_cull_min;  /* D10: the binning emits only the instances of a surfel's tile rectangle whose tile the
                             * footprint can reach (include/sls_det_math.h: sls_tile_outside), for rectangles of at
                             * least this many (and at most 64) tiles.  0: the default (SLS_TILE_CULL_MIN_DEFAULT: off since
                             * round 3, include/sls_spec.h); 1: test off, every tile of the rectangle; k >= 2: threshold k */
    float fx, fy, cx, cy;   /* K = projmatrix[:3,:3]^T : u = fx*az+cx, v = fy*el+cy */
    float scale_modifier;
    float near_cut, far_cut;
    uint32_t flags;         /* SLS_CAM_LEAN_ALLMAP (bit 0): the caller neither reads allmap's median / distortion planes
                             * (5, 6) nor sends a gradient into them — true for the reference's mapper and tracker, which
                             * run at depth_ratio = 0 and use rend_dist only when meshing
                             * (gaussian_renderer/__init__.py:65-86, scene/postprocessing.py:167-170).  The staged forward
                             * then writes zeros there and sls_backward ignores dL/dallmap[5:7]: the kernels
                             * sls_mapping_step runs.  0 (set by sls_camera_from_matrices): all seven planes. */
    float Rvw[9];           /* row-major: p_view = Rvw * p_world + tvw          */
    float tvw[3];
    float pix_offset[2];    /* D1: pixel (c, r) has image coordinate (c + pix_offset[0], r + pix_offset[1]) in
                             * K-space.  (0, 0) = the lineage convention `pixf = (float)pix` (default, set by
                             * sls_camera_from_matrices); (-0.5, -0.5) = the convention of the reference's own
                             * back-projection and projector (utils/graphic_utils.py:46-49,
                             * scene/preprocessing.py:42-64).  Honoured by the pixel rays (sls_ray_tables), the
                             * centre pixel and with it the tile rectangle, the low-pass term and every cull:
                             * the rasterizer works with the principal point (cx - pix_offset[0],
                             * cy - pix_offset[1]), each rounded once in float. */
} SlsCamera;
#define SLS_CAM_LEAN_ALLMAP 1u

const char *sls_last_error(void);
int sls_version(void);

/* Compile-time tile size of the binning/render kernels (D8). */
int sls_tile_w(void);
int sls_tile_h(void);
/* floats per surfel record / gradient record (include/sls_spec.h). */
int sls_rec_stride(void);
int sls_grec_stride(void);

/* Host helper.  view/proj: row-major 4x4 float, exactly the tensors in
 * GaussianRasterizationSettings.viewmatrix / .projmatrix. */
int sls_camera_from_matrices(const float *view_host, const float *proj_host, int H, int W,
                             float scale_modifier, SlsCamera *out);

/* Host helper: per-column (cos az, sin az) and per-row (cos el, sin el) of the
 * pixel rays at the camera's pix_offset, evaluated in double and rounded once.
 * col_cs_host: 2*W floats, row_cs_host: 2*H floats.  The caller uploads them
 * (they depend on K and pix_offset only). */
int sls_ray_tables(const SlsCamera *cam, float *col_cs_host, float *row_cs_host);
/* Same at image coordinate (c + col_offset, r + row_offset) whatever cam->pix_offset
 * says; the reference's back-projection uses (-0.5, -0.5) (utils/graphic_utils.py:46-49),
 * which is what sls_consumer_fwd_bwd / sls_mapping_step expect as col_cs_half / row_cs_half. */
int sls_ray_tables_at(const SlsCamera *cam, float col_offset, float row_offset, float *col_cs_host,
                      float *row_cs_host);

/* ---- forward, stage 1: preprocess + depth order + scan ---------------------
 * col_cs / row_cs: the DEVICE copies of sls_ray_tables (the tile test of D10 takes its tile-centre directions
 * from them; needed only while that test is on: cam->tile_cull_min >= 2, or 0 with a non-zero default).
 * rec: N*20 floats, radii: N int32, rect: N*4 int32 {txlo,ncols,tylo,nrows},
 * tiles_touched: N uint32 = number of tile instances the surfel emits,
 * tile_mask: N uint64 — bit k set: the k-th tile of the rectangle (row-major, the emission order) is emitted;
 *   rectangles of fewer than cam->tile_cull_min or more than 64 tiles are not tested and emit every tile (mask =
 *   all ones below the tile count); may be null while the test is off,
 * block_box (optional, may be null): N uint32 — the surfel's support box as two ranges over the image's 8x2 pixel
 *   blocks (one word; images up to 4096 x 128).  Handed to stage 2, it lets the tile sort deliver the sorted list
 *   as (surfel, mask of the tile's sixteen pixel blocks the surfel can reach) pairs, which the forward tile kernel
 *   scans 256 at a time instead of staging every record (its "dense rounds", the kernel sls_mapping_step runs),
 * depth: N floats (range of the centre, the sort key),
 * order: N uint32 = surfel index at each position of the (range, index) order (ALL surfels,
 *        culled ones included at their range; they have tiles_touched = 0 and emit nothing),
 * offsets: N uint32 = inclusive scan of tiles_touched[order[.]],
 * total_out: 1 uint32 on the DEVICE = number of tile instances R.
 * The caller reads total_out (one D2H sync, as the lineage does) to size the
 * stage-2 buffers (sls_mapping_step has no such sync). */
size_t sls_stage1_scratch_bytes(int N);
int sls_forward_stage1(const SlsCamera *cam, int N,
                       const float *means3D, const float *scales, const float *rotations,
                       const float *opacities, const float *col_cs, const float *row_cs,
                       float *rec, int32_t *radii, int32_t *rect, uint32_t *tiles_touched, uint64_t *tile_mask,
                       uint32_t *block_box,
                       float *depth, uint32_t *order, uint32_t *offsets, uint32_t *total_out,
                       void *scratch, size_t scratch_bytes, void *stream);

/* ---- forward, stage 2: binning, stable sort by tile, ranges, per-tile render
 * total_dev: the device word stage 1 wrote (= R).  tile_keys/vals and the _tmp
 * pair: R uint32 each (ping-pong).  keys64_out (optional, R uint64): the 64-bit keys
 * (tile << 32 | depth bits) the list is ordered by (asks for the two-array sort: no pairs then).
 * The sorted list of surfel indices comes back as (*sorted_list, *sorted_stride): entry j is
 * (*sorted_list)[j * *sorted_stride] — stride 1: a plain array (vals or vals_tmp; *sorted_in_tmp says which); stride 2: the
 * (surfel, block mask) pairs inside sort_scratch (block_box given, lists long enough or list_pairs = 1, at most
 * 2048 tiles): sort_scratch then has to stay alive as long as the list is used (the backward, the caller).
 * list_pairs: 0 = pairs where R >= 1500 T (the rule of sls_mapping_step), 1 = whenever possible, 2 = never.
 * tile_keys / tile_keys_tmp are SCRATCH: the sorted tile ids are NOT an output.  Where the direct binning serves the
 * image (<= 512 tiles, D10 off — every size the reference meets) nothing is written to them, nor to vals_tmp, and
 * tiles_touched / offsets / total_dev / tile_mask are not read; a caller that wants the keys the list is ordered by
 * passes keys64_out (or derives them from ranges + list + depth, as splat_loam_amd/rasterizer.py:_list_and_keys does).
 * ranges: T*2 uint32 with T = ceil(W/tw)*ceil(H/th).  allmap: 7*H*W floats;
 * pix_state: H*W float4 {T_final, M1, M2, 0}; pix_contrib: H*W uint2
 * {n_contrib, median_contrib}; tile_consumed: T uint32 (list entries consumed
 * before the tile finished, the R_eff of SURVEY §8d).
 * block_masks (optional, may be null; sls_block_mask_bytes(R, H, W) bytes = 128 bytes per
 * instance of capacity + a header: room for every list entry in each of a tile's 16 pixel
 * blocks, of which only what contributes is written or read): forward -> backward hand-over,
 * per pixel block the compact list of the (list position, surfel) pairs that reached one of
 * its pixels; with it sls_backward walks exactly those, 64 per round, instead of re-deriving
 * them with a box test over the tile's whole list (the name is round 2's, when the hand-over
 * was a bit mask per 64 list entries).  *block_masks_shape (may be null): the producer's tag of the hand-over
 * (0: none, 3: the 8x2 pixel blocks' compact lists) — hand it to sls_backward together with the buffer. */
size_t sls_sort_scratch_bytes(uint64_t R);
size_t sls_block_mask_bytes(uint64_t R, int H, int W);
int sls_forward_stage2(const SlsCamera *cam, int N, uint64_t R,
                       const float *rec, const int32_t *rect, const uint32_t *tiles_touched,
                       const uint64_t *tile_mask, const uint32_t *block_box,
                       const float *depth, const uint32_t *order, const uint32_t *offsets,
                       const uint32_t *total_dev,
                       uint32_t *tile_keys, uint32_t *vals, uint32_t *tile_keys_tmp, uint32_t *vals_tmp,
                       void *sort_scratch, size_t sort_scratch_bytes, int *sorted_in_tmp,
                       uint64_t *keys64_out, int list_pairs,
                       const uint32_t **sorted_list, int *sorted_stride,
                       uint32_t *ranges, const float *col_cs, const float *row_cs,
                       float *allmap, float *pix_state, uint32_t *pix_contrib,
                       uint32_t *tile_consumed, uint64_t *block_masks, int *block_masks_shape, void *stream);

/* ---- backward ----------------------------------------------------------
 * vals_sorted (+ vals_stride: 1 or 2, as stage 2 returned them)/ranges/rec/pix_* are the forward's buffers
 * (never allmap: the caller may have overwritten it in place).  block_masks + block_masks_shape: the forward's
 * hand-over and its producer's tag; the compact lists are walked only for tag 3 (otherwise, or with null / 0, the
 * backward culls the tile's list itself).  grec: N*16 floats of
 * scratch (zeroed by the call).  Outputs: dL/dmeans3D (N*3), dL/dscales (N*2),
 * dL/drotations (N*4, w.r.t. the normalised quaternion as passed in),
 * dL/dopacities (N). */
int sls_backward(const SlsCamera *cam, int N, uint64_t R,
                 const float *means3D, const float *scales, const float *rotations,
                 const int32_t *radii, const float *rec,
                 const uint32_t *ranges, const uint32_t *vals_sorted, int vals_stride,
                 const float *col_cs, const float *row_cs,
                 const float *pix_state, const uint32_t *pix_contrib,
                 const float *dL_dallmap, float *grec,
                 float *dL_dmeans3D, float *dL_dscales, float *dL_drotations,
                 float *dL_dopacities, const uint64_t *block_masks, int block_masks_shape, void *stream);

/* ---- pose gradient -------------------------------------------------------------
 * Every backward below has a `_pose` form that also returns g = dL/dxi at xi = 0 for the LEFT perturbation of the view
 * transform, T_vw(xi) = Exp(xi) T_vw with xi = (v, w): to first order p_view -> p_view + w x p_view + v.  pose_grad: 6
 * floats [v | w] in DEVICE memory, written by the backward of the projection itself (a reduction over its surfels: one
 * row per workgroup, added in a fixed order — the same bits from run to run wherever the gradient records are).
 * pose_scratch: sls_pose_grad_scratch_bytes(N) bytes of DEVICE memory, 8-byte aligned, caller-kept, zero-initialised ONCE
 * by the caller; every call leaves it ready for the next (one call at a time per buffer).  A null pose_grad is the
 * call without the suffix, bit for bit.  The discrete choices of the forward are frozen as for the surfels' gradients. */
size_t sls_pose_grad_scratch_bytes(int N);
int sls_backward_pose(const SlsCamera *cam, int N, uint64_t R,
                      const float *means3D, const float *scales, const float *rotations,
                      const int32_t *radii, const float *rec,
                      const uint32_t *ranges, const uint32_t *vals_sorted, int vals_stride,
                      const float *col_cs, const float *row_cs,
                      const float *pix_state, const uint32_t *pix_contrib,
                      const float *dL_dallmap, float *grec,
                      float *dL_dmeans3D, float *dL_dscales, float *dL_drotations,
                      float *dL_dopacities, const uint64_t *block_masks, int block_masks_shape,
                      float *pose_grad, void *pose_scratch, size_t pose_scratch_bytes, void *stream);

/* The same backward with DETERMINISTIC accumulation of the per-surfel gradient records: integer atomics
 * instead of float atomics (first launch: the largest |contribution| per surfel and field; second launch:
 * every contribution scaled by 2^(39 - unbiased exponent of that maximum), rounded, added as a 64-bit integer:
 * 39 fractional bits below the largest term, |q| < 2^40, 23 bits of headroom for the sum), so
 * that two runs on the same inputs return the same bits.  No `grec` buffer; det_scratch: DEVICE scratch of
 * sls_backward_det_scratch_bytes(N). */
size_t sls_backward_det_scratch_bytes(int N);
int sls_backward_det(const SlsCamera *cam, int N, uint64_t R,
                     const float *means3D, const float *scales, const float *rotations, const int32_t *radii,
                     const float *rec, const uint32_t *ranges, const uint32_t *vals_sorted, int vals_stride,
                     const float *col_cs, const float *row_cs, const float *pix_state, const uint32_t *pix_contrib,
                     const float *dL_dallmap,
                     float *dL_dmeans3D, float *dL_dscales, float *dL_drotations, float *dL_dopacities,
                     const uint64_t *block_masks, int block_masks_shape, void *det_scratch, size_t det_scratch_bytes,
                     void *stream);
int sls_backward_det_pose(const SlsCamera *cam, int N, uint64_t R,
                          const float *means3D, const float *scales, const float *rotations, const int32_t *radii,
                          const float *rec, const uint32_t *ranges, const uint32_t *vals_sorted, int vals_stride,
                          const float *col_cs, const float *row_cs, const float *pix_state, const uint32_t *pix_contrib,
                          const float *dL_dallmap,
                          float *dL_dmeans3D, float *dL_dscales, float *dL_drotations, float *dL_dopacities,
                          const uint64_t *block_masks, int block_masks_shape, void *det_scratch, size_t det_scratch_bytes,
                          float *pose_grad, void *pose_scratch, size_t pose_scratch_bytes, void *stream);

/* ---- forward / backward in ONE call each, against a capacity (no host read of R) ---------------------------
 * What `GaussianRasterizer` runs by default (gaussian_renderer/__init__.py:26,40-47; slam/mapper.py:201): the kernels
 * of sls_mapping_step behind the staged interface's contract.  The instance buffers are sized for `R_capacity` (the
 * caller's guess: last call's R with head room); the status block (R, bit 0 of `overflow`: capacity too small, bit 1:
 * the repaired depth order was not exact) reaches `status_mirror` (pinned HOST memory, optional) from the first
 * workgroup of the binning kernel, a few microseconds into it, words 0..6 before word 7: the caller arms words 0 and 7 with a value
 * the device never writes (0xFFFFFFFF) and polls them while the binning and the tile forward run; a non-zero `overflow` means the
 * outputs are void — repeat with more room resp. with reuse_rounds = 0.
 * depth_order (N uint32, caller-kept PER CAMERA, may be null with reuse_rounds = 0): receives the depth order;
 * reuse_rounds 1..4 repairs the order found there (from this camera's previous call) instead of sorting from scratch
 * — verified exact on the device, bit 1 otherwise.  list_pairs as in stage 2.
 * workspace: sls_forward_ws_bytes(N, H, W, R_capacity) bytes, 256-byte aligned, alive until the backward has run;
 * workspace_ready = 0 on its first use (a region of it must start from zero; forward and backward leave it so).
 * want_backward = 0 (render() under no_grad: Mapper.densify, the tracker): no forward -> backward hand-over is written.
 * radii (N int32), allmap (7*H*W floats): tensors of the caller's own.  *sorted_list / *sorted_stride /
 * *block_masks_shape: what sls_backward_ws wants back (pointers into the workspace).
 * Serves what the direct binning serves (<= 512 tiles, images the block boxes describe, D10 off): otherwise
 * SLS_E_UNSUPPORTED, and the staged forward is the way. */
struct SlsMappingStatus;
size_t sls_forward_ws_bytes(int N, int H, int W, uint64_t R_capacity);
int sls_forward_ws(const SlsCamera *cam, int N, const float *means3D, const float *scales, const float *rotations,
                   const float *opacities, const float *col_cs, const float *row_cs, uint64_t R_capacity,
                   uint32_t *depth_order, int reuse_rounds, int list_pairs, int workspace_ready, int want_backward,
                   int32_t *radii, float *allmap, void *workspace, size_t workspace_bytes, struct SlsMappingStatus *status_dev,
                   struct SlsMappingStatus *status_mirror, const uint32_t **sorted_list, int *sorted_stride,
                   int *block_masks_shape, void *stream);
/* Blocks until words 0 and 7 of the pinned status mirror sls_forward_ws was given differ from `sentinel` (the caller
 * arms both with a value the device never writes): a bounded spin on the calling thread — no interpreter lock is held by
 * a ctypes caller meanwhile — then a drain of the stream as a last resort. */
int sls_wait_status_mirror(const void *mirror_host, uint32_t sentinel, void *stream);
/* The backward of that forward: tile backward (it marks the surfels it reaches) + the projection's backward, which
 * reads — and clears — only the marked surfels' gradient records: no 64 N-byte memset per call.  block_order (optional;
 * sls_block_order_bytes(H, W) bytes, zero-initialised, caller-kept PER CAMERA): the tile backward walks its pixel blocks
 * most expensive first in the order this camera's previous backward left there, and leaves the next one.  Float atomics
 * (sls_backward_det on the staged buffers is the bit-reproducible alternative). */
int sls_backward_ws(const SlsCamera *cam, int N, const float *means3D, const float *scales, const float *rotations,
                    const int32_t *radii, const float *col_cs, const float *row_cs, const float *dL_dallmap,
                    uint64_t R_capacity, void *workspace, size_t workspace_bytes, const uint32_t *sorted_list,
                    int sorted_stride, int block_masks_shape, uint32_t *block_order, float *dL_dmeans3D,
                    float *dL_dscales, float *dL_drotations, float *dL_dopacities, void *stream);
int sls_backward_ws_pose(const SlsCamera *cam, int N, const float *means3D, const float *scales, const float *rotations,
                         const int32_t *radii, const float *col_cs, const float *row_cs, const float *dL_dallmap,
                         uint64_t R_capacity, void *workspace, size_t workspace_bytes, const uint32_t *sorted_list,
                         int sorted_stride, int block_masks_shape, uint32_t *block_order, float *dL_dmeans3D,
                         float *dL_dscales, float *dL_drotations, float *dL_dopacities, float *pose_grad,
                         void *pose_scratch, size_t pose_scratch_bytes, void *stream);

/* ---- fused consumer of allmap: render() post-processing + mapper loss ------
 * Computes, from allmap (7*H*W, NOT modified), the three per-pixel loss terms of
 * slam/mapper.py:174-187 on top of the maps of gaussian_renderer/__init__.py:48-93
 * and writes dL/dallmap (7*H*W) for a loss weight of 1.
 *   loss_sums (4 floats, device): [sum_valid |s-gt|, sum_valid (1-<n_hat,n_surf*alpha>),
 *                                  sum_valid BCE(alpha,1), total]
 *   total = sums[0]/(H*W) + lambda_normal*sums[1]/n_valid + lambda_alpha*sums[2]/n_valid
 * gt_depth: H*W floats, valid: H*W uint8 (1 = valid), col_cs_half/row_cs_half: ray
 * tables at offset (-0.5,-0.5) (device), n_valid: number of valid pixels (host). */
size_t sls_consumer_scratch_bytes(int H, int W);
int sls_consumer_fwd_bwd(int H, int W, const float *allmap, const float *gt_depth, const uint8_t *valid,
                         const float *col_cs_half, const float *row_cs_half, float depth_ratio,
                         float lambda_normal, float lambda_alpha, int n_valid, float *loss_sums,
                         float *dL_dallmap, void *scratch, size_t scratch_bytes, void *stream);

/* render()'s post-processing alone — what the reference's NO-GRAD callers of gaussian_renderer.render read
 * (gaussian_renderer/__init__.py:48-93 + utils/graphic_utils.py:26-88; callers: slam/mapper.py:52-54,
 * slam/tracker.py:173-175, slam/slam.py:81-82, scene/postprocessing.py:162): one launch instead of ~30 torch kernels.
 *   view_rot9: HOST pointer, world_view_transform[:3,:3] row-major (as a matrix: view frame -> world);
 *   out: rend_normal (3*H*W, world frame), surf_depth (H*W), surf_normal (3*H*W, world frame, x alpha, zero border);
 *   rend_alpha / rend_dist are planes 1 / 6 of allmap themselves. */
int sls_render_maps(int H, int W, const float *allmap, const float *view_rot9, const float *col_cs_half,
                    const float *row_cs_half, float depth_ratio, float *rend_normal, float *surf_depth,
                    float *surf_normal, void *stream);

/* Mapper.densify's candidates and sampling weights (slam/mapper.py:51-102 with densify_threshold_egeom <= 0;
 * utils/graphic_utils.py:91-106): weights_out[H*W] = |central differences of log(depth)| at the valid pixels rendered
 * with alpha <= threshold_opacity (rend_alpha = NULL: at every valid pixel — a model's first keyframe), 0 elsewhere;
 * stats_out (4 words, device): [#candidates, float bits of the gradient's maximum over the image, float sum of the
 * weights, 0].  valid: uint8, 1 = valid. */
int sls_densify_weights(int H, int W, const float *image_depth, const uint8_t *valid, const float *rend_alpha,
                        float threshold_opacity, float *weights_out, uint32_t *stats_out, void *stream);

/* Mapper.densify's draw on the device: sls_densify_weights, then WHICH candidates become surfels — weighted sampling
 * without replacement, proportional to the weights (the distribution of torch.multinomial(replacement=False)), as an
 * exponential race whose every random word is a pure function of (pixel, seed, draw_index): include/sls_draw_math.h
 * states the arithmetic, DESIGN.md section 2 the selection (the k = (uint32)(percentage * #candidates) smallest of
 * (key bits, pixel); nothing where k < 2, the gradient's maximum is not > 0 or sum / maximum <= 1e-5).  The same
 * (weights, seed, draw_index) give the same pixels on every run and device.
 *   weights_out (H*W floats), stats_out[0..2]: as sls_densify_weights leaves them.
 *   pixels_out (capacity H*W int64): the n_drawn drawn pixels, row-major indices in ascending order (what torch's
 *       nonzero() of the drawn mask holds: sls_densify_rows takes them as they are); the rest is not written.
 *   stats_out (8 words, device): [#candidates, gradient maximum bits, weight sum bits, n_drawn, k, bits of the k-th
 *       key, how many pixels of exactly that key are drawn, 1].
 *   stats_mirror (optional, PINNED HOST, 8 words): the same block written by the device as soon as n_drawn is known
 *       (words 5 and 6 still 0); arm words 0 and 7 with a value the device never writes (0xFFFFFFFF) and wait with
 *       sls_wait_status_mirror — the one host read of the draw.
 *   scratch: sls_densify_draw_scratch_bytes(H, W) bytes, 16-byte aligned.
 * Serves H*W <= SLS_DENSIFY_DRAW_MAX_PIXELS (the selection is one workgroup over keys resident in L2); SLS_E_UNSUPPORTED
 * beyond.  SLS_E_ARG before anything is enqueued: a null pointer (rend_alpha and stats_mirror may be null), a
 * non-positive size, percentage outside [0, 1] or NaN, too little scratch. */
#define SLS_DENSIFY_DRAW_MAX_PIXELS 262144
size_t sls_densify_draw_scratch_bytes(int H, int W);
int sls_densify_draw(int H, int W, const float *image_depth, const uint8_t *valid, const float *rend_alpha,
                     float threshold_opacity, double percentage, uint64_t seed, uint32_t draw_index, float *weights_out,
                     int64_t *pixels_out, uint32_t *stats_out, uint32_t *stats_mirror, void *scratch, size_t scratch_bytes,
                     void *stream);

/* Mapper.densify's new rows (slam/mapper.py:104-137) for n drawn pixels (row-major indices, int64 as torch's nonzero
 * leaves them): centres = the measured points in the model frame, rotations = unit quaternions (w,x,y,z; w >= 0) whose
 * third axis is the measured normal (utils/general_utils.py:85-187).  All pointers DEVICE; cam_to_model16 =
 * inv(world_view_transform^T), model_T_frame16 = the keyframe's pose in the model, both row-major 4x4.  Scales (3-NN,
 * sls_knn_dist2) and opacity (0.9) are the caller's. */
int sls_densify_rows(int n, int H, int W, const int64_t *pixels, const float *image_depth, const float *image_normal,
                     const float *col_cs_half, const float *row_cs_half, const float *cam_to_model16,
                     const float *model_T_frame16, float *xyz_out, float *quat_out, void *stream);

/* Oriented surface points of a rendered keyframe — steps 3-4 of the reference's mesh_poisson
 * (scene/postprocessing.py:164-188): filter by rend_alpha / rend_dist, back-project, sample kf_samples pixels, move to
 * the world frame — without its boolean gather, its host copies and its unseeded np.random.choice.  DESIGN.md section 2,
 * "Surface samples", states every step; include/sls_draw_math.h the random word and the rank (sls_sample_word,
 * sls_sample_index).
 *   allmap: the rasterizer forward's 7*H*W floats, FULL (plane 6, rend_dist, is read: not a lean_allmap render).
 *   valid pixel: !(alpha < min_opacity) && !(dist > max_depth_dist); sample j takes the valid pixel of row-major rank
 *       sls_sample_index(sls_sample_word(j, seed, frame_id), n_valid): uniform, with replacement, row j of the output.
 *   points_out / normals_out (n_samples*3 each): M (depth ray) and R(M) (N / alpha); depth = (1 - depth_ratio) D / alpha +
 *       depth_ratio median (the divisions where alpha > 0), ray from the half-pixel tables (sls_ray_tables_at(-.5, -.5)).
 *   cam_to_world12: DEVICE, 3x4 row-major, M = world_T_model inv(world_view_transform^T).
 *   pixels_out (optional, n_samples int32): the selected row-major pixel of each row.
 *   status_out (DEVICE, 4 words): [n_valid, rows written (n_samples, or 0 where n_valid == 0: nothing else is written
 *       then), 0, 1].  Nothing is read back: a run keeps its keyframes' words in one array and reads it once.
 *   scratch: sls_surface_scratch_bytes(H, W) bytes, 8-byte aligned (one validity bit per pixel).
 * Two launches, ordered by the stream alone.  Serves H*W <= SLS_SURFACE_MAX_PIXELS (the prefix of the validity words'
 * popcounts lives in LDS); SLS_E_UNSUPPORTED beyond.  SLS_E_ARG before anything is enqueued: a null pointer (pixels_out
 * may be null), a non-positive size, n_samples < 1, a NaN threshold or depth_ratio, too little scratch. */
#define SLS_SURFACE_MAX_PIXELS 262144
size_t sls_surface_scratch_bytes(int H, int W);
int sls_surface_samples(int H, int W, const float *allmap, const float *col_cs_half, const float *row_cs_half,
                        const float *cam_to_world12, float min_opacity, float max_depth_dist, float depth_ratio,
                        int n_samples, uint64_t seed, uint32_t frame_id, float *points_out, float *normals_out,
                        int32_t *pixels_out, uint32_t *status_out, void *scratch, size_t scratch_bytes, void *stream);

/* ---- one whole mapping iteration, enqueued without any host sync -----------
 * slam/mapper.py:150-204 for one keyframe: activations (scene/gaussian_model.py:
 * 39-44) -> rasterizer forward -> sls_consumer_fwd_bwd -> rasterizer backward ->
 * activation backward + scale regulariser (slam/mapper.py:190-195) -> Adam.
 * Parameters are the RAW (pre-activation) tensors of the model.  grads /
 * exp_avg / exp_avg_sq are flat 10*N buckets laid out [xyz 3N | opacity N |
 * scaling 2N | rotation 4N] (the optimiser's group order) — one contiguous
 * buffer, i.e. one RCCL all-reduce in the keyframe-parallel mode.
 * The instance count R stays on the device: buffers are sized for R_capacity;
 * if R exceeds it the excess is dropped, status.overflow is set and the Adam
 * update is skipped (the caller grows the capacity and repeats the iteration).
 * status_dev lives in DEVICE memory; read it after the stream has drained.
 * *allmap_out (optional) receives the address of allmap inside the workspace; with
 * depth_ratio == 0 the loss neither reads nor differentiates planes 5 (median) and 6
 * (distortion) — gaussian_renderer/__init__.py:79-86 — and this call leaves them zero
 * (sls_forward_stage2 always fills all seven). */
struct SlsMappingStatus;
typedef struct SlsMappingConfig {
    float lambda_alpha, lambda_normal, scaling_max, scaling_max_penalty, depth_ratio;
    float lr_xyz, lr_opacity, lr_scaling, lr_rotation;
    int32_t apply_adam;   /* 0: gradients only (all-reduce them, then sls_adam_step) */
    int32_t reuse_depth_order; /* 0: sort from scratch.  2 (up to 4): as 1 with that many repair rounds, each of which
                                * lets a surfel travel one more window of 1024 positions (still one launch: only the windows near
                                * a boundary that one round leaves out of order run the further rounds).
                                * 1: the workspace still holds the depth order of the previous iteration on the
                                * SAME keyframe and surfel set: repair it (windowed re-sort + verification)
                                * instead of sorting from scratch.  If the repair does not reach the exact
                                * order, bit 1 of status.overflow is set, Adam is skipped, repeat with 0. */
    int32_t keep_grads;   /* apply_adam = 1 only: 1 = also write the gradients to `grads` (with 0 they are
                           * consumed where they are produced and `grads` is left untouched) */
    int32_t workspace_ready; /* 0 on the first call with a (new) workspace, 1 afterwards: the call keeps the
                              * accumulation buffers inside the workspace zeroed for its successor */
    double beta1, beta2, eps;
    uint32_t *depth_order;   /* optional DEVICE buffer of N uint32: where this keyframe's depth order is kept
                              * (read with reuse_depth_order >= 1, always written); null: inside the workspace */
    struct SlsMappingStatus *status_mirror; /* optional, HOST-visible (pinned, device-mapped) memory: the last
                              * kernel of the iteration copies *status_dev there, so the caller can read the
                              * status after an event/stream wait without enqueuing a device->host copy */
    float *void_flags_out;   /* optional DEVICE pointer to 2 floats (keyframe-parallel mode: the two words after the
                              * gradient bucket): [0] = 1.0 if bit 0 of status.overflow is set, [1] = 1.0 if any
                              * other bit is, else 0.0 — summed over ranks by the gradient all-reduce and then
                              * handed to sls_adam_step_reduced */
    uint32_t grad_chunk;     /* 0: `grads` is the flat bucket [xyz 3N | opacity N | scaling 2N | rotation 4N].
                              * C > 0 (a multiple of 4, N even, apply_adam = 0): reduce-scatter layout for
                              * `grad_ranks` ranks — flat element e lives at e + 4 * (e / C), i.e. rank g's chunk of C
                              * elements is followed by 4 words whose first two receive the void flags (as
                              * void_flags_out, which is ignored then): after a SUM reduce-scatter every rank finds the
                              * group's verdict behind its own chunk.  `grads` holds grad_ranks * (C + 4) floats. */
    uint32_t grad_ranks;
    int32_t deterministic;   /* 1: the backward tile kernel accumulates the gradient records with integer atomics
                              * (two launches: per-field maximum, then fixed-point sum scaled by it): bit-identical
                              * gradients from run to run, about one extra tile-backward per iteration.  0: float
                              * atomics, whose order — and so the last bits of the sums — changes between runs.
                              * 2: the same in ONE launch — every (surfel, field)'s scale is predicted from its sum in
                              * the keyframe's previous iteration (`det_prev`, needed), or from the field's default where
                              * there is no history (defaults are set by iterations run with 1 on the same workspace:
                              * run the first one with 1).  A prediction off by more than 2^22 sets bit 3 of
                              * status.overflow: the iteration is void, repeat it with 1.  Needs the default 8x2 tile
                              * kernels.  Deterministic: the scales depend on earlier (deterministic) results only. */
    int32_t block_masks;     /* the forward tile kernel's dense rounds (tile sort delivers (surfel, block mask) pairs,
                              * DESIGN.md section 4): 0 = where the lists are long enough to pay (capacity >= 1500
                              * instances per tile), 1 = always, 2 = never.  Same results either way. */
    uint64_t *grad_bitmap;   /* optional DEVICE buffer of sls_grad_bitmap_words(N) uint64 (apply_adam = 0, flat `grads`):
                              * bit i of word i / 64 is set iff surfel i has a non-zero gradient in this iteration
                              * (the keyframe reached it, or the scale regulariser pushes on it); the two words behind
                              * the bitmap receive the void flags (non-zero: bit 0 resp. any other bit of
                              * status.overflow) — OR-reduced over the ranks they are the group's verdict
                              * (sls_grad_compact / sls_adam_step_sparse) */
    uint8_t *det_prev;       /* optional DEVICE buffer of 16 N bytes, zero-initialised by the caller, one per keyframe
                              * (deterministic = 1 or 2): the predicted scale of every (surfel, field), rewritten by each
                              * iteration that is not void */
    int32_t phase;           /* 0: the whole iteration.  1: up to and including the tile backward; 2: the rest (backward
                              * of the projection [+ Adam]) of the iteration phase 1 started — same arguments, same
                              * workspace.  Between the two the caller can start a collective that needs nothing of
                              * phase 2: with grad_bitmap, phase 1 ends by writing the bitmap EARLY — the surfels the
                              * tile backward reached or the scale regulariser may push on, a superset of the non-zero
                              * gradients (zero rows change no sum) — so that the ranks' bitmaps can be all-gathered
                              * while phase 2 runs (MappingEngine.overlap) */
    int32_t reserved;
    uint32_t *block_order;   /* optional DEVICE buffer of sls_block_order_bytes(H, W) bytes, zero-initialised by the caller, one
                              * per keyframe: the launch order of the keyframe's tile backward (most expensive pixel blocks
                              * first), written by every iteration for the keyframe's next one.  With it the loss stage
                              * has no launch of its own: the tile backward computes the per-pixel loss terms and their
                              * gradient itself (default 8x2 kernel, depth_ratio = 0; otherwise the buffer is ignored).
                              * Same gradients bit for bit; loss_sums are added up in another order (last bits) */
    const uint64_t *union_bitmap;  /* phase 2 of the touched-set exchange (below; apply_adam = 1, N even): the OR of the ranks'
                              * bitmaps (sls_grad_union's output).  The backward of the projection then WRITES the gradient
                              * row of every surfel of the union into its slot of `grad_compact` (no flat bucket, no packing
                              * launch) and leaves its parameters alone; every other surfel — zero gradient on every rank —
                              * gets its Adam update right there, as on one GPU.  After the SUM of the rows,
                              * sls_adam_step_union updates the union's surfels.  A non-zero gradient outside
                              * the union (a bitmap that was no superset) sets bit 5 of status.overflow. */
    const uint32_t *union_prefix;  /* sls_grad_union's word_prefix */
    float *grad_compact;     /* capacity x 10 floats */
    uint32_t *grad_compact_index;  /* capacity uint32: the surfel of every slot (for sls_adam_step_union) */
    uint32_t grad_compact_capacity;
    uint32_t reserved2;
    float *pose_grad;        /* optional DEVICE pointer to 6 floats [v | w]: the keyframe's pose gradient (D11, see
                              * sls_backward_pose) of the pixel loss, written by the iteration's last launch — served with
                              * apply_adam 0 and 1, deterministic 0 / 1 / 2 (1 and 2: the same bits from run to run), phase 0
                              * and 2 (phase 1 ends before that launch and does not touch it).  With the touched-set
                              * exchange (union_bitmap) the kernel takes the same reduction, but no test runs that
                              * combination: treat it as unexercised.  The scale regulariser does not depend on the
                              * pose.  Void iteration: void gradient.
                              * Null: the iteration as it was, bit for bit.  sls_mapping_step_batch: must be null here (one
                              * pointer per SlsKeyframeInputs instead) */
    void *pose_scratch;      /* with pose_grad: sls_pose_grad_scratch_bytes(N) bytes (x G for a batch), 8-byte aligned,
                              * zero-initialised once by the caller; NOT part of the workspace, whose sizes are unchanged */
    size_t pose_scratch_bytes;
} SlsMappingConfig;
typedef struct SlsMappingStatus {
    uint32_t R;           /* tile instances of this iteration */
    uint32_t overflow;    /* bit 0: R > R_capacity; bit 1: depth-order repair failed (reuse_depth_order); bit 2: the
                           * sparse exchange's compact buffer was too small (sls_grad_union / sls_grad_compact); bit 3: a predicted scale
                           * of the one-pass deterministic accumulation was off (deterministic = 2: repeat with 1).
                           * Non-zero: results of this iteration are void, Adam was skipped */
    float loss_sums[4];   /* sums of the three pixel terms, pixel-loss total */
    float loss_reg;       /* scale regulariser */
    uint32_t exchange_count;  /* sparse exchange only: number of surfels in the union of the ranks' touched sets */
} SlsMappingStatus;
size_t sls_mapping_workspace_bytes(int N, int H, int W, uint64_t R_capacity);
size_t sls_block_order_bytes(int H, int W);   /* SlsMappingConfig.block_order */
/* The same for ONE configuration: without cfg->deterministic the two fixed-point accumulators (192 B per
 * surfel, about as much as the rest of the per-surfel workspace) are not reserved.  A workspace sized by
 * sls_mapping_workspace_bytes fits every configuration. */
size_t sls_mapping_workspace_bytes_cfg(int N, int H, int W, uint64_t R_capacity, const struct SlsMappingConfig *cfg);
int sls_mapping_step(const SlsCamera *cam, int N,
                     float *xyz, float *scaling_raw, float *rotation_raw, float *opacity_raw,
                     float *grads, float *exp_avg, float *exp_avg_sq, int64_t adam_step,
                     const float *gt_depth, const uint8_t *valid, int n_valid,
                     const float *col_cs, const float *row_cs,
                     const float *col_cs_half, const float *row_cs_half,
                     const SlsMappingConfig *cfg, uint64_t R_capacity,
                     void *workspace, size_t workspace_bytes,
                     SlsMappingStatus *status_dev, float **allmap_out, void *stream);

/* ---- keyframe-batched mapping step: G keyframes, gradients summed, ONE Adam update ------------------------------
 * sls_mapping_step_batch computes sum_g dL_g/dtheta over G distinct keyframes of the same H x W (each keyframe's pixel
 * loss exactly as sls_mapping_step computes it) plus the scale regulariser ONCE, and applies one Adam update (adam_step:
 * the batch's step number).  The keyframes' fronts (forward, loss, tile backward: the kernels of sls_mapping_step, G
 * launches each) run one after another and share the workspace's scratch; each keeps only what the last launch reads
 * (radii, gradient records, loss terms, block costs) in a part of its own.  ONE launch then reads the parameters once, chains every
 * keyframe's gradient record through its camera, sums them in the order 0..G-1, adds the regulariser and applies Adam.
 * If any keyframe's iteration is void (instance overflow, failed depth-order repair) the whole batch is void: no
 * parameter and no moment changes.
 *   cfg: shared by the keyframes; cfg->depth_order / block_order / det_prev / reuse_depth_order are not read (they are
 *        per keyframe, below).  phase must be 0; grad_chunk, grad_bitmap and union_bitmap are not served.
 *        apply_adam = 0 writes the summed gradient to the flat bucket `grads` and the batch's void flags to
 *        cfg->void_flags_out (the keyframe-parallel all-reduce consumes both).  deterministic = 2 runs as 1 (two
 *        launches per keyframe); det_prev, where given, is still rewritten (the fields' defaults that a one-launch
 *        sls_mapping_step keeps in ITS workspace are not: a keyframe without history there predicts from them).
 *        status_mirror receives status_dev[0].
 *   status_dev: G + 1 blocks in DEVICE memory.  [0] the batch: OR of the keyframes' overflow bits, the largest R, the
 *        loss sums added over the keyframes, the regulariser; [1 + g] keyframe g (its R, bits, loss sums; no regulariser).
 *   SLS_E_ARG (sls_last_error says why), before anything is enqueued: G outside [1, SLS_MAX_BATCH], keyframes of
 *        different H x W, a null per-keyframe pointer (block_order and det_prev are optional, block_order on all
 *        keyframes or none; pose_grad likewise), the same depth_order / block_order / det_prev / pose_grad buffer on
 *        two keyframes, a non-null cfg->pose_grad. */
#define SLS_MAX_BATCH 8
typedef struct SlsKeyframeInputs {
    SlsCamera cam;
    const float *gt_depth;        /* H x W */
    const uint8_t *valid;         /* H x W */
    int32_t n_valid;
    int32_t reuse_depth_order;    /* as SlsMappingConfig.reuse_depth_order, for this keyframe's depth_order */
    const float *col_cs, *row_cs;           /* sls_ray_tables */
    const float *col_cs_half, *row_cs_half; /* the same at pixel offset 0.5 */
    uint32_t *depth_order;        /* N uint32: the keyframe's depth order (as SlsMappingConfig.depth_order; required) */
    uint32_t *block_order;        /* optional: sls_block_order_bytes(H, W) (as SlsMappingConfig.block_order) */
    uint8_t *det_prev;            /* optional: 16 N bytes (as SlsMappingConfig.det_prev) */
    float *pose_grad;             /* optional, on every keyframe or on none: 6 DEVICE floats, this keyframe's pose gradient
                                   * through its own camera (scratch: cfg->pose_scratch, G x sls_pose_grad_scratch_bytes(N)) */
} SlsKeyframeInputs;
/* One sls_mapping_workspace_bytes_cfg workspace + G - 1 per-keyframe parts (0 for G outside [1, SLS_MAX_BATCH]) */
size_t sls_mapping_workspace_bytes_batch(int G, int N, int H, int W, uint64_t R_capacity, const SlsMappingConfig *cfg);
int sls_mapping_step_batch(int G, const SlsKeyframeInputs *keyframes, int N,
                           float *xyz, float *scaling_raw, float *rotation_raw, float *opacity_raw,
                           float *grads, float *exp_avg, float *exp_avg_sq, int64_t adam_step,
                           const SlsMappingConfig *cfg, uint64_t R_capacity, void *workspace, size_t workspace_bytes,
                           SlsMappingStatus *status_dev, void *stream);

/* ---- frame-to-keyframe registration on spherical range images -------
 * The job of the reference's `gsaligner` extension (slam/tracker.py:141-197: set_query /
 * set_reference / align(iguess) -> (T, fitness, _)).  That submodule is not vendored, so the
 * algorithm is this repository's own: projective nearest-pixel association
 * under the spherical model of `projmatrix`, point-to-plane + range-image residuals with Huber
 * weights, Gauss-Newton on SE(3) (left perturbation), the 6x6 system solved on the device.
 *   depth: H*W floats (0 / <= depth_min = invalid), points: H*W*3 floats in the frame's own
 *   coordinates (utils/graphic_utils.py:26-66 with transform_in_world=False), normals: H*W*3.
 *   T_host: row-major 4x4 ref_T_query initial guess (HOST); workspace: DEVICE scratch. */
typedef struct SlsAlignerParams {
    int32_t num_iterations;   /* Gauss-Newton iterations */
    int32_t min_inliers;      /* fewer associated pixels: the pose is left as it is */
    float max_distance;       /* association gate |T p - q| (m) */
    float min_cos_angle;      /* gate on cos(angle between reference normal and viewing ray) */
    float huber_delta;        /* point-to-plane residual (m) */
    float range_weight;       /* weight of the range-image term (0: off) */
    float range_huber;        /* (m) */
    float depth_min, depth_max;
    float damping;            /* added to the diagonal of the normal equations */
} SlsAlignerParams;
typedef struct SlsAlignerResult {
    float pose[12];           /* row-major 3x4 [R|t] of ref_T_query */
    float fitness;            /* associated / valid query pixels at the final pose */
    float chi2;               /* weighted squared error at the final pose */
    float last_step;          /* |xi| of the last update (-1: system was not positive definite) */
    int32_t inliers, valid_query, iterations;
} SlsAlignerResult;
size_t sls_aligner_workspace_bytes(void);
int sls_aligner_normals(const SlsCamera *cam, const float *depth, const float *points, float depth_min,
                        float *normals, void *stream);
/* one linearisation at T_host; sys_out (DEVICE, 32 doubles): H upper triangle (21) | b (6) |
 * chi2 | inliers | valid query pixels | 0 0   (tests compare it with the checker) */
int sls_aligner_linearize(const SlsCamera *cam, const SlsAlignerParams *prm, const float *ref_depth,
                          const float *ref_points, const float *ref_normals, const float *query_depth,
                          const float *query_points, const float *T_host, void *workspace, double *sys_out,
                          void *stream);
/* num_iterations iterations + one evaluation, enqueued without a host sync; result_dev: DEVICE */
int sls_aligner_align(const SlsCamera *cam, const SlsAlignerParams *prm, const float *ref_depth,
                      const float *ref_points, const float *ref_normals, const float *query_depth,
                      const float *query_points, const float *T_host, void *workspace,
                      SlsAlignerResult *result_dev, void *stream);

/* ---- spherical projector (scene/preprocessing.py:42-64, the job of `pyprojections`) ----------
 * A LiDAR scan (n,3) f32 -> the images a keyframe is built from.  Convention (pinned by
 * utils/graphic_utils.py:41-59): pixel (c, r) holds the directions with floor(fx*az + cx + 1) = c,
 * floor(fy*el + cy + 1) = r; a 360-degree image wraps in azimuth; the nearest return wins a pixel.
 * scratch: sls_projector_scratch_bytes(H, W), 8-byte aligned, initialised ONCE by sls_projector_prepare;
 * every later call leaves it ready for the next scan.  Nothing synchronises with the host. */
size_t sls_projector_scratch_bytes(int H, int W);
int sls_projector_prepare(int H, int W, void *scratch, size_t scratch_bytes, void *stream);
/* pyp.calculate_spherical_intrinsics (scene/preprocessing.py:42-44): intrinsics_out = 12 DEVICE floats:
 * K row-major (9), vfov, hfov, 1.0 if the cloud had any point off the origin. */
int sls_projector_intrinsics(int n, const float *cloud, int H, int W, float full_azimuth_threshold_deg,
                             float *intrinsics_out, void *scratch, size_t scratch_bytes, void *stream);
/* pyp.Camera(...).project + the image gathering of scene/preprocessing.py:45-64.  K_dev: 9 DEVICE floats.
 * lut (H*W int32, -1 = empty; may be null), range_image (H*W; 0 where empty), normals_image (H*W*3,
 * -p/|p| , scene/preprocessing.py:112; may be null), valid (H*W bytes).  Points with range outside
 * (depth_min, depth_max] are dropped. */
int sls_projector_project(int n, const float *cloud, const float *K_dev, int H, int W, float depth_min,
                          float depth_max, int32_t *lut, float *range_image, float *normals_image,
                          uint8_t *valid, void *scratch, size_t scratch_bytes, void *stream);

/* ---- fused Adam over up to 8 parameter tensors in one launch ------------
 * torch.optim.Adam semantics (no weight decay, no amsgrad); step is 1-based
 * and shared by all groups. */
typedef struct SlsAdamGroup {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t numel;
    float lr;
    float pad;
} SlsAdamGroup;
int sls_adam_step(const SlsAdamGroup *groups_host, int ngroups, double beta1, double beta2,
                  double eps, int64_t step, void *stream);
/* Same, but the update is skipped on the device when *skip_flag_dev != 0 (the
 * overflow word of SlsMappingStatus, possibly OR-reduced over ranks). */
int sls_adam_step_guarded(const SlsAdamGroup *groups_host, int ngroups, double beta1, double beta2,
                          double eps, int64_t step, const uint32_t *skip_flag_dev, void *stream);
/* Keyframe-parallel form: void_flags_dev points at the two floats SlsMappingConfig.void_flags_out
 * produced, AFTER the SUM all-reduce.  The update is skipped if either is > 0 (some rank voided the
 * iteration), and the reduced bits (bit 0 / bit 1) are stored to status_dev->overflow (status_dev may be
 * null) so that the caller's status read sees the group's verdict; with status_mirror (HOST-visible, as in
 * SlsMappingConfig) the status block is also copied there by this, the iteration's last, kernel. */
int sls_adam_step_reduced(const SlsAdamGroup *groups_host, int ngroups, double beta1, double beta2,
                          double eps, int64_t step, const float *void_flags_dev,
                          struct SlsMappingStatus *status_dev, struct SlsMappingStatus *status_mirror,
                          void *stream);

/* ---- keyframe-parallel exchange of the touched set only -----------------------
 * A keyframe reaches ~10 % of a local model's surfels; only they (and the few the scale regulariser pushes on)
 * carry a non-zero gradient.  Instead of all-reducing the dense 40 B x N bucket:
 *   sls_mapping_step(apply_adam = 0, cfg->grad_bitmap = B)      B: sls_grad_bitmap_words(N) uint64
 *   all-gather(B) -> G bitmaps                                   G x N / 8 bytes (RCCL has no bitwise-OR reduction)
 *   sls_grad_compact(N, bitmaps, G, U, grads, compact, capacity, prefix, status)
 *        U (sls_grad_bitmap_words(N) uint64, out) = OR of the G bitmaps: the union of the touched sets + the verdict;
 *        compact[slot][10] = the gradient of the slot-th surfel of the union, [xyz 3 | opacity | scaling 2 |
 *        rotation 4]; status->exchange_count = K = size of the union; K > capacity sets bit 2 of
 *        status->overflow (void: repeat with more room); status->overflow = the group's verdict
 *   all-reduce(compact[0 .. 10 * K_send), SUM)                   K_send <= capacity chosen by the host
 *        (grads_flat / compact null: the union and its prefix only — sls_grad_union)
 *   sls_adam_step_sparse(...)                                    Adam on every surfel, gradient from its slot or 0;
 *        skipped when the iteration is void; copies the status block to status_mirror (HOST-visible) if given.
 *        `part`: 0 = every surfel in one launch; 1 = only the surfels OUTSIDE the union (their gradient is zero on
 *        every rank: their update needs nothing from the collective, so this launch can run while the rows are being
 *        reduced); 2 = only the union's surfels (after the reduction; mirrors the status) — 1 then 2 give the bits of 0.
 * word_prefix: DEVICE scratch of (N + 63) / 64 uint32. */
/* The form MappingEngine runs (dp_mode "sparse"): the rows never exist as a flat bucket.
 *   sls_mapping_step(apply_adam = 0, grad_bitmap = B, phase = 1)  up to the tile backward; B = the surfels it reached or
 *                                                                 the regulariser may push on (a superset) + the verdict
 *   all-gather(B);  sls_grad_union(N, bitmaps, G, U, capacity, prefix, status)      U, prefix, K, the group's verdict
 *   sls_mapping_step(apply_adam = 1, phase = 2, union_bitmap = U, union_prefix = prefix, grad_compact = compact,
 *                    grad_compact_capacity = capacity)            rows of the union -> their slots; Adam everywhere else
 *   all-reduce(compact[0 .. 10 * K_send), SUM);  sls_adam_step_union(...)           Adam on the union; mirrors the status */
int sls_grad_union(int N, const uint64_t *bitmaps, int n_bitmaps, uint64_t *union_bitmap, uint32_t capacity,
                   uint32_t *word_prefix, struct SlsMappingStatus *status_dev, void *stream);
/* Adam on the union's surfels only, a thread per slot (compact_index[slot] = the surfel; status->exchange_count slots
 * are live); skipped when the iteration is void; copies the status block to status_mirror (HOST-visible) if given. */
int sls_adam_step_union(int N, float *xyz, float *opacity_raw, float *scaling_raw, float *rotation_raw,
                        const uint32_t *compact_index, const float *compact_reduced, uint32_t capacity, float *exp_avg,
                        float *exp_avg_sq, float lr_xyz, float lr_opacity, float lr_scaling, float lr_rotation, double beta1,
                        double beta2, double eps, int64_t step, struct SlsMappingStatus *status_dev,
                        struct SlsMappingStatus *status_mirror, void *stream);
size_t sls_grad_bitmap_words(int N);
int sls_grad_compact(int N, const uint64_t *bitmaps, int n_bitmaps, uint64_t *union_bitmap, const float *grads_flat,
                     float *compact, uint32_t capacity, uint32_t *word_prefix, struct SlsMappingStatus *status_dev,
                     void *stream);
int sls_adam_step_sparse(int N, float *xyz, float *opacity_raw, float *scaling_raw, float *rotation_raw,
                         const uint64_t *union_bitmap, const uint32_t *word_prefix, const float *compact_reduced,
                         float *exp_avg, float *exp_avg_sq, float lr_xyz, float lr_opacity, float lr_scaling,
                         float lr_rotation, double beta1, double beta2, double eps, int64_t step, int part,
                         struct SlsMappingStatus *status_dev, struct SlsMappingStatus *status_mirror, void *stream);

/* ---- simple-knn ---------------------------------------------------------
 * out[i] = mean of squared distances from point i to its 3 nearest other
 * points. */
size_t sls_knn_scratch_bytes(int M);
int sls_knn_dist2(int M, const float *xyz, float *out, void *scratch, size_t scratch_bytes,
                  void *stream);
/* The same for the FIRST M_first points only (out: M_first floats), neighbours searched among all M: what Mapper.densify
 * keeps of `distCUDA2(cat(new, existing))` (slam/mapper.py:109-117 reads `[:n_new]`).  Same values as sls_knn_dist2's
 * first M_first; the search runs only for the waves of the sorted curve that hold a query. */
int sls_knn_dist2_first(int M, int M_first, const float *xyz, float *out, void *scratch, size_t scratch_bytes,
                        void *stream);

/* ---- nearest neighbour between two clouds, distance statistics -------------
 * For every query point the nearest TARGET point (the exact search of sls_knn_dist2's spatial index, queried by a second
 * cloud): with d2(q, t) = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), d* = t.* - q.* in float32 (include/sls_nn_math.h),
 *   out_dist2[q] = min over t of d2(q, t),
 *   out_index[q] = the LOWEST original target index attaining that minimum, bit for bit (optional: may be null),
 * in the caller's query order.  All pointers DEVICE; target_xyz (Mt x 3) and query_xyz (Mq x 3) row-major floats.
 *   scratch: sls_nn_scratch_bytes(Mt, Mq) bytes (0 for Mt < 1 or Mq < 0), 256-byte aligned.
 * Mq == 0 succeeds and writes nothing.  Before anything is enqueued: SLS_E_ARG for Mt < 1, Mq < 0, a null pointer,
 * scratch that is not 256-byte aligned; SLS_E_SCRATCH for too little scratch. */
size_t sls_nn_scratch_bytes(int Mt, int Mq);
int sls_nn_query(int Mt, const float *target_xyz, int Mq, const float *query_xyz, float *out_dist2, int32_t *out_index,
                 void *scratch, size_t scratch_bytes, void *stream);
/* Statistics of M squared distances (sls_nn_query's out_dist2).  tau2 = truncation * truncation in float32; entry i is
 * kept when dist2[i] < tau2 and then contributes d = sqrtf(dist2[i]) (correctly rounded); any other entry contributes
 * d = truncation when include_truncated != 0 and is dropped otherwise.
 *   out_stats (DEVICE, 4 words): [n = contributing entries, n_below = those with d < threshold in float32,
 *       the bits of the double sum of (double)d, M].
 * The sum is taken in a fixed order (per-block partials of a grid that depends on M alone, then one fixed-order pass,
 * no atomics): the same input gives the same bits on every run.  M == 0 writes [0, 0, bits(0.0), 0] (dist2 may be
 * null then).
 *   scratch: SLS_NN_STATS_SCRATCH_BYTES bytes, 256-byte aligned; sls_nn_scratch_bytes(Mt, Mq) is never smaller, so
 *       the query's scratch serves.
 * SLS_E_ARG (M < 0, a null pointer, a NaN truncation or threshold, misaligned scratch) and SLS_E_SCRATCH before
 * anything is enqueued. */
#define SLS_NN_STATS_SCRATCH_BYTES 32768
int sls_nn_stats(int M, const float *dist2, float truncation, float threshold, int include_truncated, uint64_t *out_stats,
                 void *scratch, size_t scratch_bytes, void *stream);

/* ---- exact point-to-mesh distance, error colours ---------------------------------------------------------------------
 * For every query point the nearest TRIANGLE of a mesh (include/sls_meshdist_math.h): with d2(q, f) the header's squared
 * distance of q to face f, float32,
 *   out_dist2[q] = min over f of d2(q, f),
 *   out_face[q] = the LOWEST face index attaining that minimum (optional: may be null),
 *   out_closest[q] (Mq x 3, optional) = the header's closest point of that face, recomputed once from (q, face),
 * in the caller's query order: the values of the header, bit for bit, for (query, returned face).  Unsigned: no inside or
 * outside.  The search is the box sweep of sls_nn_query over an index of triangles whose boxes bound all three vertices;
 * it prunes with a relative slack of 1e-5 on squared gaps, so the float64 distance to the returned face exceeds the true
 * minimum by no more than the header's own rounding error.  All pointers DEVICE; vertices (V x 3)
 * row-major floats, faces (F x 3) int32, query_xyz (Mq x 3).  Queries must be finite: this is not checked, but every
 * access stays inside the buffers.
 *   out_status (4 words): [F, faces with a vertex index outside [0, V), faces with a non-finite vertex, 1].  Such faces
 *       are never dereferenced out of range; when either count is non-zero the other outputs are unspecified.
 *   scratch: sls_mesh_distance_scratch_bytes(V, F, Mq) bytes (0 for V < 1, F < 1 or Mq < 0), 256-byte aligned; a multiple
 *       of 256, monotone, and never below SLS_NN_STATS_SCRATCH_BYTES, so sls_nn_stats can follow on the same scratch.
 * Mq == 0 succeeds and writes only the status (query_xyz and out_dist2 may be null then).  Before anything is enqueued:
 * SLS_E_ARG for V < 1, F < 1, Mq < 0, a null pointer other than the two optional ones, scratch that is not 256-byte
 * aligned; SLS_E_SCRATCH for too little scratch.
 *
 * sls_error_colors: out_rgb[i] (M x 3 bytes) = the header's error colour of dist2[i] at `truncation` — green at 0, yellow
 * at half the truncation, red at or beyond it, blue for a NaN.  SLS_E_ARG for M < 0, a null pointer (M > 0), a
 * truncation that is not finite and > 0.  M == 0 succeeds and writes nothing. */
size_t sls_mesh_distance_scratch_bytes(int V, int F, int Mq);
int sls_mesh_distance(int V, const float *vertices, int F, const int32_t *faces, int Mq, const float *query_xyz,
                      float *out_dist2, int32_t *out_face, float *out_closest, uint32_t *out_status, void *scratch,
                      size_t scratch_bytes, void *stream);
int sls_error_colors(int M, const float *dist2, float truncation, uint8_t *out_rgb, void *stream);

/* ---- first hits of rays on a mesh ---------------------------------------------------------------------------------------
 * For every ray (origin o, direction d, need not be unit) the FIRST triangle it hits (include/sls_raycast_math.h): with
 * hit(r, f) the header's watertight test of ray r against face f within [t_min, t_max], float32,
 *   out_t[r] = the smallest t over the faces hit (the hit point is o + t d), +inf on a miss,
 *   out_face[r] (optional) = the LOWEST face index attaining it, -1 on a miss,
 *   out_uv[r] (Mr x 2, optional) = the barycentric weights of that face's second and third vertex, recomputed once from
 *       (ray, face); 0, 0 on a miss,
 * in the caller's ray order: the values of the header, bit for bit, for (ray, returned face).  Both sides of a face hit.
 * No ray passes between two faces that share an edge or a vertex (the header says why).  The index is sls_mesh_distance's
 * index of triangles, built ONCE by sls_mesh_rayindex_build and cast against any number of times — it is valid for the
 * (V, vertices, F, faces) it was built from, which must be passed again unchanged; that is not checked.
 * All pointers DEVICE; vertices (V x 3) row-major floats, faces (F x 3) int32, origins and directions (Mr x 3).
 *   out_status (4 words): [F, faces with a vertex index outside [0, V), faces with a non-finite vertex, rays refused];
 *       the build writes the first three and 0.  Such faces are never dereferenced out of range and never hit; when either
 *       count is non-zero the other outputs are unspecified.  A refused ray (a non-finite component, or a direction whose
 *       largest |component| is below 2^-100) misses.
 *   index: sls_mesh_rayindex_bytes(V, F) bytes (0 for V < 1 or F < 1), 256-byte aligned.
 * Mr == 0 succeeds and writes only the status (origins, directions and out_t may be null then).  Before anything is
 * enqueued: SLS_E_ARG for V < 1, F < 1, Mr < 0, a null pointer other than the two optional ones, an index that is not
 * 256-byte aligned, t_min NaN or negative, t_max NaN or below t_min; SLS_E_SCRATCH for too small an index. */
size_t sls_mesh_rayindex_bytes(int V, int F);
int sls_mesh_rayindex_build(int V, const float *vertices, int F, const int32_t *faces, void *index, size_t index_bytes,
                            uint32_t *out_status, void *stream);
int sls_mesh_raycast(int V, const float *vertices, int F, const int32_t *faces, const void *index, size_t index_bytes, int Mr,
                     const float *origins, const float *directions, float t_min, float t_max, float *out_t, int32_t *out_face,
                     float *out_uv, uint32_t *out_status, void *stream);

/* ---- the signed distance to a mesh ---------------------------------------------------------------------------------------
 * sls_mesh_distance with a SIGN (include/sls_signdist_math.h): |out_sdist| = sqrtf of the squared distance, out_face and
 * out_closest are the bits sls_mesh_distance gives for the same input; the value is negative iff the query lies behind the
 * angle-weighted pseudo-normal (Baerentzen and Aanaes 2005) of the feature of the returned face that the closest point
 * lies on — out_feature (optional, one byte a query): 0 the face, 1-3 its edge AB, BC, CA, 4-6 its vertex a, b, c.  A point
 * on the surface, or one whose feature has a zero row, gets the non-negative value.  The sign is correct for a closed,
 * consistently oriented mesh and locally for an open oriented one; it is what the faces' orientation says, nothing is
 * repaired.  It is not an inside / outside test by ray parity.
 *
 * sls_mesh_pseudonormals builds the three tables once for a mesh, nothing read back: out_face_normals (F x 3: the unit
 * normals), out_edge_normals (F x 3 x 3: row 3 f + k is the sum of the unit normals of the faces sharing the undirected
 * edge of corner k of face f, in ascending corner id), out_vertex_normals (V x 3: the sum of corner angle x unit normal
 * over the corners at the vertex, in ascending corner id) — float64 sums, each component rounded once to float32; no
 * float atomics: the same bytes on every run.
 *   out_status (8 words): [faces with two equal indices or an index outside [0, V), those of them with an index outside,
 *       faces with a non-finite vertex, zero-area faces, boundary edges (one owner), non-manifold edges (three or more),
 *       edges with two owners that run the same way (inconsistent orientation), 1].  All of these faces have the zero
 *       normal and are never dereferenced out of range.
 *   scratch: sls_mesh_pseudonormals_scratch_bytes(V, F) bytes (0 for sizes out of range), 256-byte aligned.
 * sls_mesh_signed_distance: the tables are those of the (V, vertices, F, faces) passed, which is not checked.
 *   out_status (4 words): those of sls_mesh_distance.  scratch: sls_mesh_signed_distance_scratch_bytes(V, F, Mq).
 *   Mq == 0 succeeds and writes only the status.
 * sls_signed_stats: out_words (4 x uint64) = [n: the entries with |sd| < truncation, those of them with sd < 0, the bits of
 *   the float64 sum of (double)sd over them in the fixed order of sls_nn_stats, M].  scratch: SLS_NN_STATS_SCRATCH_BYTES.
 * sls_signed_error_colors: L = 255 for |sd| >= truncation, else (int)(|sd| / truncation * 256): sd >= 0 gives
 *   (255, 255 - L, 255 - L), white to red; sd < 0 gives (255 - L, 255 - L, 255), white to blue; NaN (0, 0, 0).
 * All pointers DEVICE.  Before anything is enqueued: SLS_E_ARG for sizes out of range, a null pointer other than the
 * optional outputs, a scratch that is not 256-byte aligned, a NaN truncation (stats) or one that is not finite and > 0
 * (colours); SLS_E_SCRATCH for too small a scratch. */
size_t sls_mesh_pseudonormals_scratch_bytes(int V, int F);
int sls_mesh_pseudonormals(int V, const float *vertices, int F, const int32_t *faces, float *out_face_normals,
                           float *out_edge_normals, float *out_vertex_normals, uint32_t *out_status, void *scratch,
                           size_t scratch_bytes, void *stream);
size_t sls_mesh_signed_distance_scratch_bytes(int V, int F, int Mq);
int sls_mesh_signed_distance(int V, const float *vertices, int F, const int32_t *faces, const float *face_normals,
                             const float *edge_normals, const float *vertex_normals, int Mq, const float *query_xyz,
                             float *out_sdist, int32_t *out_face, float *out_closest, uint8_t *out_feature, uint32_t *out_status,
                             void *scratch, size_t scratch_bytes, void *stream);
int sls_signed_stats(int M, const float *sdist, float truncation, uint64_t *out_words, void *scratch, size_t scratch_bytes,
                     void *stream);
int sls_signed_error_colors(int M, const float *sdist, float truncation, uint8_t *out_rgb, void *stream);

/* ---- the k nearest neighbours, outlier removal ---------------------------------------------------------------------
 * sls_nn_query with k answers per query (include/sls_outlier_math.h): query q's list is the min(k, Mt) smallest keys
 * (bits(d2) << 32 | original target index) over ALL targets, ascending — nearer first, then the lower index; a target
 * that is the query's own copy is a target like any other (d2 = 0).  Exact, bit for bit.
 *   out_dist2 [Mq * k] floats, out_index [Mq * k] int32 (row q: its list; slots beyond Mt: +inf and -1),
 *   out_mean [Mq] doubles: (sum in list order of (double)sqrtf(d2_j)) / min(k, Mt).
 * Each of the three may be null and is then skipped.  1 <= k <= SLS_NN_K_MAX.  Where query_xyz == target_xyz and
 * Mq == Mt the cloud's own index serves as the sorted query set.
 *   scratch: sls_nn_k_scratch_bytes(Mt, Mq, k) bytes (0 for Mt < 1, Mq < 0 or k outside [1, SLS_NN_K_MAX]), 256-byte
 *       aligned; never below sls_nn_scratch_bytes(Mt, Mq).
 * Mq == 0 succeeds and writes nothing.  Before anything is enqueued: SLS_E_ARG for Mt < 1, Mq < 0, k out of range, a
 * null target_xyz / query_xyz / scratch, scratch that is not 256-byte aligned; SLS_E_SCRATCH for too little scratch. */
#ifndef SLS_NN_K_MAX
#define SLS_NN_K_MAX 32     /* (include/sls_outlier_math.h defines the same) */
#endif
size_t sls_nn_k_scratch_bytes(int Mt, int Mq, int k);
int sls_nn_query_k(int Mt, const float *target_xyz, int Mq, const float *query_xyz, int k, float *out_dist2, int32_t *out_index,
                   double *out_mean, void *scratch, size_t scratch_bytes, void *stream);
/* Outlier removal of a cloud of M points, one call each, nothing read back inside it (include/sls_outlier_math.h).
 * Statistical — Open3D's remove_statistical_outlier(nb_neighbors = k, std_ratio) as restated there (Open3D is not a
 * dependency): mean_i = out_mean of the cloud's self-query at k, so the point itself is one of its k;
 *   cloud_mean = sum{mean_i > 0} mean_i / M, std = sqrt(sum{mean_i > 0} (mean_i - cloud_mean)^2 / (M - 1)),
 *   thr = cloud_mean + std_ratio * std; point i is kept iff mean_i > 0 && mean_i < thr.
 * So a point whose k - 1 nearest others are exact copies of it is removed, k = 1 removes everything and M = 1 removes
 * the point (thr is NaN).  The sums are float64, in a fixed order, no atomics: the same input, the same bits.
 * Radius — point i is kept iff more than nb_points points, itself included, have d2 <= radius * radius (a float32
 * product): 0 <= nb_points <= SLS_NN_K_MAX - 1.
 *   normals (optional, M x 3): rows that travel with their points into out_normals.
 *   out_xyz, out_normals (M x 3 floats), out_index (M int32: the original row): room for M rows each, the kept rows in
 *       ascending original index, the rows from `kept` on not written.  Each may be null and is then skipped
 *       (out_normals must be null when normals is).
 *   out_status (DEVICE, SLS_OUTLIER_STATUS_WORDS 64-bit words): [kept, points with a mean that is not > 0, bits of
 *       the doubles cloud_mean, std, thr, M, 0, 0]; the radius filter writes [kept, 0, 0, 0, 0, M, 0, 0].
 *   scratch: sls_outlier_scratch_bytes(M, k) bytes, k = nb_points + 1 for the radius filter (0 for M < 1 or k outside
 *       [1, SLS_NN_K_MAX]), 256-byte aligned; never below sls_nn_k_scratch_bytes(M, M, k).
 * M == 0 succeeds, zeroes out_status when that is non-null and touches nothing else.  Before anything is enqueued:
 * SLS_E_ARG for M < 0, k or nb_points out of range, a std_ratio or radius that is not a finite number > 0, a null xyz /
 * out_status / scratch, out_normals without normals, misaligned scratch; SLS_E_SCRATCH for too little scratch. */
#define SLS_OUTLIER_STATUS_WORDS 8
size_t sls_outlier_scratch_bytes(int M, int k);
int sls_outlier_statistical(int M, const float *xyz, const float *normals, int k, double std_ratio, float *out_xyz,
                            float *out_normals, int32_t *out_index, uint64_t *out_status, void *scratch, size_t scratch_bytes,
                            void *stream);
int sls_outlier_radius(int M, const float *xyz, const float *normals, int nb_points, float radius, float *out_xyz,
                       float *out_normals, int32_t *out_index, uint64_t *out_status, void *scratch, size_t scratch_bytes,
                       void *stream);

/* ---- clusters of a cloud ---------------------------------------------------------------------------------------------
 * sls_cloud_dbscan: DBSCAN over exact radius neighbours, with the border rule of Open3D's cluster_dbscan as restated in
 * include/sls_cluster_math.h (Open3D is not a dependency; no parity is claimed).  With r2 = eps * eps (a float32 product)
 * and d2 the expression of sls_nn_query, t is a neighbour of q iff d2 <= r2 — itself and exact copies included; a point
 * is CORE iff at least min_points points are its neighbours; the clusters are the connected components of the cores,
 * numbered in ascending order of their lowest core index; a non-core point with a core neighbour takes the lowest
 * cluster number among its core neighbours' clusters and joins nothing; any other point is noise.  One call, nothing read
 * back inside it; integers and one float32 comparison: the same input gives the same bytes on every run, those of the
 * header's all-pairs routine, on any finite input.  The cost grows with the pairs within eps: eps is meant to be a few
 * point spacings.  Coordinates must be finite (not checked; every access stays inside the buffers).
 *   out_labels [M] int32: the cluster number, -1 for noise.  out_counts [room for M] int32: entries 0 .. C-1, the points
 *       of each cluster, cores and borders; the entries from C on are not written.
 *   out_status (DEVICE, SLS_CLUSTER_STATUS_WORDS words): [C, cores, borders, noise, the largest count, M, 0, 1].
 *   scratch: sls_cloud_dbscan_scratch_bytes(M) bytes (0 for M < 1), 256-byte aligned, a multiple of 256, monotone in M.
 * M == 0 succeeds and writes only out_status.  Before anything is enqueued: SLS_E_ARG for M < 0, an eps that is not a
 * finite number > 0 or whose square is not finite, min_points < 1, a null out_status, for M > 0 a null xyz / out_labels /
 * out_counts / scratch or misaligned scratch; SLS_E_SCRATCH for too little scratch.
 *
 * sls_cloud_select: the rule of sls_mesh_filter over the clusters of a cloud.  C = cluster_status[0] is read on the
 * device; n_min = max(max(min_cluster_points, 0), the min(keep, C)-th largest count), the second term 0 for keep <= 0; a
 * point is kept iff its label is >= 0 and counts[label] >= n_min (ties at the K-th place all stay).  An ordered
 * compaction, as in the outlier filters:
 *   normals (optional, M x 3): rows that travel with their points into out_normals.
 *   out_xyz, out_normals (M x 3 floats), out_index (M int32: the original row): room for M rows each, the kept rows in
 *       ascending original index, the rows from `kept` on not written.  Each may be null and is then skipped
 *       (out_normals must be null when normals is).
 *   out_status (DEVICE, SLS_CLUSTER_SELECT_STATUS_WORDS words): [kept, n_min, M, 1].
 *   scratch: sls_cloud_select_scratch_bytes(M) bytes (0 for M < 1), 256-byte aligned.
 * M == 0 succeeds and writes only out_status.  Before anything is enqueued: SLS_E_ARG for M < 0, a null out_status, for
 * M > 0 a null xyz / labels / counts / cluster_status / scratch, out_normals without normals, misaligned scratch;
 * SLS_E_SCRATCH for too little scratch. */
#ifndef SLS_CLUSTER_STATUS_WORDS
#define SLS_CLUSTER_STATUS_WORDS 8      /* (include/sls_cluster_math.h defines the same) */
#define SLS_CLUSTER_SELECT_STATUS_WORDS 4
#endif
size_t sls_cloud_dbscan_scratch_bytes(int M);
int sls_cloud_dbscan(int M, const float *xyz, float eps, int min_points, int32_t *out_labels, int32_t *out_counts,
                     uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream);
size_t sls_cloud_select_scratch_bytes(int M);
int sls_cloud_select(int M, const float *xyz, const float *normals, const int32_t *labels, const int32_t *counts,
                     const uint32_t *cluster_status, int keep, int min_cluster_points, float *out_xyz, float *out_normals,
                     int32_t *out_index, uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream);

/* ---- normals of a cloud by PCA --------------------------------------------------------------------------------------
 * Open3D's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn = k)) followed by
 * orient_normals_towards_camera_location(viewpoint), restated in include/sls_normals_math.h (Open3D is not a dependency).
 * One call, nothing read back inside it, no float atomics: the cloud's self-query at k writes every point's list into the
 * scratch, one more kernel — a thread per point — takes the prefix of the list with d2 <= radius * radius (a float32
 * product; the point itself is its first entry) as the neighbourhood, n_i points, and from it
 *   n_i >= 3: the float64 mean and covariance in list order, a cyclic Jacobi eigen-solve (+ - * / and sqrt only), the
 *             eigenvector of the smallest eigenvalue, normalised, flipped towards the viewpoint, rounded to float32;
 *   n_i <  3: unit(viewpoint - p), or (0, 0, 1) where that is the zero vector.
 * The same input gives the same bits on every run, and the bits of the header compiled for the host.
 *   k: 1 <= k <= SLS_NORMALS_NN_MAX (beyond SLS_NN_K_MAX the search takes two passes: the 32 nearest, then the k - 32
 *       nearest beyond the 32nd key; only this call reaches them).
 *   radius: finite and > 0, or +inf: the k nearest whatever their distance.
 *   viewpoint3: three floats in HOST memory, read before the call returns.
 *   out_normals [M * 3] floats; out_count [M] int32: n_i; out_eigenvalues [M * 3] floats, ascending, zeros where
 *       n_i < 3.  The last two may be null and are then skipped.
 *   scratch: sls_cloud_normals_scratch_bytes(M, k) bytes (0 for M < 1 or k outside [1, SLS_NORMALS_NN_MAX]), 256-byte
 *       aligned, a multiple of 256, monotone in M and k; never below sls_nn_scratch_bytes(M, M) + 8 * M * k (the rows) + 8 * M.
 *       On return (in stream order) it holds every point's list as sls_nn_query_k writes it: with up(v) = v rounded up to
 *       a multiple of 256, out_dist2 [M * k] floats at byte up(sls_nn_scratch_bytes(M, M)) and out_index [M * k] int32 at
 *       up(4 * M * k) bytes behind that.
 * M == 0 succeeds and touches nothing.  Before anything is enqueued: SLS_E_ARG for M < 0, k out of range, a radius that is
 * NaN or not > 0, a null xyz / viewpoint3 / out_normals / scratch, misaligned scratch; SLS_E_SCRATCH for too little
 * scratch.  Coordinates must be finite (not checked; every access stays inside the buffers). */
#ifndef SLS_NORMALS_NN_MAX
#define SLS_NORMALS_NN_MAX 64   /* (include/sls_normals_math.h defines the same) */
#endif
size_t sls_cloud_normals_scratch_bytes(int M, int k);
int sls_cloud_normals(int M, const float *xyz, int k, float radius, const float *viewpoint3, float *out_normals,
                      int32_t *out_count, float *out_eigenvalues, void *scratch, size_t scratch_bytes, void *stream);

/* ---- the ground of a scan --------------------------------------------------------------------------------------------
 * The reference's `preprocessing.enable_ground_segmentation` ("segment and assign up-facing normals to the ground",
 * scene/preprocessing.py:85-118), which is not implemented there.  A region-wise ground-plane fit in the manner of
 * Patchwork (Lim et al., RA-L 2021) — concentric zones, seeds from the lowest points of every bin, an iterated PCA plane
 * fit, uprightness / elevation / flatness tests — RESTATED from the paper in include/sls_ground_math.h, with sectors cut in
 * the diamond angle (no atan2): patchwork / patchwork++ are not dependencies and no parity with them is claimed; the
 * defaults (sls_ground_defaults there) are a judgement.  One call, nothing read back inside it, no float atomics; the same
 * input gives the same bits on every run, and the bits of the header compiled for the host.
 *   xyz [M * 3] floats, sensor frame, z up.  Rows with a non-finite coordinate are legal: they have no bin.
 *   prm: HOST memory, read before the call returns.
 *   out_label [M] bytes: 1 ground, 0 not.  out_bin [M] int32: the point's bin, -1 for none.
 *   out_planes [SLS_GROUND_BINS * 8] doubles: nx, ny, nz, d, mean_z, the eigenvalues ascending (zeros for a bin without a
 *       fit); nz >= 0.  out_info [SLS_GROUND_BINS * 4] int32: n, seeds, candidates, state (SLS_GROUND_EMPTY ... _GROUND in
 *       the header).  out_bin, out_planes, out_info may be null and are then skipped.
 *   out_status (DEVICE, 8 words): [points with a bin, ground points, non-finite rows, GROUND bins, 0, 0, 0, 1].
 *   scratch: sls_ground_scratch_bytes(M) bytes (0 for M < 1), 256-byte aligned, a multiple of 256, monotone in M.
 * M == 0 succeeds and touches nothing but out_status.  Before anything is enqueued: SLS_E_ARG for M < 0, a null prm /
 * out_status, for M > 0 a null xyz / out_label / scratch or misaligned scratch, a range, height or threshold that is not
 * a finite number > 0, min_range >= max_range, num_iter outside [1, 8], num_lpr < 1, num_min_pts < 3; SLS_E_SCRATCH for
 * too little scratch. */
#define SLS_GROUND_BINS 504     /* (include/sls_ground_math.h defines the same) */
#ifndef SLS_GROUND_PARAMS_DEFINED
#define SLS_GROUND_PARAMS_DEFINED
typedef struct SlsGroundParams {    /* (include/sls_ground_math.h defines the same) */
    float sensor_height, min_range, max_range, th_seeds, th_dist, uprightness_thr, noise_margin, elevation_thr[4],
        flatness_thr[4];
    int32_t num_lpr, num_iter, num_min_pts;
} SlsGroundParams;
#endif
size_t sls_ground_scratch_bytes(int M);
int sls_ground_segment(int M, const float *xyz, const SlsGroundParams *prm, uint8_t *out_label, int32_t *out_bin,
                       double *out_planes, int32_t *out_info, uint32_t *out_status, void *scratch, size_t scratch_bytes,
                       void *stream);

/* ---- registration of two clouds: ICP ---------------------------------------------------------------------------------
 * Gauss-Newton point-to-plane (SLS_ICP_PLANE) or point-to-point (SLS_ICP_POINT) ICP of a source cloud onto a target cloud,
 * on the EXACT nearest neighbours of sls_nn_query with a hard distance gate and no robust weight; the rule — transform,
 * association, the 29 sums and their order, the damped Cholesky solve, the Cayley update, the convergence test — is
 * include/sls_icp_math.h.  It is NOT a global registration: the initial pose must bring the clouds within the gate.  Not
 * Open3D's registration_icp, which is not a dependency; no parity with it is claimed.  One call, nothing read back inside
 * it, no float atomics: the target's index is built once, every pass moves the source by the device-resident pose, sorts
 * it along the target's curve, searches, linearises (a thread per point, fixed-order float64 sums) and solves.  The same
 * input gives the same bits on every run, and the bits of the header compiled for the host.
 *   source_xyz [Ms * 3], target_xyz [Mt * 3], target_normals [Mt * 3] floats (DEVICE); the normals may be null for
 *       SLS_ICP_POINT, which ignores them.
 *   prm (HOST, read before the call returns): method; max_distance: the gate, a finite number > 0; iterations in
 *       [0, 1000]: up to that many updates, then ONE evaluation pass at the final pose (0: one linearisation at the initial
 *       pose); damping: finite, >= 0; eps_rot, eps_trans: finite, >= 0; min_inliers >= 0.  The defaults
 *       (sls_icp_defaults in the header) are a judgement.
 *   init_pose12 (HOST, read before the call returns): 12 finite doubles, the row-major 3 x 4 target_T_source.
 *   out_status (DEVICE, SLS_ICP_STATUS_WORDS 64-bit words): [updates applied, inliers, Ms, Mt, flags (SLS_ICP_FLAG_*), the
 *       bits of the double sum of r^2, the bits of the 12 pose doubles (words 6 .. 17), 2 (the evaluation pass has run), 0].
 *       Inliers and the sum belong to the final pose.  After an update that converged, or a pass that kept the pose (too
 *       few inliers, a system that is not positive definite), the remaining passes change nothing: iterations = 50 on
 *       an input that ends after k updates gives the bits of iterations = k.
 *   out_system (optional, 32 doubles): the 29 sums of the last linearisation (21 upper entries of J^T J row-major, J^T r,
 *       sum r^2, inliers), then three zeros.
 *   out_index [Ms] int32, out_dist2 [Ms] floats (optional): the last association, as sls_nn_query writes it.
 *   scratch: sls_cloud_icp_scratch_bytes(Ms, Mt) bytes (0 for Ms < 0 or Mt < 1), 256-byte aligned, a multiple of 256,
 *       monotone in both, never below sls_nn_scratch_bytes(Mt, Ms).
 * Ms == 0 succeeds: the pose is the initial pose, flags = SLS_ICP_FLAG_FEW, only out_status (and out_system) written.
 * Before anything is enqueued: SLS_E_ARG for a negative size, Mt < 1, a null source_xyz (Ms > 0) / target_xyz / prm /
 * init_pose12 / out_status / scratch, normals missing for the plane method, an unknown method, a max_distance that is not
 * a finite number > 0, a damping / eps_rot / eps_trans that is NaN, negative or infinite, a negative min_inliers,
 * iterations outside [0, 1000], a pose entry that is not finite, misaligned scratch; SLS_E_SCRATCH for too little scratch.
 * Coordinates and normals must be finite (not checked; every access stays inside the buffers). */
#define SLS_ICP_PLANE 0
#define SLS_ICP_POINT 1
#define SLS_ICP_STATUS_WORDS 20
#define SLS_ICP_MAX_ITERATIONS 1000
#ifndef SLS_ICP_FLAG_CONVERGED
#define SLS_ICP_FLAG_CONVERGED 1    /* (include/sls_icp_math.h defines the same) */
#define SLS_ICP_FLAG_FEW 2
#define SLS_ICP_FLAG_NOT_PD 4
#endif
#ifndef SLS_ICP_PARAMS_DEFINED
#define SLS_ICP_PARAMS_DEFINED
typedef struct SlsIcpParams {       /* (include/sls_icp_math.h defines the same) */
    int32_t method, iterations, min_inliers;
    float max_distance;
    double damping, eps_rot, eps_trans;
} SlsIcpParams;
#endif
size_t sls_cloud_icp_scratch_bytes(int Ms, int Mt);
int sls_cloud_icp(int Ms, const float *source_xyz, int Mt, const float *target_xyz, const float *target_normals,
                  const SlsIcpParams *prm, const double *init_pose12, uint64_t *out_status, double *out_system,
                  int32_t *out_index, float *out_dist2, void *scratch, size_t scratch_bytes, void *stream);

/* ---- voxel down-sampling and mesh sampling (what evaluate_recon does before its metric block) -----------------------
 * Open3D's voxel_down_sample for points only, restated (include/sls_cloud_math.h): every point gets the voxel
 * (ix, iy, iz), i_a = floor(((double)p_a - o_a) / voxel_size), o_a = (double)min_a - 0.5 * voxel_size, packed into the
 * key ix | iy << 21 | iz << 42.  Output row v is the voxel with the v-th smallest key (Open3D's hash-map order is
 * unspecified; this is the order this project defines): out_xyz[v] = (float)(float64 sum of the voxel's points / count),
 * out_count[v] = the number of its points (optional: may be null).  Both have room for M rows; the rows from n_voxels on
 * are not written.  The sum of a voxel adds its points in ascending input index — one lane for a voxel of at most 64
 * points, 64 lanes (lane l the points l, l + 64, ... of that order, then a fixed butterfly) beyond — no floating-point
 * atomics: the same input gives the same bits on every run.
 *   out_status (DEVICE, 4 words): [n_voxels, points with a non-finite coordinate, points with an index >= 2^21, 0].
 *       Where either error count is not 0 the output rows are unspecified (every access stays inside the buffers); the
 *       call still returns SLS_OK and the caller decides after its read.
 *   scratch: sls_voxel_scratch_bytes(M) bytes (0 for M < 1), 256-byte aligned; never below sls_sort_scratch_bytes(M).
 * M == 0 succeeds, writes four zeros to out_status when that is non-null and touches nothing else.  Before anything is
 * enqueued: SLS_E_ARG for M < 0, a null pointer, a voxel_size that is not finite or not > 0, misaligned scratch;
 * SLS_E_SCRATCH for too little scratch. */
size_t sls_voxel_scratch_bytes(int M);
int sls_voxel_downsample(int M, const float *xyz, double voxel_size, float *out_xyz, int32_t *out_count,
                         uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream);

/* Area-weighted uniform sampling of a triangle mesh, seeded: Open3D's sample_points_uniformly with a defined random
 * stream — sample i is a pure function of (mesh, crop box, seed, i), include/sls_cloud_math.h states every step.
 *   vertices (V x 3 floats), faces (F x 3 int32), crop_box (optional: 6 DEVICE floats, min xyz then max xyz).
 *   A face has weight 0 when an index is outside [0, V) (counted in out_status[1]), when its float64 area is not
 *   finite, or when a crop box is given and one of its vertices lies outside the closed box (Open3D's crop keeps a
 *   triangle when all its vertices are kept).  Otherwise w = floor(area / largest area * 2^32): the prefix sum is an
 *   integer, exact in any order; faces below 2^-32 of the largest one are never drawn.
 *   out_xyz (n_samples x 3), out_face (optional, n_samples int32): the points and the face each was drawn from.
 *   out_status (DEVICE, 4 words): [rows written: n_samples, or 0 when no face has weight (nothing else is written
 *       then), faces with an index outside [0, V), 1 when no face has weight, 0].
 *   scratch: sls_mesh_sample_scratch_bytes(V, F, n_samples) bytes (0 for a negative argument), 256-byte aligned.
 * n_samples == 0 succeeds, writes four zeros to out_status when that is non-null and touches nothing else.  Before
 * anything is enqueued: SLS_E_ARG for a negative size, a null pointer (crop_box and out_face may be null; vertices
 * with V == 0 and faces with F == 0 too), misaligned scratch; SLS_E_SCRATCH for too little scratch. */
size_t sls_mesh_sample_scratch_bytes(int V, int F, int n_samples);
int sls_mesh_sample(int V, const float *vertices, int F, const int32_t *faces, const float *crop_box, int n_samples,
                    uint64_t seed, float *out_xyz, int32_t *out_face, uint32_t *out_status, void *scratch,
                    size_t scratch_bytes, void *stream);

/* ---- a sparse TSDF volume: from rendered keyframes to a triangle mesh ------------------------------------------------
 * include/sls_tsdf_math.h states every rule; DESIGN.md section 2, "TSDF volume".  A block is 8 x 8 x 8 voxels of edge
 * voxel_size; block b (int32 x 3, every |b_a| < 2^20) covers origin + 8 voxel_size [b, b + 1); voxel
 * l = x | y << 3 | z << 6 of block k lives at slot 512 k + l of the float32 arrays tsdf (normalised, in [-1, 1]) and
 * weight.  The block list is kept in ascending order of kx | ky << 21 | kz << 42, k_a = b_a + 2^20.  origin3: three
 * doubles on the HOST.  All three operations require voxel_size and trunc finite and > 0 and
 * trunc + voxel_size <= 8 voxel_size.
 *
 * The blocks a point set names: for each of the M DEVICE points p every block the box [p - m, p + m] touches,
 * m = trunc + voxel_size (at most three per axis); the unique ones in ascending key order as out_blocks (room for
 * `capacity` rows of three int32: 27 M always suffices; rows from `capacity` on are not written, out_status[0] still
 * counts them).
 *   out_status (DEVICE, 4 words): [B, points with a non-finite coordinate, points with a block index outside
 *       (-2^20, 2^20), 1]; a counted point names no block.
 *   scratch: sls_tsdf_blocks_scratch_bytes(M) bytes (0 for M < 1 or M > SLS_TSDF_MAX_POINTS), 256-byte aligned.
 * Keys, sort, head scan and compaction run in a fixed order (no floating-point atomics, no hash table): the same cloud
 * gives the same array on every run.  M == 0 succeeds, writes [0, 0, 0, 1] to out_status when that is non-null and
 * touches nothing else.  Before anything is enqueued: SLS_E_ARG for M < 0 or > SLS_TSDF_MAX_POINTS, a negative capacity,
 * a null pointer, a bad voxel_size / trunc, misaligned scratch; SLS_E_SCRATCH for too little scratch. */
#define SLS_TSDF_MAX_POINTS 67108864    /* 2^26: 27 candidate keys per point are sorted under 32-bit positions */
#define SLS_TSDF_MAX_BLOCKS 524288      /* 2^19: a 2 GB volume; the triangle count stays below 2^32 */
size_t sls_tsdf_blocks_scratch_bytes(int M);
int sls_tsdf_blocks(int M, const float *xyz, double voxel_size, double trunc, const double *origin3, int capacity,
                    int32_t *out_blocks, uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream);

/* One keyframe into the volume: one launch, no scratch, nothing read back.  allmap: the full seven planes of a
 * rasterizer forward at cam->H x cam->W (planes 0, 1, 5, 6 are read); cam: Rvw / tvw map the VOLUME's frame to the view
 * frame, fx, fy, cx, cy, wrap and near_cut as the forward had them (pix_offset is not read: the pixel of a voxel is
 * floor(fx az + cx + 1), floor(fy el + cy + 1), the inverse of the half-pixel back-projection of sls_surface_samples).
 * Per voxel, nearest pixel: valid iff !(alpha < min_opacity) && !(dist > max_depth_dist);
 * depth = (1 - depth_ratio) D / alpha + depth_ratio median; sdf = depth - |q|; skipped below -trunc;
 * tsdf <- (tsdf weight + min(1, sdf / trunc)) / (weight + 1), weight <- weight + 1.  Every voxel is owned by one thread
 * and keyframes are ordered by the stream: the result is bit-reproducible and equals the header run on the host.
 * B == 0 succeeds.  SLS_E_ARG before the launch: a null pointer, B < 0 or > SLS_TSDF_MAX_BLOCKS, a camera without
 * pixels, a NaN threshold or depth_ratio, a bad voxel_size / trunc. */
int sls_tsdf_integrate(const SlsCamera *cam, int B, const int32_t *blocks, float *tsdf, float *weight, const float *allmap,
                       double voxel_size, double trunc, const double *origin3, float min_opacity, float max_depth_dist,
                       float depth_ratio, void *stream);

/* The zero surface as a triangle soup, marching tetrahedra over the Freudenthal split of every cube all of whose eight
 * corners exist (a corner in an absent +x/+y/+z neighbour block does not) with weight >= min_weight.  Order: ascending
 * block, ascending cube l, tetrahedron 0..5, triangle 0..1; normals point to the positive (free-space) side.
 * Two calls.  count: counts[k] = the triangles of block k, prefix[k] = their exclusive prefix (B words each, DEVICE),
 * out_status (DEVICE, 4 words) = [T, B, 0, 1]; the caller reads T and allocates.  emit: triangles (T x 3 x 3 floats)
 * with every triangle at its prefixed position (in-workgroup scans, no atomics); T is the count call's total and
 * nothing is written past it.  B == 0 succeeds (count writes [0, 0, 0, 1]); emit with T == 0 succeeds and launches
 * nothing.  SLS_E_ARG before a launch: B < 0 or > SLS_TSDF_MAX_BLOCKS, a null pointer, a NaN min_weight, a bad
 * voxel_size. */
int sls_tsdf_extract_count(int B, const int32_t *blocks, const float *tsdf, const float *weight, float min_weight,
                           uint32_t *counts, uint32_t *prefix, uint32_t *out_status, void *stream);
int sls_tsdf_extract_emit(int B, const int32_t *blocks, const float *tsdf, const float *weight, float min_weight,
                          double voxel_size, const double *origin3, const uint32_t *prefix, uint32_t T, float *triangles_out,
                          void *stream);

/* ---- screened Poisson reconstruction over the block volume ----------------------------------------------------------
 * include/sls_poisson_math.h states every rule and every order of summation; DESIGN.md section 2, "Poisson volume".  The
 * grid is the TSDF volume's: blocks (B x 3 int32, DEVICE) in ascending key order, voxel l of block k at slot 512 k + l.
 * It IS a least-squares fit of the gradient of an indicator to the splatted normal field on a uniform band, screened by
 * the sample density, solved by Jacobi-preconditioned conjugate gradients.  It is NOT Kazhdan's adaptive octree, uses
 * trilinear splats (not B-splines), has no Dirichlet envelope and is not compared against Open3D, which is not a
 * dependency.  Every result equals the header run on the host bit for bit; no floating-point atomics.
 *
 * splat: the M DEVICE points (xyz, normals: M x 3 floats each) into out_field (B x 512 x 4 floats: Vx, Vy, Vz, W).
 *   out_status (DEVICE, 4 words): [points with a non-finite value, points out of index range, points with at least one
 *   dropped corner (a point whose cell lies in no block is dropped whole and counted here), 1].
 *   scratch: sls_poisson_splat_scratch_bytes(M, B) bytes (0 for M < 1 or sizes beyond the limits).  M == 0 succeeds,
 *   writes [0, 0, 0, 1] to out_status when that is non-null and touches nothing else; B == 0 counts and writes no field.
 * solve: (L + alpha diag(W)) x = b from x = 0, at most `iterations` passes, ended when <r,r> <= tol^2 <b,b>; out_chi
 *   (B x 512 floats) = x - iso, iso the W-weighted mean of x.  out_status (DEVICE, SLS_POISSON_STATUS_WORDS 64-bit
 *   words): [passes run, flags (SLS_POISSON_FLAG_*), B, the bits of the doubles <r,r>, <b,b>, iso, sum W, 0].  Nothing
 *   is read back and nothing synchronises inside the call; once ended the remaining passes change nothing.
 *   scratch: sls_poisson_solve_scratch_bytes(B).  B == 0 succeeds: [0, CONVERGED | EMPTY, 0, ...].
 * density: W after `sweeps` averaging sweeps over the present neighbours, as out_density (B x 512 floats).
 *   scratch: sls_poisson_density_scratch_bytes(B).  B == 0 succeeds and writes nothing.
 * Before anything is enqueued: SLS_E_ARG for a null pointer, M or B negative or above SLS_TSDF_MAX_POINTS /
 * SLS_TSDF_MAX_BLOCKS, a voxel_size that is not finite and > 0, an origin that is not finite, alpha not finite and > 0,
 * tol NaN, negative or infinite, iterations outside [0, SLS_POISSON_MAX_ITERATIONS], sweeps outside
 * [0, SLS_POISSON_MAX_SWEEPS], misaligned scratch; SLS_E_SCRATCH for too little scratch. */
#define SLS_POISSON_MAX_ITERATIONS 1000
#define SLS_POISSON_MAX_SWEEPS 64
#ifndef SLS_POISSON_FLAG_CONVERGED
#define SLS_POISSON_FLAG_CONVERGED 1    /* (include/sls_poisson_math.h defines the same, and refuses to compile after other values) */
#define SLS_POISSON_FLAG_NOT_PD 2
#define SLS_POISSON_FLAG_EMPTY 4
#define SLS_POISSON_STATUS_WORDS 8
#endif
size_t sls_poisson_splat_scratch_bytes(int M, int B);
int sls_poisson_splat(int M, const float *xyz, const float *normals, int B, const int32_t *blocks, double voxel_size,
                      const double *origin3, float *out_field, uint32_t *out_status, void *scratch, size_t scratch_bytes,
                      void *stream);
size_t sls_poisson_solve_scratch_bytes(int B);
int sls_poisson_solve(int B, const int32_t *blocks, const float *field, double alpha, int iterations, double tol,
                      float *out_chi, uint64_t *out_status, void *scratch, size_t scratch_bytes, void *stream);
size_t sls_poisson_density_scratch_bytes(int B);
int sls_poisson_density(int B, const int32_t *blocks, const float *field, int sweeps, float *out_density, void *scratch,
                        size_t scratch_bytes, void *stream);

/* ---- cleaning an extracted mesh: weld, clusters, selection, vertex normals ------------------------------------------
 * include/sls_mesh_math.h states every rule; DESIGN.md section 2, "Mesh cleaning".  Every pointer is a DEVICE pointer;
 * every scratch is 256-byte aligned and its size comes from the matching _scratch_bytes (0 for a size below 1 or above
 * the limits).  A last status word of 1 means "written".  Outputs beyond the written count are left
 * untouched.  Before anything is enqueued: SLS_E_ARG for a negative size, a size above the limits, a null pointer,
 * misaligned scratch; SLS_E_SCRATCH for too little scratch.  A size of 0 succeeds and writes only the status words (when
 * out_status is non-null).  No floating-point atomics anywhere: the same input gives the same bytes on every run.
 *
 * SLS_MESH_MAX_TRIANGLES: 3 T + 2, the largest edge / corner id, fits the sorter's u32 value and every row, vertex and
 * triangle index fits int32. */
#define SLS_MESH_MAX_TRIANGLES 536870912     /* 2^29 */
#define SLS_MESH_MAX_VERTICES 1610612736     /* 3 x 2^29 */

/* Weld: soup, n_rows x 3 float32 (n_rows <= 3 SLS_MESH_MAX_TRIANGLES).  Two rows are the same vertex iff their three words
 * are equal as integers.  out_vertices (room for n_rows rows): the V unique rows in ascending lexicographic order of
 * (x, y, z) as signed int32; out_index[r] (n_rows int32): the rank of row r; out_status (4 words) = [V, 0, 0, 1]. */
size_t sls_mesh_weld_scratch_bytes(int n_rows);
int sls_mesh_weld(int n_rows, const float *soup, float *out_vertices, int32_t *out_index, uint32_t *out_status, void *scratch,
                  size_t scratch_bytes, void *stream);

/* Clusters: faces, T x 3 int32 over V vertices (0 <= V <= SLS_MESH_MAX_VERTICES).  A triangle with two equal indices or an
 * index outside [0, V) is degenerate: out_labels[t] = -1.  Non-degenerate triangles that share an undirected edge are
 * joined; out_labels[t] (T int32) is the cluster of triangle t, clusters numbered in ascending order of their lowest
 * triangle; out_counts[c] (room for T int32) the triangles of cluster c < C.
 *   out_status (6 words) = [C, degenerate triangles (both kinds), those of them with an index outside [0, V), edges with
 *   exactly one triangle, edges with more than two, 1]. */
size_t sls_mesh_clusters_scratch_bytes(int T);
int sls_mesh_clusters(int T, const int32_t *faces, int V, int32_t *out_labels, int32_t *out_counts, uint32_t *out_status,
                      void *scratch, size_t scratch_bytes, void *stream);

/* Selection: labels / counts / cluster_status as sls_mesh_clusters wrote them for these faces (C is read from
 * cluster_status[0] on the device).  n_min = max(max(min_triangles, 0), the min(keep_clusters, C)-th largest count; 0 for
 * keep_clusters <= 0); a triangle is kept iff its label is >= 0 and counts[label] >= n_min.  out_faces (room for T rows):
 * the kept triangles in input order, re-indexed; out_vertices (room for V rows): the vertices they reference, in input
 * order; out_vmap (V int32, may be null): the new index of every vertex, -1 for one that left.
 *   out_status (4 words) = [V', T', n_min, 1].  V == 0 or T == 0 writes [0, 0, max(min_triangles, 0), 1] alone. */
size_t sls_mesh_filter_scratch_bytes(int V, int T);
int sls_mesh_filter(int V, const float *vertices, int T, const int32_t *faces, const int32_t *labels, const int32_t *counts,
                    const uint32_t *cluster_status, int keep_clusters, int min_triangles, float *out_vertices,
                    int32_t *out_faces, int32_t *out_vmap, uint32_t *out_status, void *scratch, size_t scratch_bytes,
                    void *stream);

/* Vertex normals: out_normals[v] (V x 3 float32) = the normalised sum, in ascending triangle index, of
 * (p1 - p0) x (p2 - p0) over the non-degenerate triangles that reference v; zeros for a vertex without one or with a sum
 * of zero or non-finite length.  Equals the header run on the host bit for bit.  Nothing is read back; V == 0 succeeds
 * and writes nothing, T == 0 writes zeros. */
size_t sls_mesh_vertex_normals_scratch_bytes(int V, int T);
int sls_mesh_vertex_normals(int V, const float *vertices, int T, const int32_t *faces, float *out_normals, void *scratch,
                            size_t scratch_bytes, void *stream);

/* Simplification by vertex clustering (include/sls_simplify_math.h states every rule; DESIGN.md section 2, "Mesh
 * simplification").  The live vertices (those a non-degenerate triangle references) of one voxel of edge voxel_size become
 * one vertex: their float64 mean (contraction 0) or the minimum of the voxel's error quadric, regularised towards that
 * mean by `regularisation` times the quadric's trace (contraction 1).  Triangles are mapped to clusters, dropped when they
 * collapse, rotated so that their smallest index comes first and de-duplicated (the lowest input index stays); kept
 * triangles stay in input order, the surviving clusters leave in ascending voxel key.  out_vertices (room for V rows),
 * out_faces (room for T rows), out_vmap (V int32, may be null): the output vertex of every input vertex, -1 for one that
 * left.  The conventions of the mesh cleaning calls apply; additionally SLS_E_ARG for a voxel_size that is not finite and
 * > 0, a contraction other than 0 or 1, a regularisation that is not finite and >= 0.  Face rows of -1 and unreferenced
 * vertex rows take no part: the call runs behind sls_mesh_filter at capacity.  Equals the header run on the host bit for
 * bit.
 *   out_status (8 words) = [V', T', live vertices with a non-finite coordinate, live vertices with a voxel index >= 2^21
 *   (not 0: the outputs are unspecified), collapsed triangles, duplicate triangles, quadric fallbacks to the mean, 1].
 *   V == 0 or T == 0 writes [0, 0, 0, 0, 0, 0, 0, 1] and out_vmap = -1 alone. */
size_t sls_mesh_simplify_scratch_bytes(int V, int T);
int sls_mesh_simplify(int V, const float *vertices, int T, const int32_t *faces, double voxel_size, int contraction,
                      double regularisation, float *out_vertices, int32_t *out_faces, int32_t *out_vmap, uint32_t *out_status,
                      void *scratch, size_t scratch_bytes, void *stream);

/* The edge graph of a mesh and smoothing over it (include/sls_smooth_math.h states every rule; DESIGN.md section 2, "Mesh
 * smoothing").  sls_mesh_adjacency: the DISTINCT neighbours of every vertex in ascending index, in CSR form — out_offsets
 * (V + 1 words; unsigned 32-bit values, which pass 2^31 only for T above 357 913 941), out_neighbours (room for 6 T int32,
 * the first 2 E written, E = the distinct undirected edges), out_boundary[v] = 1 iff v is an end of an edge that exactly one
 * non-degenerate triangle owns.  Degenerate triangles (sls_mesh_degenerate; rows of -1 too) take no part: the calls run
 * behind sls_mesh_filter and sls_mesh_simplify at capacity.
 * sls_mesh_smooth: `iterations` sweeps of method 0 (simple: Open3D's filter_smooth_simple), 1 (laplacian: steps of factor
 * lambda) or 2 (taubin: a step of factor lambda, then one of factor mu, per iteration) with weights 0 (uniform) or 1
 * (inverse distance); a vertex without a neighbour, and with fix_boundary a boundary vertex, is copied bit for bit.  The
 * adjacency is built inside the scratch, the sweeps ping-pong between two float4 buffers of the scratch and the last one
 * writes out_vertices (V x 3; iterations == 0 copies `vertices`); nothing is read back.  Every sum is float64 in a fixed
 * order: equal to the header run on the host bit for bit.  The conventions of the mesh cleaning calls apply; additionally
 * SLS_E_ARG for out_vertices == vertices, a negative `iterations`, an unknown method or weights, a lambda or mu that is not
 * finite.
 *   out_status (8 words) = [live vertices (those with a neighbour), E, boundary vertices, live vertices with a non-finite
 *   coordinate (sls_mesh_smooth alone; not 0: out_vertices is unspecified), degenerate triangles (both kinds), those of
 *   them with an index outside [0, V), the largest number of neighbours of a vertex, 1].
 *   V == 0 or T == 0 writes [0, 0, 0, 0, 0, 0, 0, 1]; out_offsets and out_boundary are zeros, out_vertices = vertices. */
size_t sls_mesh_adjacency_scratch_bytes(int V, int T);
int sls_mesh_adjacency(int V, int T, const int32_t *faces, int32_t *out_offsets, int32_t *out_neighbours, uint8_t *out_boundary,
                       uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream);
size_t sls_mesh_smooth_scratch_bytes(int V, int T);
int sls_mesh_smooth(int V, const float *vertices, int T, const int32_t *faces, int method, int weights, int iterations, double lambda,
                    double mu, int fix_boundary, float *out_vertices, uint32_t *out_status, void *scratch, size_t scratch_bytes,
                    void *stream);

/* Hole filling (include/sls_fill_math.h states every rule; DESIGN.md section 2, "Mesh hole filling").  Both calls take the
 * mesh at capacity — V vertex rows, T face rows — and optionally in_counts, two device words [V_live, T_live] (each clamped
 * to its capacity; null: V and T): rows beyond them are ignored, which lets the calls run behind sls_mesh_filter without a
 * host read.  Degeneracy is judged against V_live.
 * sls_mesh_boundary_loops: out_halfedges (room for 3 T pairs of int32): the B boundary half-edges (a, b) in ascending
 * (a, b); out_loop (room for 3 T int32): the loop of every half-edge, -1 for an open one; out_loop_edges (room for T
 * int32): the half-edges of every loop.  Loops are numbered in ascending order of their lowest vertex.
 * sls_mesh_fill_holes: every loop of at most max_edges half-edges, with finite vertices and (max_size > 0) a bounding-box
 * diagonal of at most max_size, is closed — a loop of three by one triangle, a longer one by a fan over its float64
 * centroid.  out_vertices (cap_vertices x 3): the V_live rows, then the new vertices; out_faces (cap_triangles x 3): the
 * T_live rows, then the new triangles, then rows of -1.  Where the needed rows exceed either capacity nothing is filled:
 * the outputs are the live input, and status word 14 is 1.  Every sum is float64 in a fixed order: equal to the header run
 * on the host bit for bit.  The conventions of the mesh cleaning calls apply; additionally SLS_E_ARG for max_edges < 3, a
 * max_size that is not finite and >= 0, cap_vertices < V or cap_triangles < T, a capacity above the SLS_MESH_MAX_* limits,
 * out_vertices == vertices or out_faces == faces.
 *   out_status (16 words) = [V', T', B, loops, filled loops, loops skipped for max_edges, for max_size, for a non-finite
 *   vertex, open half-edges, complex vertices, degenerate live triangles (both kinds), those of them with an index outside
 *   the live vertices, needed vertices, needed triangles, overflow, 1]; sls_mesh_boundary_loops leaves words 0, 1, 4 to 7
 *   and 12 to 14 at 0.  V == 0 or T == 0: no half-edge; words 10 and 11 are T_live where V == 0; the fill copies the live
 *   rows and pads the faces. */
size_t sls_mesh_boundary_loops_scratch_bytes(int V, int T);
int sls_mesh_boundary_loops(int V, int T, const int32_t *faces, const uint32_t *in_counts, int32_t *out_halfedges, int32_t *out_loop,
                            int32_t *out_loop_edges, uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream);
size_t sls_mesh_fill_holes_scratch_bytes(int V, int T);
int sls_mesh_fill_holes(int V, const float *vertices, int T, const int32_t *faces, const uint32_t *in_counts, int max_edges,
                        double max_size, int cap_vertices, float *out_vertices, int cap_triangles, int32_t *out_faces,
                        uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream);

/* visible[i] = 1 if surfel centre i survives the near cut (radii would be >0
 * unless it is off-image). */
int sls_mark_visible(const SlsCamera *cam, int N, const float *means3D, uint8_t *visible,
                     void *stream);

/* Optional per-kernel timing with HIP events recorded on the launch stream
 * (bench.py's roofline figures).  sls_timing_collect synchronises on the
 * recorded events, fills total_ms[slot] / counts[slot] for slot <
 * sls_timing_slots() and resets the recorder; returns 1 if the event pool ran
 * out (later launches untimed). */
int sls_timing_slots(void);
const char *sls_timing_name(int slot);
int sls_timing_enable(int mode);   /* 0 off, 1 every launch, 2 the two tile kernels only, 3 render_bwd only,
                                    * 4 every 8th render_bwd launch (a timed region that keeps its own clock) */
int sls_timing_collect(double *total_ms_host, int64_t *counts_host);

/* Diagnostic: when non-null, the tile kernels write the shader-clock cycles each
 * wave spent (T * waves_per_tile uint32 each, DEVICE pointers) — used to look at
 * load balance across tiles.  Pass nulls to switch it off (the default). */
int sls_debug_wave_cycles(uint32_t *fwd_cycles, uint32_t *bwd_cycles);

/* Kept for binary compatibility: the tile kernels' pixel-block shape, forward and backward.  3 (8x2 blocks) is the
 * only one; it and negative values are accepted and change nothing, anything else (2, the removed 4x4 blocks,
 * included) returns SLS_E_ARG.  Sets no state. */
int sls_debug_variant(int fwd, int bwd);

/* Device self-test of the wave64 primitives (DPP reduction, ballot ranking).
 * Returns 0 if they behave as the kernels assume.  Synchronises. */
int sls_selftest(void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SLS_ABI_H */

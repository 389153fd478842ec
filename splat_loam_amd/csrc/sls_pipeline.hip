// sls_pipeline.hip — host-side orchestration behind the C-ABI: the two-stage
// forward and the backward of the drop-in rasterizer interface, and
// sls_mapping_step, which enqueues one WHOLE mapping iteration
// (slam/mapper.py:150-204: render -> loss -> backward -> Adam) on a stream with
// no device->host sync and no torch op in between.
#include <stdlib.h>
#include <string.h>

#include "sls_consumer_dev.hpp"
#include "sls_bin.hpp"

namespace sls {

// launchers implemented in the other translation units
int launch_preprocess_fwd(const DevCam &cam, int raw, float smax, float pen, float *reg_out, int N,
                          const float *means, const float *scales, const float *rots, const float *opac, float *rec,
                          int32_t *radii, int32_t *rect, uint32_t *tiles, float *depth, uint32_t *order_keys,
                          uint32_t *order_vals, uint32_t *n_dev, hipStream_t st, uint32_t *status_clear = nullptr,
                          const float *col_cs = nullptr, const float *row_cs = nullptr, uint64_t *tile_mask = nullptr,
                          int32_t *erec = nullptr, const uint32_t *resort_prev_order = nullptr,
                          uint64_t *resort_comp = nullptr, uint32_t *sbox = nullptr, int erec_box = 0,
                          uint32_t *zero_words = nullptr, int n_zero_words = 0);
uint64_t *resort_comp_buffer(int N, void *scratch);
void depth_order_key_buffers(int N, void *scratch, uint32_t *order, uint32_t **keys, uint32_t **vals0,
                             uint32_t **n_dev);
int launch_preprocess_bwd(const DevCam &cam, int raw, float smax, float pen, int N, const float *means,
                          const float *scales, const float *rots, const float *opac, const int32_t *radii,
                          const float *grec, float *dmeans, float *dscales, float *drots, float *dopac,
                          hipStream_t st, const AdamFuse *fuse = nullptr, const PoseOut *pose = nullptr);
int launch_preprocess_bwd_batch(float smax, float pen, int N, float *means, float *scales, float *rots, float *opac,
                                float *dmeans, float *dscales, float *drots, float *dopac, const BatchFuse &bf,
                                hipStream_t st, const PoseOut *pose = nullptr);
size_t sort_scratch_bytes(uint64_t cap);
size_t order_scratch_bytes(int N);
int launch_bin_sort(const DevCam &cam, int N, const uint32_t *count_ptr, uint32_t cap, const uint32_t *order,
                    const int32_t *rect, const uint32_t *tiles, const uint64_t *tile_mask, const int32_t *erec,
                    const float *depth, const uint32_t *offsets,
                    uint32_t *tkeys, uint32_t *vals, uint32_t *tkeys_tmp, uint32_t *vals_tmp, void *scratch,
                    size_t scratch_bytes, int *sorted_in_tmp, uint32_t *ranges, uint64_t *keys64_out,
                    uint32_t *overflow, hipStream_t st, const ScanHandoff *handoff = nullptr,
                    uint32_t *total_out = nullptr, const uint32_t *sbox = nullptr, const uint2 **bmask_out = nullptr,
                    int bmask_mode = 0);
int launch_render_fwd(const DevCam &, const uint32_t *, const uint32_t *, const float *, const float *,
                      const float *, float *, float *, uint32_t *, uint32_t *, hipStream_t, bool consumed_zeroed = false,
                      uint64_t *block_masks = nullptr, bool no_median_dist = false, uint32_t *block_cost = nullptr,
                      const uint2 *bmask = nullptr, bool order_in_handover = false);
int launch_render_bwd(const DevCam &, const uint32_t *, const uint32_t *, const float *, const float *,
                      const float *, const float *, const uint32_t *, const float *, float *, hipStream_t,
                      const uint64_t *block_masks = nullptr, bool no_median_dist_grad = false,
                      uint8_t *touched = nullptr, const struct ConsumerArgs *fused_consumer = nullptr,
                      uint32_t *det_max = nullptr, unsigned long long *det_acc = nullptr,
                      const uint32_t *block_order = nullptr, int vals_stride = 1, int block_masks_shape = -1,
                      bool order_in_handover = false, const uint8_t *det_prev = nullptr, const uint32_t *det_gex = nullptr,
                      uint32_t *det_flag = nullptr, bool consumer_b_inline = false, uint32_t order_tag = 0u);
size_t block_mask_bytes(uint64_t cap, int T);
size_t consumer_scratch_bytes(int H, int W);
int launch_consumer(int H, int W, const float *allmap, const float *gt_depth, const uint8_t *valid,
                    const float *col_h, const float *row_h, float depth_ratio, float lambda_n, float lambda_a,
                    int n_valid, float *sums, float *dL_dallmap, void *scratch, size_t scratch_bytes,
                    hipStream_t st, bool sums_zeroed = false, struct ConsumerArgs *args_out_skip_c = nullptr,
                    int order_tiles = 0, const uint32_t *block_cost = nullptr, uint32_t *block_order = nullptr,
                    bool no_launch = false);
int launch_touched_bitmap(int N, const uint8_t *touched, const float *scaling_raw, float smax, float pen,
                          const uint32_t *status_block, uint64_t *bitmap, hipStream_t st);
int launch_adam(const SlsAdamGroup *groups, int ngroups, double beta1, double beta2, double eps, int64_t step,
                const uint32_t *skip_flag, hipStream_t stream, const float *void_flags = nullptr,
                uint32_t *status_block = nullptr, uint32_t *status_mirror = nullptr);

// ---------------------------------------------------------------------------
// workspace of sls_mapping_step: one caller-owned buffer, carved here
// ---------------------------------------------------------------------------
struct MapWs {
    float *rec; int32_t *radii; int32_t *rect; uint32_t *tiles; uint64_t *tmask; int32_t *erec; int32_t *serec; uint32_t *sbox; float *depth; uint32_t *order; uint32_t *offsets;
    void *order_scratch; size_t order_scratch_bytes;
    uint32_t *tkeys, *vals, *tkeys_tmp, *vals_tmp; void *sort_scratch; size_t sort_scratch_bytes;
    uint32_t *ranges; float *allmap; float *pix_state; uint32_t *pix_contrib; uint32_t *tile_consumed;
    float *dL_dallmap; void *consumer_scratch; size_t consumer_scratch_bytes; float *grec; size_t zero_bytes; uint64_t *block_masks; float *reg_accum; uint8_t *touched;
    uint32_t *det_max; unsigned long long *det_acc; size_t det_bytes;    // deterministic accumulation (zeroed per iteration when used)
    uint32_t *det_gex;                                                   // one-pass variant: the fields' default scales (16 words)
    uint32_t *block_cost, *block_order;                                  // backward blocks: cost from the forward, order (most expensive first)
    size_t total;
};

static MapWs carve(int N, int H, int W, uint64_t cap, void *base, bool deterministic)
{
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    MapWs w;
    char *p = (char *)base;
    size_t off = 0;
    auto take = [&](size_t bytes) { void *r = (void *)(p + off); off += al(bytes); return r; };
    const size_t n = (size_t)(N > 0 ? N : 1), P = (size_t)H * W, c = (size_t)(cap > 0 ? cap : 1);
    const int GX = (W + kTileW - 1) / kTileW, GY = (H + kTileH - 1) / kTileH;
    const size_t T = (size_t)GX * GY;
    w.rec = (float *)take(n * SLS_REC_STRIDE * 4);
    w.radii = (int32_t *)take(n * 4);
    w.rect = (int32_t *)take(n * 16);
    w.tiles = (uint32_t *)take(n * 4);
    w.tmask = (uint64_t *)take(n * 8);
    w.erec = (int32_t *)take(n * 16);
    w.serec = (int32_t *)take(n * 8);          // direct binning: the emission records by depth position
    w.sbox = (uint32_t *)take(n * 4);          // block box per surfel (sls_common.hpp: make_block_box)
    w.depth = (float *)take(n * 4);
    w.order = (uint32_t *)take(n * 4);
    w.offsets = (uint32_t *)take(n * 4);
    w.order_scratch_bytes = order_scratch_bytes(N);
    w.order_scratch = take(w.order_scratch_bytes);
    w.tkeys = (uint32_t *)take(c * 4);
    w.vals = (uint32_t *)take(c * 4);
    w.tkeys_tmp = (uint32_t *)take(c * 4);
    w.vals_tmp = (uint32_t *)take(c * 4);
    w.sort_scratch_bytes = sort_scratch_bytes(cap);
    w.sort_scratch = take(w.sort_scratch_bytes);
    w.ranges = (uint32_t *)take(T * 8);
    w.allmap = (float *)take(P * 7 * 4);
    w.pix_state = (float *)take(P * 16);
    w.pix_contrib = (uint32_t *)take(P * 8);
    w.dL_dallmap = (float *)take(P * 7 * 4);
    w.consumer_scratch_bytes = consumer_scratch_bytes(H, W);
    w.consumer_scratch = take(w.consumer_scratch_bytes);
    w.block_masks = (uint64_t *)take(block_mask_bytes(cap, (int)T));
    // zeroed together on the first use of a workspace: [reg_accum | tile_consumed | touched | grec]
    w.reg_accum = (float *)take(4);
    w.det_gex = (uint32_t *)take(16 * 4);
    w.tile_consumed = (uint32_t *)take(T * 4);
    w.touched = (uint8_t *)take(n);
    w.grec = (float *)take(n * SLS_GREC_STRIDE * 4);
    w.zero_bytes = (size_t)((char *)w.grec - (char *)w.reg_accum) + n * SLS_GREC_STRIDE * 4;
    w.block_cost = (uint32_t *)take(T * (kTilePix / 16) * 4);
    w.block_order = (uint32_t *)take(T * (kTilePix / 16) * 4);
    // deterministic accumulation only (192 B per surfel: as much again as everything per-surfel above)
    w.det_max = nullptr; w.det_acc = nullptr; w.det_bytes = 0;
    if (deterministic) {
        w.det_max = (uint32_t *)take(n * SLS_GREC_STRIDE * 4);
        w.det_acc = (unsigned long long *)take(n * SLS_GREC_STRIDE * 8);
        w.det_bytes = (size_t)((char *)w.det_acc - (char *)w.det_max) + n * SLS_GREC_STRIDE * 8;
    }
    w.total = off;
    return w;
}

// Workspace of sls_mapping_step_batch.  The keyframes' fronts run one after another on the stream, so everything a
// front uses and leaves behind for nobody (instances, lists, sort scratch, pixel state, maps, dL/dallmap, block masks)
// is SHARED: keyframe 0's slice is a whole workspace.  Each further keyframe gets only what the batched projection
// backward reads after all fronts: radii, the loss stage's scratch (its per-block loss terms), the forward's block
// costs, the zeroed group [reg_accum | det_gex | tile_consumed | touched | grec] and the fixed-point accumulators.
// w[g] is keyframe g's view; the return value is the total size.
static size_t carve_batch(int G, int N, int H, int W, uint64_t cap, void *base, bool deterministic, MapWs *w)
{
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const MapWs w0 = carve(N, H, W, cap, base, deterministic);
    const size_t n = (size_t)(N > 0 ? N : 1);
    const int GX = (W + kTileW - 1) / kTileW, GY = (H + kTileH - 1) / kTileH;
    const size_t T = (size_t)GX * GY;
    size_t off = w0.total;
    for (int g = 0; g < G; ++g) {
        MapWs k = w0;
        if (g > 0) {
            char *p = (char *)base;
            auto take = [&](size_t bytes) { void *r = (void *)(p + off); off += al(bytes); return r; };
            k.radii = (int32_t *)take(n * 4);
            k.consumer_scratch = take(k.consumer_scratch_bytes);
            k.block_cost = (uint32_t *)take(T * (kTilePix / 16) * 4);
            k.reg_accum = (float *)take(4);
            k.det_gex = (uint32_t *)take(16 * 4);
            k.tile_consumed = (uint32_t *)take(T * 4);
            k.touched = (uint8_t *)take(n);
            k.grec = (float *)take(n * SLS_GREC_STRIDE * 4);
            k.zero_bytes = (size_t)((char *)k.grec - (char *)k.reg_accum) + n * SLS_GREC_STRIDE * 4;
            if (deterministic) {
                k.det_max = (uint32_t *)take(n * SLS_GREC_STRIDE * 4);
                k.det_acc = (unsigned long long *)take(n * SLS_GREC_STRIDE * 8);
                k.det_bytes = (size_t)((char *)k.det_acc - (char *)k.det_max) + n * SLS_GREC_STRIDE * 8;
            }
        }
        k.total = 0;
        if (w) w[g] = k;
    }
    return off;
}

}  // namespace sls

using namespace sls;

extern "C" {

size_t sls_stage1_scratch_bytes(int N) { return order_scratch_bytes(N); }

int sls_forward_stage1(const SlsCamera *cam, int N, const float *means3D, const float *scales,
                       const float *rotations, const float *opacities, const float *col_cs, const float *row_cs,
                       float *rec, int32_t *radii, int32_t *rect,
                       uint32_t *tiles_touched, uint64_t *tile_mask, uint32_t *block_box, float *depth, uint32_t *order,
                       uint32_t *offsets, uint32_t *total_out, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(cam && total_out, "null pointer");
    SLS_REQUIRE(N >= 0, "negative N");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        SLS_HIP_CHECK(hipMemsetAsync(total_out, 0, sizeof(uint32_t), st));
        return SLS_OK;
    }
    SLS_REQUIRE(means3D && scales && rotations && opacities && rec && radii && rect && tiles_touched && depth &&
                    order && offsets && scratch,
                "null pointer");
    const DevCam dc = make_devcam(*cam);
    // (the ray tables and the mask buffer are D10's: required only while the tile-level footprint test is on)
    SLS_REQUIRE(dc.tile_cull == 0 || (col_cs && row_cs && tile_mask),
                "the tile-level footprint test (SlsCamera.tile_cull_min >= 2) needs the ray tables and a tile_mask buffer");
    if (scratch_bytes < order_scratch_bytes(N)) {
        set_error("stage1 scratch too small");
        return SLS_E_SCRATCH;
    }
    // without the tables the preprocess writes no masks: every tile of every rectangle is emitted
    if (tile_mask && !(col_cs && row_cs)) SLS_HIP_CHECK(hipMemsetAsync(tile_mask, 0xFF, sizeof(uint64_t) * (size_t)N, st));
    uint32_t *okeys, *ovals, *n_dev;
    depth_order_key_buffers(N, scratch, order, &okeys, &ovals, &n_dev);
    int rc = launch_preprocess_fwd(dc, 0, 0.0f, 0.0f, nullptr, N, means3D, scales, rotations, opacities, rec, radii,
                                   rect, tiles_touched, depth, okeys, ovals, n_dev, st, nullptr, col_cs, row_cs, tile_mask,
                                   nullptr, nullptr, nullptr, block_box);
    if (rc) return rc;
    return launch_depth_order_scan(N, depth, tiles_touched, order, offsets, total_out, scratch, scratch_bytes, 1, st);
}

size_t sls_sort_scratch_bytes(uint64_t R) { return sort_scratch_bytes(R); }
size_t sls_block_mask_bytes(uint64_t R, int H, int W)
{
    return block_mask_bytes(R, ((W + kTileW - 1) / kTileW) * ((H + kTileH - 1) / kTileH));
}

int sls_forward_stage2(const SlsCamera *cam, int N, uint64_t R, const float *rec, const int32_t *rect,
                       const uint32_t *tiles_touched, const uint64_t *tile_mask, const uint32_t *block_box,
                       const float *depth, const uint32_t *order,
                       const uint32_t *offsets, const uint32_t *total_dev, uint32_t *tkeys, uint32_t *vals,
                       uint32_t *tkeys_tmp, uint32_t *vals_tmp, void *sort_scratch, size_t sort_scratch_bytes_,
                       int *sorted_in_tmp, uint64_t *keys64_out, int list_pairs, const uint32_t **sorted_list,
                       int *sorted_stride, uint32_t *ranges, const float *col_cs,
                       const float *row_cs, float *allmap, float *pix_state, uint32_t *pix_contrib,
                       uint32_t *tile_consumed, uint64_t *block_masks, int *block_masks_shape, void *stream)
{
    SLS_REQUIRE(cam && sorted_in_tmp && sorted_list && sorted_stride && ranges && col_cs && row_cs && allmap &&
                    pix_state && pix_contrib,
                "null pointer");
    SLS_REQUIRE(R == 0 || (rec && rect && tiles_touched && depth && order && offsets && total_dev && tkeys && vals &&
                           tkeys_tmp && vals_tmp && sort_scratch),
                "null pointer");
    SLS_REQUIRE(R < (1ull << 32), "more than 2^32 tile instances");
    SLS_REQUIRE(list_pairs >= 0 && list_pairs <= 2, "list_pairs: 0 auto, 1 whenever possible, 2 never");
    hipStream_t st = (hipStream_t)stream;
    const DevCam dc = make_devcam(*cam);
    // With the surfels' block boxes the tile sort delivers (surfel, block mask) pairs in list order and the forward
    // runs its dense rounds — the kernels of sls_mapping_step, under the same long-list rule (R is exact here)
    const uint2 *bmask = nullptr;
    const uint32_t *boxes = keys64_out ? nullptr : block_box;
    int rc;
    if (!keys64_out && R > 0 && bin_direct_possible(dc, N, (uint32_t)R)) {
        // direct binning (sls_sort.hip), as in sls_mapping_step; the records are gathered from rect / block_box
        *sorted_in_tmp = 0;
        if (sort_scratch_bytes_ < sort_scratch_bytes(R)) {
            set_error("sort scratch too small: %zu < %zu", sort_scratch_bytes_, sort_scratch_bytes(R));
            return SLS_E_SCRATCH;
        }
        const DirectBin db = make_direct_bin(dc, N, sort_scratch, nullptr, false);
        rc = launch_bin_direct(dc, N, (uint32_t)R, db, false, order, nullptr, rect, boxes, sort_scratch, vals, ranges,
                               nullptr, nullptr, 0, nullptr, &bmask, list_pairs, st);
    } else {
        rc = launch_bin_sort(dc, N, total_dev, (uint32_t)R, order, rect, tiles_touched,
                             dc.tile_cull ? tile_mask : nullptr, nullptr, depth, offsets, tkeys, vals,
                             tkeys_tmp, vals_tmp, sort_scratch, sort_scratch_bytes_, sorted_in_tmp, ranges,
                             keys64_out, nullptr, st, nullptr, nullptr, boxes, &bmask, list_pairs);
    }
    if (rc) return rc;
    const uint32_t *sorted_vals = *sorted_in_tmp ? vals_tmp : vals;
    *sorted_list = bmask ? (const uint32_t *)bmask : sorted_vals;
    *sorted_stride = bmask ? 2 : 1;
    if (block_masks_shape) *block_masks_shape = block_masks ? 3 : 0;
    return launch_render_fwd(dc, ranges, sorted_vals, rec, col_cs, row_cs, allmap, pix_state, pix_contrib,
                             tile_consumed, st, false, block_masks, (cam->flags & SLS_CAM_LEAN_ALLMAP) != 0, nullptr, bmask,
                             true);       // (+ the backward's launch order into the hand-over buffer)
}

// ---- pose gradient (D11): the caller's scratch = one arrival counter (a 256-byte slot) + one row per workgroup of the
// projection's backward and keyframe
static size_t pose_scratch_bytes(int G, int N)
{
    // (G times the single keyframe's: one counter is used, the documented size is the simple one)
    return (size_t)G * (256 + (size_t)((N + 255) / 256) * kPoseRow * sizeof(float));
}
size_t sls_pose_grad_scratch_bytes(int N) { return N > 0 ? pose_scratch_bytes(1, N) : 0; }

// Checks a call's pose arguments (before anything is enqueued) and fills the launcher's view of them; *use = false
// where no pose gradient is asked for (pose_grad[g] all null).
static int make_pose_out(int G, int N, float *const *pose_grad, void *scratch, size_t scratch_bytes, PoseOut *po, bool *use)
{
    memset(po, 0, sizeof(*po));
    int n = 0;
    for (int g = 0; g < G; ++g) n += pose_grad[g] ? 1 : 0;
    *use = n > 0;
    if (n == 0) return SLS_OK;
    SLS_REQUIRE(n == G, "pose_grad on every keyframe of the batch or on none");
    SLS_REQUIRE(scratch && ((uintptr_t)scratch & 7) == 0, "pose_grad needs pose_scratch (8-byte aligned, sls_pose_grad_scratch_bytes)");
    if (scratch_bytes < pose_scratch_bytes(G, N)) {
        set_error("pose-gradient scratch too small: %zu < %zu", scratch_bytes, pose_scratch_bytes(G, N));
        return SLS_E_SCRATCH;
    }
    po->counter = (uint32_t *)scratch;
    po->rows = (float *)((char *)scratch + 256);
    for (int g = 0; g < G; ++g) {
        for (int h = 0; h < g; ++h) SLS_REQUIRE(pose_grad[h] != pose_grad[g], "two keyframes share one pose_grad buffer");
        po->out[g] = pose_grad[g];
    }
    return SLS_OK;
}

int sls_backward(const SlsCamera *cam, int N, uint64_t R, const float *means3D, const float *scales,
                 const float *rotations, const int32_t *radii, const float *rec, const uint32_t *ranges,
                 const uint32_t *vals_sorted, int vals_stride, const float *col_cs, const float *row_cs,
                 const float *pix_state,
                 const uint32_t *pix_contrib, const float *dL_dallmap, float *grec, float *dL_dmeans3D,
                 float *dL_dscales, float *dL_drotations, float *dL_dopacities, const uint64_t *block_masks,
                 int block_masks_shape, void *stream)
{
    return sls_backward_pose(cam, N, R, means3D, scales, rotations, radii, rec, ranges, vals_sorted, vals_stride, col_cs,
                             row_cs, pix_state, pix_contrib, dL_dallmap, grec, dL_dmeans3D, dL_dscales, dL_drotations,
                             dL_dopacities, block_masks, block_masks_shape, nullptr, nullptr, 0, stream);
}

int sls_backward_pose(const SlsCamera *cam, int N, uint64_t R, const float *means3D, const float *scales,
                      const float *rotations, const int32_t *radii, const float *rec, const uint32_t *ranges,
                      const uint32_t *vals_sorted, int vals_stride, const float *col_cs, const float *row_cs,
                      const float *pix_state,
                      const uint32_t *pix_contrib, const float *dL_dallmap, float *grec, float *dL_dmeans3D,
                      float *dL_dscales, float *dL_drotations, float *dL_dopacities, const uint64_t *block_masks,
                      int block_masks_shape, float *pose_grad, void *pose_scratch, size_t pose_scratch_bytes_, void *stream)
{
    SLS_REQUIRE(cam, "null pointer");
    SLS_REQUIRE(N >= 0, "negative N");
    if (N == 0) {
        if (pose_grad) SLS_HIP_CHECK(hipMemsetAsync(pose_grad, 0, 6 * sizeof(float), (hipStream_t)stream));
        return SLS_OK;
    }
    PoseOut po;
    bool use_pose;
    if (int prc = make_pose_out(1, N, &pose_grad, pose_scratch, pose_scratch_bytes_, &po, &use_pose)) return prc;
    SLS_REQUIRE(means3D && scales && rotations && radii && grec && dL_dmeans3D && dL_dscales && dL_drotations &&
                    dL_dopacities,
                "null pointer");
    SLS_REQUIRE(vals_stride == 1 || vals_stride == 2, "vals_stride: 1 (plain list) or 2 ((surfel, block mask) pairs)");
    hipStream_t st = (hipStream_t)stream;
    const DevCam dc = make_devcam(*cam);
    {
        ScopedTimer tm(T_GREC_MEMSET, st);
        SLS_HIP_CHECK(hipMemsetAsync(grec, 0, sizeof(float) * (size_t)N * SLS_GREC_STRIDE, st));
    }
    if (R > 0) {
        SLS_REQUIRE(rec && ranges && vals_sorted && col_cs && row_cs && pix_state && pix_contrib && dL_dallmap,
                    "null pointer");
        int rc = launch_render_bwd(dc, ranges, vals_sorted, rec, col_cs, row_cs, pix_state, pix_contrib, dL_dallmap,
                                   grec, st, block_masks_shape ? block_masks : nullptr, (cam->flags & SLS_CAM_LEAN_ALLMAP) != 0,
                                   nullptr, nullptr, nullptr, nullptr, nullptr, vals_stride, block_masks_shape, true);
        if (rc) return rc;
    }
    return launch_preprocess_bwd(dc, 0, 0.0f, 0.0f, N, means3D, scales, rotations, nullptr, radii, grec, dL_dmeans3D,
                                 dL_dscales, dL_drotations, dL_dopacities, st, nullptr, use_pose ? &po : nullptr);
}

size_t sls_backward_det_scratch_bytes(int N) { return N > 0 ? (size_t)N * SLS_GREC_STRIDE * 12 + 256 : 256; }

int sls_backward_det(const SlsCamera *cam, int N, uint64_t R, const float *means3D, const float *scales,
                     const float *rotations, const int32_t *radii, const float *rec, const uint32_t *ranges,
                     const uint32_t *vals_sorted, int vals_stride, const float *col_cs, const float *row_cs,
                     const float *pix_state,
                     const uint32_t *pix_contrib, const float *dL_dallmap, float *dL_dmeans3D, float *dL_dscales,
                     float *dL_drotations, float *dL_dopacities, const uint64_t *block_masks, int block_masks_shape,
                     void *det_scratch, size_t det_scratch_bytes, void *stream)
{
    return sls_backward_det_pose(cam, N, R, means3D, scales, rotations, radii, rec, ranges, vals_sorted, vals_stride,
                                 col_cs, row_cs, pix_state, pix_contrib, dL_dallmap, dL_dmeans3D, dL_dscales,
                                 dL_drotations, dL_dopacities, block_masks, block_masks_shape, det_scratch,
                                 det_scratch_bytes, nullptr, nullptr, 0, stream);
}

int sls_backward_det_pose(const SlsCamera *cam, int N, uint64_t R, const float *means3D, const float *scales,
                          const float *rotations, const int32_t *radii, const float *rec, const uint32_t *ranges,
                          const uint32_t *vals_sorted, int vals_stride, const float *col_cs, const float *row_cs,
                          const float *pix_state,
                          const uint32_t *pix_contrib, const float *dL_dallmap, float *dL_dmeans3D, float *dL_dscales,
                          float *dL_drotations, float *dL_dopacities, const uint64_t *block_masks, int block_masks_shape,
                          void *det_scratch, size_t det_scratch_bytes, float *pose_grad, void *pose_scratch,
                          size_t pose_scratch_bytes_, void *stream)
{
    SLS_REQUIRE(cam, "null pointer");
    SLS_REQUIRE(N >= 0, "negative N");
    if (N == 0) {
        if (pose_grad) SLS_HIP_CHECK(hipMemsetAsync(pose_grad, 0, 6 * sizeof(float), (hipStream_t)stream));
        return SLS_OK;
    }
    PoseOut po;
    bool use_pose;
    if (int prc = make_pose_out(1, N, &pose_grad, pose_scratch, pose_scratch_bytes_, &po, &use_pose)) return prc;
    SLS_REQUIRE(means3D && scales && rotations && radii && det_scratch && dL_dmeans3D && dL_dscales && dL_drotations &&
                    dL_dopacities,
                "null pointer");
    SLS_REQUIRE(vals_stride == 1 || vals_stride == 2, "vals_stride: 1 (plain list) or 2 ((surfel, block mask) pairs)");
    if (det_scratch_bytes < sls_backward_det_scratch_bytes(N)) {
        set_error("deterministic-backward scratch too small");
        return SLS_E_SCRATCH;
    }
    hipStream_t st = (hipStream_t)stream;
    const DevCam dc = make_devcam(*cam);
    unsigned long long *acc = (unsigned long long *)(((uintptr_t)det_scratch + 255) & ~(uintptr_t)255);
    uint32_t *mx = (uint32_t *)(acc + (size_t)N * SLS_GREC_STRIDE);
    SLS_HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)N * SLS_GREC_STRIDE * 12, st));
    if (R > 0) {
        SLS_REQUIRE(rec && ranges && vals_sorted && col_cs && row_cs && pix_state && pix_contrib && dL_dallmap,
                    "null pointer");
        int rc = launch_render_bwd(dc, ranges, vals_sorted, rec, col_cs, row_cs, pix_state, pix_contrib, dL_dallmap,
                                   nullptr, st, block_masks_shape ? block_masks : nullptr,
                                   (cam->flags & SLS_CAM_LEAN_ALLMAP) != 0, nullptr, nullptr, mx, acc,
                                   nullptr, vals_stride, block_masks_shape, true);
        if (rc) return rc;
    }
    AdamFuse fuse;
    memset(&fuse, 0, sizeof(fuse));
    fuse.det_max = mx;
    fuse.det_acc = (const long long *)acc;
    return launch_preprocess_bwd(dc, 0, 0.0f, 0.0f, N, means3D, scales, rotations, nullptr, radii, nullptr, dL_dmeans3D,
                                 dL_dscales, dL_drotations, dL_dopacities, st, &fuse, use_pose ? &po : nullptr);
}

// ---- the drop-in forward without the host read of R --------------------------------------------------------------
// (the status block — R, void bits — reaches the caller's pinned host mirror from the first workgroup of bin_direct)
size_t sls_forward_ws_bytes(int N, int H, int W, uint64_t R_capacity)
{
    if (N < 0 || H <= 0 || W <= 0) return 0;
    return carve(N, H, W, R_capacity, nullptr, false).total;
}

int sls_forward_ws(const SlsCamera *cam, int N, const float *means3D, const float *scales, const float *rotations,
                   const float *opacities, const float *col_cs, const float *row_cs, uint64_t R_capacity,
                   uint32_t *depth_order, int reuse_rounds, int list_pairs, int workspace_ready, int want_backward,
                   int32_t *radii, float *allmap, void *workspace, size_t workspace_bytes, SlsMappingStatus *status_dev,
                   SlsMappingStatus *status_mirror, const uint32_t **sorted_list, int *sorted_stride,
                   int *block_masks_shape, void *stream)
{
    SLS_REQUIRE(cam && status_dev && workspace && sorted_list && sorted_stride && block_masks_shape, "null pointer");
    SLS_REQUIRE(N > 0, "N must be positive");
    SLS_REQUIRE(means3D && scales && rotations && opacities && col_cs && row_cs && radii && allmap, "null pointer");
    SLS_REQUIRE(R_capacity > 0 && R_capacity < (1ull << 32), "bad instance capacity");
    SLS_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    SLS_REQUIRE(reuse_rounds >= 0 && reuse_rounds <= 4, "reuse_rounds: 0 from scratch, 1..4 repair rounds");
    SLS_REQUIRE(reuse_rounds == 0 || depth_order, "a repair needs the camera's previous depth order");
    SLS_REQUIRE(list_pairs >= 0 && list_pairs <= 2, "list_pairs: 0 auto, 1 whenever possible, 2 never");
    const int H = cam->H, W = cam->W;
    const DevCam dc = make_devcam(*cam);
    const uint32_t cap = (uint32_t)R_capacity;
    if (!bin_direct_possible(dc, N, cap)) {
        set_error("sls_forward_ws serves what the direct binning serves (<= 512 tiles, D10 off): use the staged forward");
        return SLS_E_UNSUPPORTED;
    }
    const MapWs w = carve(N, H, W, R_capacity, workspace, false);
    if (workspace_bytes < w.total) {
        set_error("forward workspace too small: %zu < %zu", workspace_bytes, w.total);
        return SLS_E_SCRATCH;
    }
    hipStream_t st = (hipStream_t)stream;
    if (!workspace_ready) {     // the gradient records and the touched marks start from zero; the backward leaves them so
        ScopedTimer tm(T_GREC_MEMSET, st);
        SLS_HIP_CHECK(hipMemsetAsync(w.reg_accum, 0, w.zero_bytes, st));
    }
    uint32_t *okeys, *ovals, *n_dev;
    uint32_t *order = depth_order ? depth_order : w.order;
    depth_order_key_buffers(N, w.order_scratch, order, &okeys, &ovals, &n_dev);
    const bool merged_sort = reuse_rounds >= 1;
    DirectBin db = make_direct_bin(dc, N, w.sort_scratch, (uint2 *)w.serec, reuse_rounds >= 1, true);
    // (as in sls_mapping_step: the direct binning reads the emission records only)
    int rc = launch_preprocess_fwd(dc, 0, 0.0f, 0.0f, nullptr, N, means3D, scales, rotations, opacities, w.rec, radii,
                                   nullptr, nullptr, nullptr, merged_sort ? nullptr : okeys, ovals, n_dev, st,
                                   (uint32_t *)status_dev, col_cs, row_cs, w.tmask, w.erec, merged_sort ? order : nullptr,
                                   merged_sort ? resort_comp_buffer(N, w.order_scratch) : nullptr, nullptr, 1, db.coarse,
                                   (int)direct_coarse_words(dc, N));
    if (rc) return rc;
    ScanHandoff handoff = { nullptr, 0, nullptr, 0 };
    rc = launch_depth_order_scan(N, w.depth, w.tiles, order, w.offsets, &status_dev->R, w.order_scratch,
                                 w.order_scratch_bytes, 1, st, reuse_rounds, &status_dev->overflow, &handoff, merged_sort,
                                 &db, (const int4 *)w.erec, dc.GX);
    if (rc) return rc;
    const uint2 *bmask = nullptr;
    rc = launch_bin_direct(dc, N, cap, db, handoff.counted != 0, order, w.erec, nullptr, nullptr, w.sort_scratch, w.vals,
                           w.ranges, &status_dev->R, &status_dev->overflow, handoff.resort_windows, handoff.resort_edges,
                           &bmask, list_pairs, st, (uint32_t *)status_mirror);      // (the status block leaves from its first workgroup)
    if (rc) return rc;
    const uint32_t *list = bmask ? (const uint32_t *)bmask : w.vals;
    *sorted_list = list;
    *sorted_stride = bmask ? 2 : 1;
    // a forward nobody differentiates (render() under no_grad: Mapper.densify, the tracker) writes no hand-over; one
    // that is leaves the backward its blocks' compact lists and their costs (sorted into the camera's launch order by
    // passengers of the backward's last kernel, for the camera's NEXT backward: as sls_mapping_step does)
    *block_masks_shape = want_backward ? 3 : 0;
    return launch_render_fwd(dc, w.ranges, list, w.rec, col_cs, row_cs, allmap, w.pix_state, w.pix_contrib, nullptr, st,
                             true, want_backward ? w.block_masks : nullptr, (cam->flags & SLS_CAM_LEAN_ALLMAP) != 0,
                             want_backward ? w.block_cost : nullptr, bmask, false);
}

int sls_backward_ws(const SlsCamera *cam, int N, const float *means3D, const float *scales, const float *rotations,
                    const int32_t *radii, const float *col_cs, const float *row_cs, const float *dL_dallmap,
                    uint64_t R_capacity, void *workspace, size_t workspace_bytes, const uint32_t *sorted_list,
                    int sorted_stride, int block_masks_shape, uint32_t *block_order, float *dL_dmeans3D,
                    float *dL_dscales, float *dL_drotations, float *dL_dopacities, void *stream)
{
    return sls_backward_ws_pose(cam, N, means3D, scales, rotations, radii, col_cs, row_cs, dL_dallmap, R_capacity, workspace,
                                workspace_bytes, sorted_list, sorted_stride, block_masks_shape, block_order, dL_dmeans3D,
                                dL_dscales, dL_drotations, dL_dopacities, nullptr, nullptr, 0, stream);
}

int sls_backward_ws_pose(const SlsCamera *cam, int N, const float *means3D, const float *scales, const float *rotations,
                         const int32_t *radii, const float *col_cs, const float *row_cs, const float *dL_dallmap,
                         uint64_t R_capacity, void *workspace, size_t workspace_bytes, const uint32_t *sorted_list,
                         int sorted_stride, int block_masks_shape, uint32_t *block_order, float *dL_dmeans3D,
                         float *dL_dscales, float *dL_drotations, float *dL_dopacities, float *pose_grad,
                         void *pose_scratch, size_t pose_scratch_bytes_, void *stream)
{
    SLS_REQUIRE(cam && workspace && sorted_list, "null pointer");
    SLS_REQUIRE(N > 0, "N must be positive");
    PoseOut po;
    bool use_pose;
    if (int prc = make_pose_out(1, N, &pose_grad, pose_scratch, pose_scratch_bytes_, &po, &use_pose)) return prc;
    SLS_REQUIRE(means3D && scales && rotations && radii && col_cs && row_cs && dL_dallmap && dL_dmeans3D && dL_dscales &&
                    dL_drotations && dL_dopacities,
                "null pointer");
    SLS_REQUIRE(sorted_stride == 1 || sorted_stride == 2, "sorted_stride: 1 (plain list) or 2 ((surfel, block mask) pairs)");
    const MapWs w = carve(N, cam->H, cam->W, R_capacity, workspace, false);
    if (workspace_bytes < w.total) {
        set_error("forward workspace too small: %zu < %zu", workspace_bytes, w.total);
        return SLS_E_SCRATCH;
    }
    hipStream_t st = (hipStream_t)stream;
    const DevCam dc = make_devcam(*cam);
    // the tile backward marks the surfels it reaches; the projection's backward reads — and clears — only their records:
    // no 64 N-byte memset per call
    // the blocks most expensive first per XCD, in the order this camera's PREVIOUS backward left in the caller's buffer
    // (its tag word says whether one has: a first visit walks the natural order)
    const int T = dc.GX * dc.GY;
    const bool order_bwd = block_order != nullptr && block_masks_shape == 3 && T % 32 == 0 && kTileW == 16 && kTileH == 16;
    // (the launcher walks the forward's compact lists only when block_masks_shape is 3, otherwise the backward culls the
    //  tiles' lists itself; the kernel's tag check is a last guard against a FOREIGN buffer, which the workspace lease
    //  rules out on this path)
    int rc = launch_render_bwd(dc, w.ranges, sorted_list, w.rec, col_cs, row_cs, w.pix_state, w.pix_contrib, dL_dallmap,
                               w.grec, st, block_masks_shape ? w.block_masks : nullptr,
                               (cam->flags & SLS_CAM_LEAN_ALLMAP) != 0, w.touched, nullptr, nullptr, nullptr,
                               order_bwd ? block_order : nullptr, sorted_stride, block_masks_shape, false, nullptr, nullptr,
                               nullptr, false, order_bwd ? block_order_tag(T) : 0u);
    if (rc) return rc;
    AdamFuse fuse;
    memset(&fuse, 0, sizeof(fuse));
    fuse.clear_grec = 1;
    fuse.touched = w.touched;
    if (order_bwd) { fuse.order_T = T; fuse.order_cost = w.block_cost; fuse.order_out = block_order; }
    return launch_preprocess_bwd(dc, 0, 0.0f, 0.0f, N, means3D, scales, rotations, nullptr, radii, w.grec, dL_dmeans3D,
                                 dL_dscales, dL_drotations, dL_dopacities, st, &fuse, use_pose ? &po : nullptr);
}

// The front of an iteration (forward, loss, tile backward) on ONE keyframe, into ONE workspace slice: sls_mapping_step
// and, per keyframe, sls_mapping_step_batch
static int mapping_front(const SlsCamera *cam, int N, const float *xyz, const float *scaling_raw, const float *rotation_raw,
                         const float *opacity_raw, const float *gt_depth, const uint8_t *valid, int n_valid,
                         const float *col_cs, const float *row_cs, const float *col_cs_half, const float *row_cs_half,
                         const SlsMappingConfig *cfg, uint32_t cap, const MapWs &w, SlsMappingStatus *status_dev,
                         hipStream_t st)
{
    const int H = cam->H, W = cam->W;
    const DevCam dc = make_devcam(*cam);
    uint8_t *touched = w.touched;
    const bool det = cfg->deterministic != 0;
    const bool det_one = cfg->deterministic == 2 && cfg->det_prev != nullptr;
    const bool fuse_c = cfg->depth_ratio == 0.0f;
    const bool fuse_b = fuse_c && cfg->block_order != nullptr;
    const bool order_bwd = (dc.GX * dc.GY) % 32 == 0 && kTileW == 16 && kTileH == 16;
    // (the status block is zeroed by thread 0 of preprocess_fwd, the iteration's first kernel)
    if (!cfg->workspace_ready) {
        // first use of this workspace: the gradient records must start from zero; afterwards the backward
        // of the projection leaves them zeroed behind itself (no 64*N-byte memset per iteration)
        ScopedTimer tm(T_GREC_MEMSET, st);
        SLS_HIP_CHECK(hipMemsetAsync(w.reg_accum, 0, w.zero_bytes, st));
    }

    // ---- forward ---------------------------------------------------------------
    uint32_t *okeys, *ovals, *n_dev;
    // the depth order lives in the workspace, or in a caller-owned buffer (one per keyframe, so that every
    // keyframe of a window can repair ITS order when the mapper samples keyframes at random)
    uint32_t *order = cfg->depth_order ? cfg->depth_order : w.order;
    depth_order_key_buffers(N, w.order_scratch, order, &okeys, &ovals, &n_dev);
    // Repairing the previous order: its first step (sorting windows of the old order by the new keys) rides in the
    // preprocess launch — it needs nothing the preprocess produces
    const bool merged_sort = cfg->reuse_depth_order >= 1;
    // Direct binning (sls_sort.hip) where it applies: no unsorted instance array, no scan of tiles_touched; the preprocess
    // then leaves the emission records in the form its first kernel gathers (rectangle + block box)
    const bool direct = bin_direct_possible(dc, N, cap);
    // (the staged API scans the count table's rows with a launch of its own instead)
    DirectBin db;
    if (direct) db = make_direct_bin(dc, N, w.sort_scratch, (uint2 *)w.serec, cfg->reuse_depth_order >= 1, true);
    // (the direct binning reads the emission records only — not the rectangles, the tile counts, the depths or the
    //  block boxes as arrays of their own; a repair whose window sort rides in the preprocess launch computes its
    //  keys itself: 32 bytes per surfel that are not written)
    const bool trim = direct;
    int rc = launch_preprocess_fwd(dc, 1, cfg->scaling_max, cfg->scaling_max_penalty, w.reg_accum, N, xyz,
                                   scaling_raw, rotation_raw, opacity_raw, w.rec, w.radii, trim ? nullptr : w.rect,
                                   trim ? nullptr : w.tiles, trim ? nullptr : w.depth,
                                   (trim && merged_sort) ? nullptr : okeys, ovals, n_dev, st,
                                   (uint32_t *)status_dev, col_cs, row_cs, w.tmask, w.erec,
                                   merged_sort ? order : nullptr,
                                   merged_sort ? resort_comp_buffer(N, w.order_scratch) : nullptr, trim ? nullptr : w.sbox, direct ? 1 : 0,
                                   (direct && db.coarse) ? db.coarse : nullptr,
                                   (direct && db.coarse) ? (int)direct_coarse_words(dc, N) : 0);
    if (rc) return rc;
    ScanHandoff handoff = { nullptr, 0, nullptr, 0 };   // the binning finishes (or does not need) the scan of tiles_touched
    rc = launch_depth_order_scan(N, w.depth, w.tiles, order, w.offsets, &status_dev->R, w.order_scratch,
                                 w.order_scratch_bytes, 1, st, cfg->reuse_depth_order, &status_dev->overflow, &handoff,
                                 merged_sort, direct ? &db : nullptr, (const int4 *)w.erec, dc.GX);
    if (rc) return rc;
    int in_tmp = 0;
    const uint2 *bmask = nullptr;
    if (direct) {
        rc = launch_bin_direct(dc, N, cap, db, handoff.counted != 0, order, w.erec, nullptr, nullptr, w.sort_scratch, w.vals,
                               w.ranges, &status_dev->R, &status_dev->overflow, handoff.resort_windows,
                               handoff.resort_edges, &bmask, cfg->block_masks, st);
    } else {
        rc = launch_bin_sort(dc, N, &status_dev->R, cap, order, w.rect, w.tiles, dc.tile_cull ? w.tmask : nullptr,
                             (dc.GX < 65536 && dc.GY < 65536) ? w.erec : nullptr, w.depth,
                             w.offsets, w.tkeys, w.vals,
                             w.tkeys_tmp, w.vals_tmp, w.sort_scratch, w.sort_scratch_bytes, &in_tmp, w.ranges, nullptr,
                             &status_dev->overflow, st, &handoff, &status_dev->R,
                             w.sbox, &bmask, cfg->block_masks);
    }
    if (rc) return rc;
    // (with the pairs the plain value arrays are not written: the list IS the pairs, two words apart)
    const uint32_t *sorted_vals = bmask ? (const uint32_t *)bmask : (in_tmp ? w.vals_tmp : w.vals);
    const int vals_stride = bmask ? 2 : 1;
    rc = launch_render_fwd(dc, w.ranges, sorted_vals, w.rec, col_cs, row_cs, w.allmap, w.pix_state, w.pix_contrib,
                           nullptr, st, true, w.block_masks,    // (nobody reads the consumed counters here)
                           cfg->depth_ratio == 0.0f,            // (nor, then, the median / distortion planes: not tracked)
                           w.block_cost, bmask);
    if (rc) return rc;
    // ---- loss + dL/dallmap --------------------------------------------------------
    // With the keyframe's own launch-order buffer kernel B is folded in as well (fuse_b, above): the loss stage has no
    // launch; the order the backward walks is the one the keyframe's previous iteration left.
    ConsumerArgs cargs;
    rc = launch_consumer(H, W, w.allmap, gt_depth, valid, col_cs_half, row_cs_half, cfg->depth_ratio,
                         cfg->lambda_normal, cfg->lambda_alpha, n_valid, status_dev->loss_sums, w.dL_dallmap,
                         w.consumer_scratch, w.consumer_scratch_bytes, st, true, fuse_c ? &cargs : nullptr,
                         order_bwd ? dc.GX * dc.GY : 0, w.block_cost, w.block_order, fuse_b);
    if (rc) return rc;
    // ---- backward -----------------------------------------------------------------
    // (two launches: both accumulators start from zero; one launch: det_acc is left zeroed by every deterministic
    //  iteration's preprocess_bwd where it was written — and the first deterministic iteration on a workspace is a
    //  two-launch one, which also sets the fields' default scales)
    if (det && !det_one) SLS_HIP_CHECK(hipMemsetAsync(w.det_max, 0, w.det_bytes, st));
    const uint32_t *block_order = order_bwd ? (fuse_b ? cfg->block_order : w.block_order) : nullptr;
    rc = launch_render_bwd(dc, w.ranges, sorted_vals, w.rec, col_cs, row_cs, w.pix_state, w.pix_contrib, w.dL_dallmap,
                           w.grec, st, w.block_masks, cfg->depth_ratio == 0.0f, touched,    // the consumer's dL/d(median, distortion) are 0 then
                           fuse_c ? &cargs : nullptr, (det && !det_one) ? w.det_max : nullptr, det ? w.det_acc : nullptr, block_order,
                           vals_stride, 3, false,
                           det_one ? cfg->det_prev : nullptr, w.det_gex, &status_dev->overflow, fuse_b,
                           (fuse_b && order_bwd) ? block_order_tag(dc.GX * dc.GY) : 0u);
    if (rc) return rc;
    if (cfg->phase == 1 && cfg->grad_bitmap)      // the bitmap EARLY: an all-gather of it can overlap phase 2
        return launch_touched_bitmap(N, touched, scaling_raw, cfg->scaling_max, cfg->scaling_max_penalty,
                                     (const uint32_t *)status_dev, cfg->grad_bitmap, st);
    return SLS_OK;
}

size_t sls_mapping_workspace_bytes(int N, int H, int W, uint64_t R_capacity)
{
    if (N < 0 || H <= 0 || W <= 0) return 0;
    return carve(N, H, W, R_capacity, nullptr, true).total;      // fits either setting of cfg->deterministic
}

size_t sls_block_order_bytes(int H, int W)
{
    if (H <= 0 || W <= 0) return 0;
    const size_t T = (size_t)((W + kTileW - 1) / kTileW) * (size_t)((H + kTileH - 1) / kTileH);
    return sizeof(uint32_t) * (1 + T * (size_t)(kTilePix / 16));
}

size_t sls_mapping_workspace_bytes_cfg(int N, int H, int W, uint64_t R_capacity, const SlsMappingConfig *cfg)
{
    if (N < 0 || H <= 0 || W <= 0) return 0;
    return carve(N, H, W, R_capacity, nullptr, !cfg || cfg->deterministic != 0).total;
}

int sls_mapping_step(const SlsCamera *cam, int N, float *xyz, float *scaling_raw, float *rotation_raw,
                     float *opacity_raw, float *grads, float *exp_avg, float *exp_avg_sq, int64_t adam_step,
                     const float *gt_depth, const uint8_t *valid, int n_valid, const float *col_cs,
                     const float *row_cs, const float *col_cs_half, const float *row_cs_half,
                     const SlsMappingConfig *cfg, uint64_t R_capacity, void *workspace, size_t workspace_bytes,
                     SlsMappingStatus *status_dev, float **allmap_out, void *stream)
{
    SLS_REQUIRE(cam && cfg && status_dev && workspace, "null pointer");
    SLS_REQUIRE(N > 0, "N must be positive");
    SLS_REQUIRE(xyz && scaling_raw && rotation_raw && opacity_raw && grads && gt_depth && valid && col_cs && row_cs &&
                    col_cs_half && row_cs_half,
                "null pointer");
    SLS_REQUIRE(!cfg->apply_adam || (exp_avg && exp_avg_sq && adam_step >= 1), "Adam state missing");
    SLS_REQUIRE(R_capacity > 0 && R_capacity < (1ull << 32), "bad instance capacity");
    SLS_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    // (every argument check before the first launch: an argument error must not leave half an iteration on the stream)
    SLS_REQUIRE(cfg->phase >= 0 && cfg->phase <= 2, "phase: 0 whole iteration, 1 up to the tile backward, 2 the rest");
    PoseOut po;
    bool use_pose;
    {
        float *pg = cfg->pose_grad;
        if (int prc = make_pose_out(1, N, &pg, cfg->pose_scratch, cfg->pose_scratch_bytes, &po, &use_pose)) return prc;
    }
    SLS_REQUIRE(!cfg->grad_bitmap || ((!cfg->apply_adam || cfg->union_bitmap) && !cfg->grad_chunk),
                "the gradient bitmap belongs to apply_adam = 0 with the flat bucket");
    SLS_REQUIRE(!cfg->union_bitmap || (cfg->phase == 2 && cfg->apply_adam && cfg->union_prefix && cfg->grad_compact && cfg->grad_compact_index &&
                                       !cfg->grad_chunk && !cfg->keep_grads && (N % 2) == 0 &&
                                       ((((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0)),
                "union_bitmap: phase 2 with apply_adam = 1, the union's prefix and row buffer, even N, 16-byte aligned moments");
    SLS_REQUIRE(!cfg->grad_chunk ||
                    (!cfg->apply_adam && cfg->grad_ranks >= 1 && (cfg->grad_chunk % 4u) == 0 && (N % 2) == 0 &&
                     (uint64_t)cfg->grad_chunk * cfg->grad_ranks >= (uint64_t)10 * (uint64_t)N &&
                     (uint64_t)10 * (uint64_t)N < (1ull << 32)),
                "reduce-scatter gradient layout: apply_adam = 0, even N, chunk a multiple of 4 covering 10 N");
    const int H = cam->H, W = cam->W;
    const MapWs w = carve(N, H, W, R_capacity, workspace, cfg->deterministic != 0);
    if (workspace_bytes < w.total) {
        set_error("mapping workspace too small: %zu < %zu", workspace_bytes, w.total);
        return SLS_E_SCRATCH;
    }
    hipStream_t st = (hipStream_t)stream;
    const DevCam dc = make_devcam(*cam);
    const uint32_t cap = (uint32_t)R_capacity;
    if (allmap_out) *allmap_out = w.allmap;
    uint8_t *touched = w.touched;   // (the backward tile kernel marks the surfels it reaches)
    const bool det = cfg->deterministic != 0;
    // one launch with predicted scales (cfg->deterministic = 2) on the forward's compact lists
    const bool det_one = cfg->deterministic == 2 && cfg->det_prev != nullptr;
    SLS_REQUIRE(cfg->deterministic >= 0 && cfg->deterministic <= 2, "deterministic: 0 off, 1 two launches, 2 one launch with predicted scales");
    SLS_REQUIRE(cfg->deterministic != 2 || cfg->det_prev, "deterministic = 2 needs the keyframe's det_prev buffer");
    // With depth_ratio = 0 the consumer's second kernel is folded into the
    // backward tile kernel: every pixel block computes its dL/dallmap from kernel B's planes itself ...
    const bool fuse_c = cfg->depth_ratio == 0.0f;
    // ... and with the keyframe's launch-order buffer kernel B's work too
    const bool fuse_b = fuse_c && cfg->block_order != nullptr;
    // the backward's blocks are launched most expensive first (cost recorded by the forward, sorted per XCD by eight
    // passenger workgroups — of the consumer's launch, or with fuse_b of the previous iteration's last launch): 8x2
    // kernels, XCD-interleaved tile mapping (T % 32 == 0)
    const bool order_bwd = (dc.GX * dc.GY) % 32 == 0 && kTileW == 16 && kTileH == 16;
    int rc = SLS_OK;
    if (cfg->phase != 2)
        rc = mapping_front(cam, N, xyz, scaling_raw, rotation_raw, opacity_raw, gt_depth, valid, n_valid, col_cs, row_cs,
                           col_cs_half, row_cs_half, cfg, cap, w, status_dev, st);
    if (rc || cfg->phase == 1) return rc;
    // flat gradient bucket: [xyz 3N | opacity N | scaling 2N | rotation 4N] (optimizer group order)
    float *g_xyz = grads, *g_op = grads + (size_t)3 * N, *g_sc = grads + (size_t)4 * N, *g_rot = grads + (size_t)6 * N;
    // ---- backward of the projection + optimiser -------------------------------------------
    // One keyframe per step: the Adam update is applied to each surfel right where its gradient is
    // produced (no gradient bucket round trip, no second pass over the parameters).
    AdamFuse fuse;
    memset(&fuse, 0, sizeof(fuse));
    fuse.clear_grec = 1;
    static_assert(sizeof(SlsMappingStatus) == 32, "the mirror copy moves 8 words");
    fuse.status_src = (uint32_t *)status_dev;
    fuse.reg_accum = w.reg_accum;
    fuse.touched = touched;
    fuse.status_mirror = (uint32_t *)cfg->status_mirror;
    fuse.void_flags = cfg->void_flags_out;
    fuse.void_count = 1; fuse.void_stride = 0;
    if (det) {
        fuse.det_max = w.det_max; fuse.det_acc = (const long long *)w.det_acc;
        fuse.det_prev = cfg->det_prev; fuse.det_gex = w.det_gex; fuse.det_onepass = det_one ? 1 : 0;
    }
    if (fuse_b) {
        // the tile backward's blocks left the loss terms (sls_consumer.hip: launch_consumer, no_launch) and the forward
        // its blocks' costs: this launch sums the first and sorts the second for the keyframe's next iteration
        fuse.loss_partials = (const float *)w.consumer_scratch;
        fuse.n_loss_partials = dc.GX * dc.GY * (kTilePix / 16);
        fuse.loss_w[0] = 1.0f / ((float)H * (float)W);
        fuse.loss_w[1] = n_valid > 0 ? cfg->lambda_normal * (1.0f / (float)n_valid) : 0.0f;
        fuse.loss_w[2] = n_valid > 0 ? cfg->lambda_alpha * (1.0f / (float)n_valid) : 0.0f;
        if (order_bwd) { fuse.order_T = dc.GX * dc.GY; fuse.order_cost = w.block_cost; fuse.order_out = cfg->block_order; }
    }
    if (cfg->grad_bitmap && cfg->phase != 2) {      // (phase 2: phase 1 wrote the bitmap early — a superset, left alone)
        fuse.grad_bitmap = cfg->grad_bitmap;
        fuse.grad_bitmap_words = (N + 63) / 64;
    }
    if (cfg->grad_chunk) {
        fuse.gchunk = cfg->grad_chunk;
        fuse.gbase = grads;
        fuse.void_flags = grads + cfg->grad_chunk;
        fuse.void_count = (int)cfg->grad_ranks;
        fuse.void_stride = (int)cfg->grad_chunk + 4;
    }
    const bool aligned = (N % 2 == 0) && ((((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0);
    if (cfg->apply_adam && aligned) {
        fuse.enabled = 1;
        fuse.write_grads = cfg->keep_grads;
        fuse.c = make_adam_coef(cfg->beta1, cfg->beta2, cfg->eps, adam_step);
        fuse.lr_xyz = cfg->lr_xyz; fuse.lr_opacity = cfg->lr_opacity;
        fuse.lr_scaling = cfg->lr_scaling; fuse.lr_rotation = cfg->lr_rotation;
        fuse.exp_avg = exp_avg; fuse.exp_avg_sq = exp_avg_sq;
        fuse.skip_flag = &status_dev->overflow;
    }
    if (cfg->union_bitmap) {
        fuse.union_bitmap = cfg->union_bitmap; fuse.union_prefix = cfg->union_prefix;
        fuse.compact = cfg->grad_compact; fuse.compact_idx = cfg->grad_compact_index; fuse.compact_cap = cfg->grad_compact_capacity;
    }
    rc = launch_preprocess_bwd(dc, 1, cfg->scaling_max, cfg->scaling_max_penalty, N, xyz, scaling_raw, rotation_raw,
                               opacity_raw, w.radii, w.grec, g_xyz, g_sc, g_rot, g_op, st, &fuse, use_pose ? &po : nullptr);
    if (rc) return rc;
    if (cfg->apply_adam && !fuse.enabled) {
        SlsAdamGroup grp[4];
        memset(grp, 0, sizeof(grp));
        float *params[4] = { xyz, opacity_raw, scaling_raw, rotation_raw };
        const size_t offs[4] = { 0, (size_t)3 * N, (size_t)4 * N, (size_t)6 * N };
        const int64_t numel[4] = { (int64_t)3 * N, (int64_t)N, (int64_t)2 * N, (int64_t)4 * N };
        const float lrs[4] = { cfg->lr_xyz, cfg->lr_opacity, cfg->lr_scaling, cfg->lr_rotation };
        for (int k = 0; k < 4; ++k) {
            grp[k].param = params[k];
            grp[k].grad = grads + offs[k];
            grp[k].exp_avg = exp_avg + offs[k];
            grp[k].exp_avg_sq = exp_avg_sq + offs[k];
            grp[k].numel = numel[k];
            grp[k].lr = lrs[k];
        }
        rc = launch_adam(grp, 4, cfg->beta1, cfg->beta2, cfg->eps, adam_step, &status_dev->overflow, st);
        if (rc) return rc;
    }
    return SLS_OK;
}


// ---- keyframe-batched step -----------------------------------------------------------------------------------------
size_t sls_mapping_workspace_bytes_batch(int G, int N, int H, int W, uint64_t R_capacity, const SlsMappingConfig *cfg)
{
    if (G < 1 || G > SLS_MAX_BATCH || N < 0 || H <= 0 || W <= 0) return 0;
    return carve_batch(G, N, H, W, R_capacity, nullptr, !cfg || cfg->deterministic != 0, nullptr);
}

int sls_mapping_step_batch(int G, const SlsKeyframeInputs *kfs, int N, float *xyz, float *scaling_raw, float *rotation_raw,
                           float *opacity_raw, float *grads, float *exp_avg, float *exp_avg_sq, int64_t adam_step,
                           const SlsMappingConfig *cfg, uint64_t R_capacity, void *workspace, size_t workspace_bytes,
                           SlsMappingStatus *status_dev, void *stream)
{
    // (every argument check before the first launch, as in sls_mapping_step)
    SLS_REQUIRE(G >= 1 && G <= SLS_MAX_BATCH, "G: 1 to SLS_MAX_BATCH keyframes");
    SLS_REQUIRE(kfs && cfg && status_dev && workspace, "null pointer");
    SLS_REQUIRE(N > 0, "N must be positive");
    SLS_REQUIRE(xyz && scaling_raw && rotation_raw && opacity_raw && grads, "null pointer");
    SLS_REQUIRE(!cfg->apply_adam || (exp_avg && exp_avg_sq && adam_step >= 1), "Adam state missing");
    SLS_REQUIRE(R_capacity > 0 && R_capacity < (1ull << 32), "bad instance capacity");
    SLS_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    SLS_REQUIRE(cfg->phase == 0 && !cfg->grad_chunk && !cfg->grad_bitmap && !cfg->union_bitmap,
                "a batch is one whole step on the flat bucket: phase 0, no grad_chunk, grad_bitmap or union_bitmap");
    SLS_REQUIRE(cfg->deterministic >= 0 && cfg->deterministic <= 2, "deterministic: 0 off, 1 two launches, 2 one launch with predicted scales");
    const int H = kfs[0].cam.H, W = kfs[0].cam.W;
    SLS_REQUIRE(H > 0 && W > 0, "bad image size");
    for (int g = 0; g < G; ++g) {
        const SlsKeyframeInputs &k = kfs[g];
        SLS_REQUIRE(k.cam.H == H && k.cam.W == W, "the keyframes of a batch share one image size");
        SLS_REQUIRE(k.gt_depth && k.valid && k.col_cs && k.row_cs && k.col_cs_half && k.row_cs_half && k.depth_order,
                    "null per-keyframe pointer");
        SLS_REQUIRE((k.block_order != nullptr) == (kfs[0].block_order != nullptr), "block_order on every keyframe or on none");
        SLS_REQUIRE(k.reuse_depth_order >= 0 && k.reuse_depth_order <= 4, "reuse_depth_order: 0 from scratch, 1..4 repair rounds");
        for (int h = 0; h < g; ++h) {
            SLS_REQUIRE(kfs[h].depth_order != k.depth_order, "two keyframes share one depth_order buffer");
            SLS_REQUIRE(!k.block_order || kfs[h].block_order != k.block_order, "two keyframes share one block_order buffer");
            SLS_REQUIRE(!k.det_prev || kfs[h].det_prev != k.det_prev, "two keyframes share one det_prev buffer");
        }
    }
    SLS_REQUIRE(!cfg->pose_grad, "a batch takes its pose gradients per keyframe: SlsKeyframeInputs.pose_grad");
    PoseOut po;
    bool use_pose;
    {
        float *pg[SLS_MAX_BATCH];
        for (int g = 0; g < G; ++g) pg[g] = kfs[g].pose_grad;
        if (int prc = make_pose_out(G, N, pg, cfg->pose_scratch, cfg->pose_scratch_bytes, &po, &use_pose)) return prc;
    }
    const bool det = cfg->deterministic != 0;
    MapWs ws[SLS_MAX_BATCH];
    const size_t need = carve_batch(G, N, H, W, R_capacity, workspace, det, ws);
    const MapWs &w0 = ws[0];
    if (workspace_bytes < need) {
        set_error("batch workspace too small: %zu < %zu", workspace_bytes, need);
        return SLS_E_SCRATCH;
    }
    hipStream_t st = (hipStream_t)stream;
    const uint32_t cap = (uint32_t)R_capacity;
    const DevCam dc0 = make_devcam(kfs[0].cam);
    const int T = dc0.GX * dc0.GY;
    const bool fuse_b = cfg->depth_ratio == 0.0f && kfs[0].block_order != nullptr;
    const bool order_bwd = T % 32 == 0 && kTileW == 16 && kTileH == 16;
    BatchFuse bf;
    memset(&bf, 0, sizeof(bf));
    bf.G = G;
    // ---- every keyframe's front (forward, loss, tile backward) into its own workspace slice ----------------------------
    for (int g = 0; g < G; ++g) {
        const SlsKeyframeInputs &k = kfs[g];
        const MapWs &w = ws[g];
        SlsMappingConfig kc = *cfg;
        kc.reuse_depth_order = k.reuse_depth_order;
        kc.depth_order = k.depth_order;
        kc.block_order = k.block_order;
        kc.det_prev = k.det_prev;
        kc.deterministic = det ? 1 : 0;          // (the one-launch scheme runs as the two-launch one in a batch)
        if (g > 0) kc.scaling_max_penalty = 0.0f;  // the regulariser once: summed by keyframe 0's preprocess
        int rc = mapping_front(&k.cam, N, xyz, scaling_raw, rotation_raw, opacity_raw, k.gt_depth, k.valid, k.n_valid,
                               k.col_cs, k.row_cs, k.col_cs_half, k.row_cs_half, &kc, cap, w, status_dev + 1 + g, st);
        if (rc) return rc;
        BatchKeyframe &b = bf.kf[g];
        b.cam = make_devcam(k.cam);
        b.radii = w.radii;
        b.grec = (float4 *)w.grec;
        b.touched = w.touched;
        b.status = (uint32_t *)(status_dev + 1 + g);
        if (det) {
            b.det_max = w.det_max; b.det_acc = (long long *)w.det_acc;
            b.det_prev = k.det_prev;     // (det_gex stays null: no launch reads a batch slice's defaults)
        }
        if (fuse_b) {
            b.loss_partials = (const float *)w.consumer_scratch;
            b.loss_w[0] = 1.0f / ((float)H * (float)W);
            b.loss_w[1] = k.n_valid > 0 ? cfg->lambda_normal * (1.0f / (float)k.n_valid) : 0.0f;
            b.loss_w[2] = k.n_valid > 0 ? cfg->lambda_alpha * (1.0f / (float)k.n_valid) : 0.0f;
            if (order_bwd) { b.order_cost = w.block_cost; b.order_out = k.block_order; }
        }
    }
    if (fuse_b) {
        bf.n_loss_partials = T * (kTilePix / 16);
        if (order_bwd) bf.order_T = T;
    }
    // ---- ONE backward of the projection over the batch + Adam -----------------------------------------------------------
    AdamFuse &af = bf.af;
    af.status_src = (uint32_t *)status_dev;
    af.reg_accum = w0.reg_accum;
    af.status_mirror = (uint32_t *)cfg->status_mirror;
    af.void_flags = cfg->void_flags_out;
    const bool aligned = (N % 2 == 0) && ((((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0);
    if (cfg->apply_adam && aligned) {
        af.enabled = 1;
        af.write_grads = cfg->keep_grads;
        af.c = make_adam_coef(cfg->beta1, cfg->beta2, cfg->eps, adam_step);
        af.lr_xyz = cfg->lr_xyz; af.lr_opacity = cfg->lr_opacity;
        af.lr_scaling = cfg->lr_scaling; af.lr_rotation = cfg->lr_rotation;
        af.exp_avg = exp_avg; af.exp_avg_sq = exp_avg_sq;
    }
    float *g_xyz = grads, *g_op = grads + (size_t)3 * N, *g_sc = grads + (size_t)4 * N, *g_rot = grads + (size_t)6 * N;
    int rc = launch_preprocess_bwd_batch(cfg->scaling_max, cfg->scaling_max_penalty, N, xyz, scaling_raw, rotation_raw,
                                         opacity_raw, g_xyz, g_sc, g_rot, g_op, bf, st, use_pose ? &po : nullptr);
    if (rc) return rc;
    if (cfg->apply_adam && !af.enabled) {      // (odd N or unaligned moments: the separate optimiser kernel, as sls_mapping_step)
        SlsAdamGroup grp[4];
        memset(grp, 0, sizeof(grp));
        float *params[4] = { xyz, opacity_raw, scaling_raw, rotation_raw };
        const size_t offs[4] = { 0, (size_t)3 * N, (size_t)4 * N, (size_t)6 * N };
        const int64_t numel[4] = { (int64_t)3 * N, (int64_t)N, (int64_t)2 * N, (int64_t)4 * N };
        const float lrs[4] = { cfg->lr_xyz, cfg->lr_opacity, cfg->lr_scaling, cfg->lr_rotation };
        for (int k = 0; k < 4; ++k) {
            grp[k].param = params[k];
            grp[k].grad = grads + offs[k];
            grp[k].exp_avg = exp_avg + offs[k];
            grp[k].exp_avg_sq = exp_avg_sq + offs[k];
            grp[k].numel = numel[k];
            grp[k].lr = lrs[k];
        }
        rc = launch_adam(grp, 4, cfg->beta1, cfg->beta2, cfg->eps, adam_step, &status_dev->overflow, st);
        if (rc) return rc;
    }
    return SLS_OK;
}

}  // extern "C"

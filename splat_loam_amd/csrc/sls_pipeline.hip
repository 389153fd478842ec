// sls_pipeline.hip — host-side orchestration behind the C-ABI: the two-stage
// forward and the backward of the drop-in rasterizer interface, and
// sls_mapping_step, which enqueues one WHOLE mapping iteration
// (slam/mapper.py:150-204: render -> loss -> backward -> Adam) on a stream with
// no device->host sync and no torch op in between.
#include <stdlib.h>
#include <string.h>

#include "sls_consumer_dev.hpp"
#include "sls_launch.hpp"

namespace sls {

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

// One walk over the workspace, 256-byte aligned pieces
struct Taker {
    char *p; size_t off;
    void *operator()(size_t bytes) { void *r = (void *)(p + off); off += (bytes + 255) & ~(size_t)255; return r; }
};

// ONE keyframe's slice, stated once.  whole: keyframe 0's (or the only one's), a whole workspace — what a front uses and
// leaves behind for nobody (instances, lists, sort scratch, pixel state, maps, dL/dallmap, block masks) is taken here too
// and SHARED by the keyframes of a batch, whose fronts run one after another on the stream.  A further keyframe (!whole,
// w = a copy of keyframe 0's view) gets only what the batched projection backward reads after all fronts: radii, the loss
// stage's scratch (its per-block loss terms), the forward's block costs, the zeroed group, the fixed-point accumulators.
static void carve_keyframe(Taker &take, int N, int H, int W, uint64_t cap, bool deterministic, bool whole, MapWs &w)
{
    const size_t n = (size_t)(N > 0 ? N : 1), P = (size_t)H * W, c = (size_t)(cap > 0 ? cap : 1);
    const int GX = (W + kTileW - 1) / kTileW, GY = (H + kTileH - 1) / kTileH;
    const size_t T = (size_t)GX * GY;
    if (whole) w.rec = (float *)take(n * SLS_REC_STRIDE * 4);
    w.radii = (int32_t *)take(n * 4);
    if (whole) {
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
    }
    w.consumer_scratch = take(w.consumer_scratch_bytes);
    if (whole) w.block_masks = (uint64_t *)take(block_mask_bytes(cap, (int)T));
    else w.block_cost = (uint32_t *)take(T * (kTilePix / 16) * 4);      // (a further keyframe's costs: in front of its zeroed group)
    // zeroed together on the first use of a workspace: [reg_accum | det_gex | tile_consumed | touched | grec]
    w.reg_accum = (float *)take(4);
    w.det_gex = (uint32_t *)take(16 * 4);
    w.tile_consumed = (uint32_t *)take(T * 4);
    w.touched = (uint8_t *)take(n);
    w.grec = (float *)take(n * SLS_GREC_STRIDE * 4);
    w.zero_bytes = (size_t)((char *)w.grec - (char *)w.reg_accum) + n * SLS_GREC_STRIDE * 4;
    if (whole) {
        w.block_cost = (uint32_t *)take(T * (kTilePix / 16) * 4);
        w.block_order = (uint32_t *)take(T * (kTilePix / 16) * 4);
    }
    // deterministic accumulation only (192 B per surfel: as much again as everything per-surfel above)
    if (deterministic) {
        w.det_max = (uint32_t *)take(n * SLS_GREC_STRIDE * 4);
        w.det_acc = (unsigned long long *)take(n * SLS_GREC_STRIDE * 8);
        w.det_bytes = (size_t)((char *)w.det_acc - (char *)w.det_max) + n * SLS_GREC_STRIDE * 8;
    }
}

static MapWs carve(int N, int H, int W, uint64_t cap, void *base, bool deterministic)
{
    MapWs w{};
    Taker take = { (char *)base, 0 };
    carve_keyframe(take, N, H, W, cap, deterministic, true, w);
    w.total = take.off;
    return w;
}

// Workspace of sls_mapping_step_batch: keyframe 0's slice is a whole workspace, the further keyframes' slices follow it.
// w[g] is keyframe g's view; the return value is the total size.
static size_t carve_batch(int G, int N, int H, int W, uint64_t cap, void *base, bool deterministic, MapWs *w)
{
    const MapWs w0 = carve(N, H, W, cap, base, deterministic);
    Taker take = { (char *)base, w0.total };
    for (int g = 0; g < G; ++g) {
        MapWs k = w0;
        if (g > 0) carve_keyframe(take, N, H, W, cap, deterministic, false, k);
        k.total = 0;
        if (w) w[g] = k;
    }
    return take.off;
}

}  // namespace sls

using namespace sls;

extern "C" {

size_t sls_stage1_scratch_bytes(int N) { return order_scratch_bytes(N); }

int sls_forward_stage1(const SlsCamera *cam, int N, const float *means3D, const float *scales,
                       const float *rotations, const float *opacities, const float *col_cs, const float *row_cs,
                       float *rec, int32_t *radii, int32_t *rect, uint32_t *tiles_touched, uint64_t *tile_mask,
                       uint32_t *block_box, float *depth, uint32_t *order, uint32_t *offsets, uint32_t *total_out,
                       void *scratch, size_t scratch_bytes, void *stream)
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
    PreFwdLaunch pf{};
    pf.N = N; pf.means = means3D; pf.scales = scales; pf.rots = rotations; pf.opac = opacities;
    pf.rec = rec; pf.radii = radii; pf.rect = rect; pf.tiles = tiles_touched; pf.depth = depth;
    pf.order_keys = okeys; pf.order_vals = ovals; pf.n_dev = n_dev;
    pf.col_cs = col_cs; pf.row_cs = row_cs; pf.tile_mask = tile_mask; pf.sbox = block_box;
    if (int rc = launch_preprocess_fwd(dc, pf, st)) return rc;
    DepthOrderScan ds{};
    ds.N = N; ds.tiles = tiles_touched; ds.order = order; ds.offsets = offsets; ds.total_out = total_out; ds.scratch = scratch;
    ds.scratch_bytes = scratch_bytes;
    return launch_depth_order_scan(ds, st, nullptr);
}

size_t sls_sort_scratch_bytes(uint64_t R) { return sort_scratch_bytes(R); }
size_t sls_block_mask_bytes(uint64_t R, int H, int W)
{
    return block_mask_bytes(R, ((W + kTileW - 1) / kTileW) * ((H + kTileH - 1) / kTileH));
}

int sls_forward_stage2(const SlsCamera *cam, int N, uint64_t R, const float *rec, const int32_t *rect,
                       const uint32_t *tiles_touched, const uint64_t *tile_mask, const uint32_t *block_box,
                       const float *depth, const uint32_t *order, const uint32_t *offsets, const uint32_t *total_dev,
                       uint32_t *tkeys, uint32_t *vals, uint32_t *tkeys_tmp, uint32_t *vals_tmp, void *sort_scratch,
                       size_t sort_scratch_bytes_, int *sorted_in_tmp, uint64_t *keys64_out, int list_pairs,
                       const uint32_t **sorted_list, int *sorted_stride, uint32_t *ranges, const float *col_cs,
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
        BinDirectLaunch bd{};
        bd.N = N; bd.cap = (uint32_t)R; bd.bmask_mode = list_pairs; bd.db = make_direct_bin(dc, N, sort_scratch, nullptr, false, false);
        bd.order = order; bd.rect = rect; bd.sbox = boxes; bd.scratch = sort_scratch; bd.vals_out = vals; bd.ranges = ranges;
        rc = launch_bin_direct(dc, bd, st, &bmask);
    } else {
        BinSortLaunch bs{};
        bs.N = N; bs.count_ptr = total_dev; bs.cap = (uint32_t)R; bs.order = order; bs.rect = rect; bs.tiles = tiles_touched;
        bs.tile_mask = dc.tile_cull ? tile_mask : nullptr; bs.depth = depth; bs.offsets = offsets; bs.sbox = boxes; bs.bmask_mode = list_pairs;
        bs.tkeys = tkeys; bs.vals = vals; bs.tkeys_tmp = tkeys_tmp; bs.vals_tmp = vals_tmp;
        bs.scratch = sort_scratch; bs.scratch_bytes = sort_scratch_bytes_; bs.ranges = ranges; bs.keys64_out = keys64_out;
        rc = launch_bin_sort(dc, bs, st, sorted_in_tmp, &bmask);
    }
    if (rc) return rc;
    const uint32_t *sorted_vals = *sorted_in_tmp ? vals_tmp : vals;
    *sorted_list = bmask ? (const uint32_t *)bmask : sorted_vals;
    *sorted_stride = bmask ? 2 : 1;
    if (block_masks_shape) *block_masks_shape = block_masks ? 3 : 0;
    RenderFwdLaunch rf{};
    rf.ranges = ranges; rf.vals = sorted_vals; rf.rec = rec; rf.col_cs = col_cs; rf.row_cs = row_cs;
    rf.allmap = allmap; rf.pix_state = pix_state; rf.pix_contrib = pix_contrib; rf.tile_consumed = tile_consumed;
    rf.block_masks = block_masks; rf.lean = (cam->flags & SLS_CAM_LEAN_ALLMAP) != 0; rf.bmask = bmask;
    rf.order_in_handover = true;       // (+ the backward's launch order into the hand-over buffer)
    return launch_render_fwd(dc, rf, st);
}

// ---- pose gradient (D11): the caller's scratch = one arrival counter (a 256-byte slot) + one row per workgroup of the
// projection's backward and keyframe
static size_t pose_scratch_bytes(int G, int N)
{
    // (G times the single keyframe's: one counter is used, the documented size is the simple one)
    return (size_t)G * (256 + (size_t)((N + 255) / 256) * kPoseRow * sizeof(float));
}
size_t sls_pose_grad_scratch_bytes(int N) { return N > 0 ? pose_scratch_bytes(1, N) : 0; }

// Checks a call's pose arguments (before anything is enqueued) and fills the launcher's view of them; po->counter stays
// null where no pose gradient is asked for (pose_grad[g] all null): pose_arg
static int make_pose_out(int G, int N, float *const *pose_grad, void *scratch, size_t scratch_bytes, PoseOut *po)
{
    memset(po, 0, sizeof(*po));
    int n = 0;
    for (int g = 0; g < G; ++g) n += pose_grad[g] ? 1 : 0;
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
static const PoseOut *pose_arg(const PoseOut &po) { return po.counter ? &po : nullptr; }

int sls_backward(const SlsCamera *cam, int N, uint64_t R, const float *means3D, const float *scales,
                 const float *rotations, const int32_t *radii, const float *rec, const uint32_t *ranges,
                 const uint32_t *vals_sorted, int vals_stride, const float *col_cs, const float *row_cs,
                 const float *pix_state, const uint32_t *pix_contrib, const float *dL_dallmap, float *grec,
                 float *dL_dmeans3D, float *dL_dscales, float *dL_drotations, float *dL_dopacities,
                 const uint64_t *block_masks, int block_masks_shape, void *stream)
{
    return sls_backward_pose(cam, N, R, means3D, scales, rotations, radii, rec, ranges, vals_sorted, vals_stride, col_cs,
                             row_cs, pix_state, pix_contrib, dL_dallmap, grec, dL_dmeans3D, dL_dscales, dL_drotations,
                             dL_dopacities, block_masks, block_masks_shape, nullptr, nullptr, 0, stream);
}

int sls_backward_pose(const SlsCamera *cam, int N, uint64_t R, const float *means3D, const float *scales,
                      const float *rotations, const int32_t *radii, const float *rec, const uint32_t *ranges,
                      const uint32_t *vals_sorted, int vals_stride, const float *col_cs, const float *row_cs,
                      const float *pix_state, const uint32_t *pix_contrib, const float *dL_dallmap, float *grec,
                      float *dL_dmeans3D, float *dL_dscales, float *dL_drotations, float *dL_dopacities,
                      const uint64_t *block_masks, int block_masks_shape, float *pose_grad, void *pose_scratch,
                      size_t pose_scratch_bytes_, void *stream)
{
    SLS_REQUIRE(cam, "null pointer");
    SLS_REQUIRE(N >= 0, "negative N");
    if (N == 0) {
        if (pose_grad) SLS_HIP_CHECK(hipMemsetAsync(pose_grad, 0, 6 * sizeof(float), (hipStream_t)stream));
        return SLS_OK;
    }
    PoseOut po;
    if (int prc = make_pose_out(1, N, &pose_grad, pose_scratch, pose_scratch_bytes_, &po)) return prc;
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
        RenderBwdLaunch rb{};
        rb.ranges = ranges; rb.vals = vals_sorted; rb.vals_stride = vals_stride; rb.rec = rec; rb.col_cs = col_cs; rb.row_cs = row_cs;
        rb.pix_state = pix_state; rb.pix_contrib = pix_contrib; rb.dL_dallmap = dL_dallmap;
        rb.block_masks = block_masks_shape ? block_masks : nullptr; rb.block_masks_shape = block_masks_shape;
        rb.lean = (cam->flags & SLS_CAM_LEAN_ALLMAP) != 0;
        rb.grec = grec; rb.order_in_handover = true;
        if (int rc = launch_render_bwd(dc, rb, st)) return rc;
    }
    PreBwdLaunch pb{};
    pb.N = N; pb.means = means3D; pb.scales = scales; pb.rots = rotations; pb.radii = radii; pb.grec = grec;
    pb.dmeans = dL_dmeans3D; pb.dscales = dL_dscales; pb.drots = dL_drotations; pb.dopac = dL_dopacities;
    pb.pose = pose_arg(po);
    return launch_preprocess_bwd(dc, pb, st);
}

size_t sls_backward_det_scratch_bytes(int N) { return N > 0 ? (size_t)N * SLS_GREC_STRIDE * 12 + 256 : 256; }

int sls_backward_det(const SlsCamera *cam, int N, uint64_t R, const float *means3D, const float *scales,
                     const float *rotations, const int32_t *radii, const float *rec, const uint32_t *ranges,
                     const uint32_t *vals_sorted, int vals_stride, const float *col_cs, const float *row_cs,
                     const float *pix_state, const uint32_t *pix_contrib, const float *dL_dallmap, float *dL_dmeans3D,
                     float *dL_dscales, float *dL_drotations, float *dL_dopacities, const uint64_t *block_masks,
                     int block_masks_shape, void *det_scratch, size_t det_scratch_bytes, void *stream)
{
    return sls_backward_det_pose(cam, N, R, means3D, scales, rotations, radii, rec, ranges, vals_sorted, vals_stride,
                                 col_cs, row_cs, pix_state, pix_contrib, dL_dallmap, dL_dmeans3D, dL_dscales,
                                 dL_drotations, dL_dopacities, block_masks, block_masks_shape, det_scratch,
                                 det_scratch_bytes, nullptr, nullptr, 0, stream);
}

int sls_backward_det_pose(const SlsCamera *cam, int N, uint64_t R, const float *means3D, const float *scales,
                          const float *rotations, const int32_t *radii, const float *rec, const uint32_t *ranges,
                          const uint32_t *vals_sorted, int vals_stride, const float *col_cs, const float *row_cs,
                          const float *pix_state, const uint32_t *pix_contrib, const float *dL_dallmap,
                          float *dL_dmeans3D, float *dL_dscales, float *dL_drotations, float *dL_dopacities,
                          const uint64_t *block_masks, int block_masks_shape, void *det_scratch, size_t det_scratch_bytes,
                          float *pose_grad, void *pose_scratch, size_t pose_scratch_bytes_, void *stream)
{
    SLS_REQUIRE(cam, "null pointer");
    SLS_REQUIRE(N >= 0, "negative N");
    if (N == 0) {
        if (pose_grad) SLS_HIP_CHECK(hipMemsetAsync(pose_grad, 0, 6 * sizeof(float), (hipStream_t)stream));
        return SLS_OK;
    }
    PoseOut po;
    if (int prc = make_pose_out(1, N, &pose_grad, pose_scratch, pose_scratch_bytes_, &po)) return prc;
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
        RenderBwdLaunch rb{};
        rb.ranges = ranges; rb.vals = vals_sorted; rb.vals_stride = vals_stride; rb.rec = rec; rb.col_cs = col_cs; rb.row_cs = row_cs;
        rb.pix_state = pix_state; rb.pix_contrib = pix_contrib; rb.dL_dallmap = dL_dallmap;
        rb.block_masks = block_masks_shape ? block_masks : nullptr; rb.block_masks_shape = block_masks_shape;
        rb.lean = (cam->flags & SLS_CAM_LEAN_ALLMAP) != 0;
        rb.det_max = mx; rb.det_acc = acc; rb.order_in_handover = true;
        if (int rc = launch_render_bwd(dc, rb, st)) return rc;
    }
    AdamFuse fuse;
    memset(&fuse, 0, sizeof(fuse));
    fuse.det_max = mx;
    fuse.det_acc = (const long long *)acc;
    PreBwdLaunch pb{};
    pb.N = N; pb.means = means3D; pb.scales = scales; pb.rots = rotations; pb.radii = radii;
    pb.dmeans = dL_dmeans3D; pb.dscales = dL_dscales; pb.drots = dL_drotations; pb.dopac = dL_dopacities;
    pb.fuse = &fuse; pb.pose = pose_arg(po);
    return launch_preprocess_bwd(dc, pb, st);
}

// ---- the binning front: projection -> depth order -> binning -> tile forward -----------------------------------------
// One function for sls_forward_ws and the mapping steps; what differs between them is named here.
struct FrontArgs {
    PreFwdLaunch pf;    // the caller's part: N, parameters (raw + regulariser: the mapping steps), ray tables, where the radii go
    uint32_t *depth_order; int reuse_rounds;        // the camera's own order (null: the workspace's), repaired in so many rounds
    int workspace_ready;
    uint32_t *status_mirror;                        // pinned host memory: the status block, early (sls_forward_ws)
    int list_pairs;                                 // list_pairs / cfg->block_masks: 0 auto, 1 whenever possible, 2 never
    float *allmap; bool lean;                       // (lean: nobody reads the median / distortion planes)
    bool want_backward;                             // leave the backward its blocks' compact lists and their costs
};

static int binning_front(const DevCam &dc, uint32_t cap, const MapWs &w, const FrontArgs &f, SlsMappingStatus *status_dev,
                         hipStream_t st, const uint32_t **sorted_list, int *sorted_stride)
{
    const int N = f.pf.N;
    // (the status block is zeroed by thread 0 of preprocess_fwd, the first kernel)
    if (!f.workspace_ready) {
        // first use of this workspace: the gradient records and the touched marks must start from zero; afterwards the
        // backward of the projection leaves them zeroed behind itself (no 64*N-byte memset per iteration)
        ScopedTimer tm(T_GREC_MEMSET, st);
        SLS_HIP_CHECK(hipMemsetAsync(w.reg_accum, 0, w.zero_bytes, st));
    }
    uint32_t *okeys, *ovals, *n_dev;
    // the depth order lives in the workspace, or in a caller-owned buffer (one per keyframe, so that every
    // keyframe of a window can repair ITS order when the mapper samples keyframes at random)
    uint32_t *order = f.depth_order ? f.depth_order : w.order;
    depth_order_key_buffers(N, w.order_scratch, order, &okeys, &ovals, &n_dev);
    // Repairing the previous order: its first step (sorting windows of the old order by the new keys) rides in the
    // preprocess launch — it needs nothing the preprocess produces
    const bool merged_sort = f.reuse_rounds >= 1;
    // Direct binning (sls_sort.hip) where it applies: no unsorted instance array, no scan of tiles_touched; the preprocess
    // then leaves the emission records in the form its first kernel gathers (rectangle + block box)
    // (the staged API scans the count table's rows with a launch of its own instead of the coarse table)
    const bool direct = bin_direct_possible(dc, N, cap);
    BinDirectLaunch bd{};
    if (direct) bd.db = make_direct_bin(dc, N, w.sort_scratch, (uint2 *)w.serec, merged_sort, true);
    PreFwdLaunch pf = f.pf;
    pf.rec = w.rec; pf.order_vals = ovals; pf.n_dev = n_dev;
    pf.status_clear = (uint32_t *)status_dev; pf.tile_mask = w.tmask; pf.erec = w.erec;
    if (merged_sort) { pf.resort_prev_order = order; pf.resort_comp = resort_comp_buffer(N, w.order_scratch); }
    if (direct) {
        // (the direct binning reads the emission records only — not the rectangles, the tile counts, the depths or the
        //  block boxes as arrays of their own; a repair whose window sort rides in the preprocess launch computes its
        //  keys itself: 32 bytes per surfel that are not written)
        pf.order_keys = merged_sort ? nullptr : okeys;
        pf.erec_box = 1;
        if (bd.db.coarse) { pf.zero_words = bd.db.coarse; pf.n_zero_words = (int)direct_coarse_words(dc, N); }
    } else {
        pf.rect = w.rect; pf.tiles = w.tiles; pf.depth = w.depth; pf.order_keys = okeys; pf.sbox = w.sbox;
    }
    if (int rc = launch_preprocess_fwd(dc, pf, st)) return rc;
    ScanHandoff handoff = { nullptr, 0, nullptr, 0 };   // the binning finishes (or does not need) the scan of tiles_touched
    DepthOrderScan ds{};
    ds.N = N; ds.tiles = w.tiles; ds.order = order; ds.offsets = w.offsets; ds.total_out = &status_dev->R;
    ds.scratch = w.order_scratch; ds.scratch_bytes = w.order_scratch_bytes;
    ds.reuse_order = f.reuse_rounds; ds.fail_flag = &status_dev->overflow; ds.window_sort_done = merged_sort;
    ds.direct = direct ? &bd.db : nullptr; ds.erec_box = (const int4 *)w.erec; ds.GX = dc.GX;
    if (int rc = launch_depth_order_scan(ds, st, &handoff)) return rc;
    int in_tmp = 0, rc;
    const uint2 *bmask = nullptr;
    if (direct) {
        bd.N = N; bd.cap = cap; bd.counted = handoff.counted != 0; bd.order = order; bd.erec_box = w.erec;
        bd.scratch = w.sort_scratch; bd.vals_out = w.vals; bd.ranges = w.ranges;
        bd.total_out = &status_dev->R; bd.overflow = &status_dev->overflow;
        bd.resort_windows = handoff.resort_windows; bd.resort_edges = handoff.resort_edges;
        bd.bmask_mode = f.list_pairs; bd.status_mirror = f.status_mirror;
        rc = launch_bin_direct(dc, bd, st, &bmask);
    } else {
        BinSortLaunch bs{};
        bs.N = N; bs.count_ptr = &status_dev->R; bs.cap = cap; bs.order = order; bs.rect = w.rect; bs.tiles = w.tiles;
        bs.tile_mask = dc.tile_cull ? w.tmask : nullptr; bs.erec = (dc.GX < 65536 && dc.GY < 65536) ? w.erec : nullptr;
        bs.depth = w.depth; bs.offsets = w.offsets; bs.sbox = w.sbox; bs.bmask_mode = f.list_pairs;
        bs.tkeys = w.tkeys; bs.vals = w.vals; bs.tkeys_tmp = w.tkeys_tmp; bs.vals_tmp = w.vals_tmp;
        bs.scratch = w.sort_scratch; bs.scratch_bytes = w.sort_scratch_bytes; bs.ranges = w.ranges;
        bs.overflow = &status_dev->overflow; bs.handoff = &handoff; bs.total_out = &status_dev->R;
        rc = launch_bin_sort(dc, bs, st, &in_tmp, &bmask);
    }
    if (rc) return rc;
    // (with the pairs the plain value arrays are not written: the list IS the pairs, two words apart)
    *sorted_list = bmask ? (const uint32_t *)bmask : (in_tmp ? w.vals_tmp : w.vals);
    *sorted_stride = bmask ? 2 : 1;
    RenderFwdLaunch rf{};
    rf.ranges = w.ranges; rf.vals = *sorted_list; rf.rec = w.rec; rf.col_cs = pf.col_cs; rf.row_cs = pf.row_cs;
    rf.allmap = f.allmap; rf.pix_state = w.pix_state; rf.pix_contrib = w.pix_contrib; rf.lean = f.lean; rf.bmask = bmask;
    rf.consumed_zeroed = true;          // (nobody reads the consumed counters here)
    if (f.want_backward) { rf.block_masks = w.block_masks; rf.block_cost = w.block_cost; }
    return launch_render_fwd(dc, rf, st);
}

// ---- the drop-in forward without the host read of R --------------------------------------------------------------
// (the status block — R, void bits — reaches the caller's pinned host mirror from the first workgroup of bin_direct)
size_t sls_forward_ws_bytes(int N, int H, int W, uint64_t R_capacity)
{
    return (N < 0 || H <= 0 || W <= 0) ? 0 : carve(N, H, W, R_capacity, nullptr, false).total;
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
    FrontArgs f{};
    f.pf.N = N; f.pf.means = means3D; f.pf.scales = scales; f.pf.rots = rotations; f.pf.opac = opacities;
    f.pf.col_cs = col_cs; f.pf.row_cs = row_cs; f.pf.radii = radii;
    f.depth_order = depth_order; f.reuse_rounds = reuse_rounds; f.workspace_ready = workspace_ready;
    f.status_mirror = (uint32_t *)status_mirror;      // (the status block leaves from the binning's first workgroup)
    f.list_pairs = list_pairs; f.allmap = allmap; f.lean = (cam->flags & SLS_CAM_LEAN_ALLMAP) != 0;
    // a forward nobody differentiates (render() under no_grad: Mapper.densify, the tracker) writes no hand-over; one
    // that is leaves the backward its blocks' compact lists and their costs (sorted into the camera's launch order by
    // passengers of the backward's last kernel, for the camera's NEXT backward: as sls_mapping_step does)
    f.want_backward = want_backward != 0;
    *block_masks_shape = want_backward ? 3 : 0;
    return binning_front(dc, cap, w, f, status_dev, (hipStream_t)stream, sorted_list, sorted_stride);
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
    if (int prc = make_pose_out(1, N, &pose_grad, pose_scratch, pose_scratch_bytes_, &po)) return prc;
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
    const bool order_bwd = block_order != nullptr && block_masks_shape == 3 && launch_order_possible(T);
    // (the launcher walks the forward's compact lists only when block_masks_shape is 3, otherwise the backward culls the
    //  tiles' lists itself; the kernel's tag check is a last guard against a FOREIGN buffer, which the workspace lease
    //  rules out on this path)
    RenderBwdLaunch rb{};
    rb.ranges = w.ranges; rb.vals = sorted_list; rb.vals_stride = sorted_stride; rb.rec = w.rec; rb.col_cs = col_cs; rb.row_cs = row_cs;
    rb.pix_state = w.pix_state; rb.pix_contrib = w.pix_contrib; rb.dL_dallmap = dL_dallmap;
    rb.block_masks = block_masks_shape ? w.block_masks : nullptr; rb.block_masks_shape = block_masks_shape;
    rb.lean = (cam->flags & SLS_CAM_LEAN_ALLMAP) != 0;
    rb.grec = w.grec; rb.touched = w.touched;
    if (order_bwd) { rb.block_order = block_order; rb.order_tag = block_order_tag(T); }
    if (int rc = launch_render_bwd(dc, rb, st)) return rc;
    AdamFuse fuse;
    memset(&fuse, 0, sizeof(fuse));
    fuse.clear_grec = 1;
    fuse.touched = w.touched;
    if (order_bwd) { fuse.order_T = T; fuse.order_cost = w.block_cost; fuse.order_out = block_order; }
    PreBwdLaunch pb{};
    pb.N = N; pb.means = means3D; pb.scales = scales; pb.rots = rotations; pb.radii = radii; pb.grec = w.grec;
    pb.dmeans = dL_dmeans3D; pb.dscales = dL_dscales; pb.drots = dL_drotations; pb.dopac = dL_dopacities;
    pb.fuse = &fuse; pb.pose = pose_arg(po);
    return launch_preprocess_bwd(dc, pb, st);
}

// What a step's configuration comes to, derived ONCE per step and handed to mapping_front
struct StepSwitches {
    bool det, det_one;      // deterministic accumulation; in ONE launch with predicted scales, on the forward's compact lists
    bool fuse_c, fuse_b;    // depth_ratio = 0: the consumer's second kernel is folded into the backward tile kernel (its pixel
                            // blocks compute dL/dallmap from kernel B's planes), with the keyframe's launch-order buffer B's too
    bool order_bwd;         // the backward's blocks are launched most expensive first (cost recorded by the forward, sorted per XCD
                            // by eight passenger workgroups of the consumer's launch, or with fuse_b of the iteration's last)
};
static StepSwitches step_switches(const SlsMappingConfig *cfg, int deterministic, bool have_det_prev, bool have_block_order, int T)
{
    StepSwitches s;
    s.det = deterministic != 0;
    s.det_one = deterministic == 2 && have_det_prev;
    s.fuse_c = cfg->depth_ratio == 0.0f;
    s.fuse_b = s.fuse_c && have_block_order;
    s.order_bwd = launch_order_possible(T);
    return s;
}

// the three loss weights of the status block's sums: 1 / pixels, lambda_n / valid pixels, lambda_a / valid pixels
static void loss_weights(const SlsMappingConfig *cfg, int H, int W, int n_valid, float *lw)
{
    lw[0] = 1.0f / ((float)H * (float)W);
    lw[1] = n_valid > 0 ? cfg->lambda_normal * (1.0f / (float)n_valid) : 0.0f;
    lw[2] = n_valid > 0 ? cfg->lambda_alpha * (1.0f / (float)n_valid) : 0.0f;
}

// What both steps' projection backward takes from the step: the status block it publishes, and Adam fused into it —
// where N is even and the moments are 16-byte aligned
static void fill_step_fuse(AdamFuse &af, const SlsMappingConfig *cfg, SlsMappingStatus *status_dev, float *reg_accum, int N,
                           float *exp_avg, float *exp_avg_sq, int64_t adam_step)
{
    static_assert(sizeof(SlsMappingStatus) == 32, "the mirror copy moves 8 words");
    af.status_src = (uint32_t *)status_dev; af.status_mirror = (uint32_t *)cfg->status_mirror;
    af.reg_accum = reg_accum; af.void_flags = cfg->void_flags_out;
    const bool aligned = (N % 2 == 0) && ((((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0);
    if (!cfg->apply_adam || !aligned) return;
    af.enabled = 1;
    af.write_grads = cfg->keep_grads;
    af.adam = make_surfel_adam(exp_avg, exp_avg_sq, cfg->lr_xyz, cfg->lr_opacity, cfg->lr_scaling, cfg->lr_rotation, cfg->beta1,
                               cfg->beta2, cfg->eps, adam_step);
}

// ... and elsewhere (odd N or unaligned moments) the separate optimiser kernel over the flat bucket's four groups
static int fallback_adam(const SlsMappingConfig *cfg, int N, float *xyz, float *scaling_raw, float *rotation_raw,
                         float *opacity_raw, float *grads, float *exp_avg, float *exp_avg_sq, int64_t adam_step,
                         const uint32_t *skip_flag, hipStream_t st)
{
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
    return launch_adam(grp, 4, cfg->beta1, cfg->beta2, cfg->eps, adam_step, skip_flag, st, nullptr, nullptr, nullptr);
}

// The front of an iteration (forward, loss, tile backward) on ONE keyframe, into ONE workspace slice: sls_mapping_step
// and, per keyframe, sls_mapping_step_batch
static int mapping_front(const SlsCamera *cam, int N, const float *xyz, const float *scaling_raw, const float *rotation_raw,
                         const float *opacity_raw, const float *gt_depth, const uint8_t *valid, int n_valid,
                         const float *col_cs, const float *row_cs, const float *col_cs_half, const float *row_cs_half,
                         const SlsMappingConfig *cfg, const StepSwitches &sw, uint32_t cap, const MapWs &w,
                         SlsMappingStatus *status_dev, hipStream_t st)
{
    const DevCam dc = make_devcam(*cam);
    const int T = dc.GX * dc.GY;
    // ---- forward ---------------------------------------------------------------
    FrontArgs f{};
    f.pf.N = N; f.pf.raw = 1; f.pf.smax = cfg->scaling_max; f.pf.pen = cfg->scaling_max_penalty; f.pf.reg_out = w.reg_accum;
    f.pf.means = xyz; f.pf.scales = scaling_raw; f.pf.rots = rotation_raw; f.pf.opac = opacity_raw;
    f.pf.col_cs = col_cs; f.pf.row_cs = row_cs; f.pf.radii = w.radii;
    f.depth_order = cfg->depth_order; f.reuse_rounds = cfg->reuse_depth_order; f.workspace_ready = cfg->workspace_ready;
    f.list_pairs = cfg->block_masks; f.allmap = w.allmap;
    f.lean = sw.fuse_c;                 // (the median / distortion planes are not tracked then)
    f.want_backward = true;
    const uint32_t *sorted_vals; int vals_stride;
    if (int rc = binning_front(dc, cap, w, f, status_dev, st, &sorted_vals, &vals_stride)) return rc;
    // ---- loss + dL/dallmap --------------------------------------------------------
    // With the keyframe's own launch-order buffer kernel B is folded in as well (fuse_b): the loss stage has no
    // launch; the order the backward walks is the one the keyframe's previous iteration left.
    ConsumerArgs cargs, cl{};
    cl.H = cam->H; cl.W = cam->W; cl.allmap = w.allmap; cl.gt_depth = gt_depth; cl.valid = valid;
    cl.col_h = (const float2 *)col_cs_half; cl.row_h = (const float2 *)row_cs_half;
    cl.depth_ratio = cfg->depth_ratio; cl.lambda_n = cfg->lambda_normal; cl.lambda_a = cfg->lambda_alpha;
    cl.sums = status_dev->loss_sums; cl.dL_dallmap = w.dL_dallmap;
    cl.order_tiles = sw.order_bwd ? T : 0; cl.block_cost = w.block_cost; cl.block_order = w.block_order;
    if (int rc = launch_consumer(cl, n_valid, w.consumer_scratch, w.consumer_scratch_bytes, sw.fuse_b, st,
                                 sw.fuse_c ? &cargs : nullptr)) return rc;
    // ---- backward -----------------------------------------------------------------
    // (two launches: both accumulators start from zero; one launch: det_acc is left zeroed by every deterministic
    //  iteration's preprocess_bwd where it was written — and the first deterministic iteration on a workspace is a
    //  two-launch one, which also sets the fields' default scales)
    if (sw.det && !sw.det_one) SLS_HIP_CHECK(hipMemsetAsync(w.det_max, 0, w.det_bytes, st));
    RenderBwdLaunch rb{};
    rb.ranges = w.ranges; rb.vals = sorted_vals; rb.vals_stride = vals_stride; rb.rec = w.rec; rb.col_cs = col_cs; rb.row_cs = row_cs;
    rb.pix_state = w.pix_state; rb.pix_contrib = w.pix_contrib; rb.dL_dallmap = w.dL_dallmap; rb.grec = w.grec;
    rb.block_masks = w.block_masks; rb.block_masks_shape = 3;
    rb.lean = sw.fuse_c;                // the consumer's dL/d(median, distortion) are 0 then
    rb.touched = w.touched;             // (the backward tile kernel marks the surfels it reaches)
    rb.fused_consumer = sw.fuse_c ? &cargs : nullptr; rb.consumer_b_inline = sw.fuse_b;
    rb.det_max = (sw.det && !sw.det_one) ? w.det_max : nullptr; rb.det_acc = sw.det ? w.det_acc : nullptr;
    rb.det_prev = sw.det_one ? cfg->det_prev : nullptr; rb.det_gex = w.det_gex; rb.det_flag = &status_dev->overflow;
    if (sw.order_bwd) rb.block_order = sw.fuse_b ? cfg->block_order : w.block_order;
    if (sw.fuse_b && sw.order_bwd) rb.order_tag = block_order_tag(T);
    if (int rc = launch_render_bwd(dc, rb, st)) return rc;
    if (cfg->phase == 1 && cfg->grad_bitmap)      // the bitmap EARLY: an all-gather of it can overlap phase 2
        return launch_touched_bitmap(N, w.touched, scaling_raw, cfg->scaling_max, cfg->scaling_max_penalty,
                                     (const uint32_t *)status_dev, cfg->grad_bitmap, st);
    return SLS_OK;
}

size_t sls_mapping_workspace_bytes(int N, int H, int W, uint64_t R_capacity)
{
    return (N < 0 || H <= 0 || W <= 0) ? 0 : carve(N, H, W, R_capacity, nullptr, true).total;   // fits either setting of cfg->deterministic
}

size_t sls_block_order_bytes(int H, int W)
{
    if (H <= 0 || W <= 0) return 0;
    const size_t T = (size_t)((W + kTileW - 1) / kTileW) * (size_t)((H + kTileH - 1) / kTileH);
    return sizeof(uint32_t) * (1 + T * (size_t)(kTilePix / 16));
}

size_t sls_mapping_workspace_bytes_cfg(int N, int H, int W, uint64_t R_capacity, const SlsMappingConfig *cfg)
{
    return (N < 0 || H <= 0 || W <= 0) ? 0 : carve(N, H, W, R_capacity, nullptr, !cfg || cfg->deterministic != 0).total;
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
    {
        float *pg = cfg->pose_grad;
        if (int prc = make_pose_out(1, N, &pg, cfg->pose_scratch, cfg->pose_scratch_bytes, &po)) return prc;
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
    SLS_REQUIRE(cfg->deterministic >= 0 && cfg->deterministic <= 2, "deterministic: 0 off, 1 two launches, 2 one launch with predicted scales");
    SLS_REQUIRE(cfg->deterministic != 2 || cfg->det_prev, "deterministic = 2 needs the keyframe's det_prev buffer");
    const int T = dc.GX * dc.GY;
    const StepSwitches sw = step_switches(cfg, cfg->deterministic, cfg->det_prev != nullptr, cfg->block_order != nullptr, T);
    int rc = SLS_OK;
    if (cfg->phase != 2)
        rc = mapping_front(cam, N, xyz, scaling_raw, rotation_raw, opacity_raw, gt_depth, valid, n_valid, col_cs, row_cs,
                           col_cs_half, row_cs_half, cfg, sw, cap, w, status_dev, st);
    if (rc || cfg->phase == 1) return rc;
    // ---- backward of the projection + optimiser -------------------------------------------
    // One keyframe per step: the Adam update is applied to each surfel right where its gradient is
    // produced (no gradient bucket round trip, no second pass over the parameters).
    AdamFuse fuse;
    memset(&fuse, 0, sizeof(fuse));
    fill_step_fuse(fuse, cfg, status_dev, w.reg_accum, N, exp_avg, exp_avg_sq, adam_step);
    if (fuse.enabled) fuse.skip_flag = &status_dev->overflow;
    fuse.clear_grec = 1;
    fuse.touched = w.touched;
    fuse.void_count = 1; fuse.void_stride = 0;
    if (sw.det) {
        fuse.det_max = w.det_max; fuse.det_acc = (const long long *)w.det_acc;
        fuse.det_prev = cfg->det_prev; fuse.det_gex = w.det_gex; fuse.det_onepass = sw.det_one ? 1 : 0;
    }
    if (sw.fuse_b) {
        // the tile backward's blocks left the loss terms (sls_consumer.hip: launch_consumer, no_launch) and the forward
        // its blocks' costs: this launch sums the first and sorts the second for the keyframe's next iteration
        fuse.loss_partials = (const float *)w.consumer_scratch;
        fuse.n_loss_partials = T * (kTilePix / 16);
        loss_weights(cfg, H, W, n_valid, fuse.loss_w);
        if (sw.order_bwd) { fuse.order_T = T; fuse.order_cost = w.block_cost; fuse.order_out = cfg->block_order; }
    }
    // (phase 2: phase 1 wrote the bitmap early — a superset, left alone)
    if (cfg->grad_bitmap && cfg->phase != 2) { fuse.grad_bitmap = cfg->grad_bitmap; fuse.grad_bitmap_words = (N + 63) / 64; }
    if (cfg->grad_chunk) {
        fuse.gchunk = cfg->grad_chunk; fuse.gbase = grads;
        fuse.void_flags = grads + cfg->grad_chunk; fuse.void_count = (int)cfg->grad_ranks; fuse.void_stride = (int)cfg->grad_chunk + 4;
    }
    if (cfg->union_bitmap) {
        fuse.union_bitmap = cfg->union_bitmap; fuse.union_prefix = cfg->union_prefix;
        fuse.compact = cfg->grad_compact; fuse.compact_idx = cfg->grad_compact_index; fuse.compact_cap = cfg->grad_compact_capacity;
    }
    PreBwdLaunch pb{};
    pb.N = N; pb.raw = 1; pb.smax = cfg->scaling_max; pb.pen = cfg->scaling_max_penalty;
    pb.means = xyz; pb.scales = scaling_raw; pb.rots = rotation_raw; pb.opac = opacity_raw; pb.radii = w.radii; pb.grec = w.grec;
    // flat gradient bucket: [xyz 3N | opacity N | scaling 2N | rotation 4N] (optimizer group order)
    pb.dmeans = grads; pb.dopac = grads + (size_t)3 * N; pb.dscales = grads + (size_t)4 * N; pb.drots = grads + (size_t)6 * N;
    pb.fuse = &fuse; pb.pose = pose_arg(po);
    rc = launch_preprocess_bwd(dc, pb, st);
    if (rc || !cfg->apply_adam || fuse.enabled) return rc;
    return fallback_adam(cfg, N, xyz, scaling_raw, rotation_raw, opacity_raw, grads, exp_avg, exp_avg_sq, adam_step,
                         &status_dev->overflow, st);
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
    {
        float *pg[SLS_MAX_BATCH];
        for (int g = 0; g < G; ++g) pg[g] = kfs[g].pose_grad;
        if (int prc = make_pose_out(G, N, pg, cfg->pose_scratch, cfg->pose_scratch_bytes, &po)) return prc;
    }
    const bool det = cfg->deterministic != 0;
    MapWs ws[SLS_MAX_BATCH];
    const size_t need = carve_batch(G, N, H, W, R_capacity, workspace, det, ws);
    if (workspace_bytes < need) {
        set_error("batch workspace too small: %zu < %zu", workspace_bytes, need);
        return SLS_E_SCRATCH;
    }
    hipStream_t st = (hipStream_t)stream;
    const uint32_t cap = (uint32_t)R_capacity;
    const DevCam dc0 = make_devcam(kfs[0].cam);
    const int T = dc0.GX * dc0.GY;
    // (the one-launch deterministic scheme runs as the two-launch one in a batch)
    const StepSwitches sw = step_switches(cfg, det ? 1 : 0, false, kfs[0].block_order != nullptr, T);
    BatchFuse bf;
    memset(&bf, 0, sizeof(bf));
    bf.G = G;
    // ---- every keyframe's front (forward, loss, tile backward) into its own workspace slice ----------------------------
    for (int g = 0; g < G; ++g) {
        const SlsKeyframeInputs &k = kfs[g];
        const MapWs &w = ws[g];
        SlsMappingConfig kc = *cfg;
        kc.reuse_depth_order = k.reuse_depth_order; kc.depth_order = k.depth_order;
        kc.block_order = k.block_order; kc.det_prev = k.det_prev; kc.deterministic = det ? 1 : 0;
        if (g > 0) kc.scaling_max_penalty = 0.0f;  // the regulariser once: summed by keyframe 0's preprocess
        int rc = mapping_front(&k.cam, N, xyz, scaling_raw, rotation_raw, opacity_raw, k.gt_depth, k.valid, k.n_valid,
                               k.col_cs, k.row_cs, k.col_cs_half, k.row_cs_half, &kc, sw, cap, w, status_dev + 1 + g, st);
        if (rc) return rc;
        BatchKeyframe &b = bf.kf[g];
        b.cam = make_devcam(k.cam);
        b.radii = w.radii; b.grec = (float4 *)w.grec; b.touched = w.touched;
        b.status = (uint32_t *)(status_dev + 1 + g);
        if (det) {
            b.det_max = w.det_max; b.det_acc = (long long *)w.det_acc;
            b.det_prev = k.det_prev;     // (det_gex stays null: no launch reads a batch slice's defaults)
        }
        if (sw.fuse_b) {
            b.loss_partials = (const float *)w.consumer_scratch;
            loss_weights(cfg, H, W, k.n_valid, b.loss_w);
            if (sw.order_bwd) { b.order_cost = w.block_cost; b.order_out = k.block_order; }
        }
    }
    if (sw.fuse_b) {
        bf.n_loss_partials = T * (kTilePix / 16);
        if (sw.order_bwd) bf.order_T = T;
    }
    // ---- ONE backward of the projection over the batch + Adam -----------------------------------------------------------
    AdamFuse &af = bf.af;
    fill_step_fuse(af, cfg, status_dev, ws[0].reg_accum, N, exp_avg, exp_avg_sq, adam_step);
    PreBwdLaunch pb{};
    pb.N = N; pb.raw = 1; pb.smax = cfg->scaling_max; pb.pen = cfg->scaling_max_penalty;
    pb.means = xyz; pb.scales = scaling_raw; pb.rots = rotation_raw; pb.opac = opacity_raw;
    pb.dmeans = grads; pb.dopac = grads + (size_t)3 * N; pb.dscales = grads + (size_t)4 * N; pb.drots = grads + (size_t)6 * N;
    pb.pose = pose_arg(po);
    int rc = launch_preprocess_bwd_batch(pb, bf, st);
    if (rc || !cfg->apply_adam || af.enabled) return rc;
    return fallback_adam(cfg, N, xyz, scaling_raw, rotation_raw, opacity_raw, grads, exp_avg, exp_avg_sq, adam_step,
                         &status_dev->overflow, st);
}

}  // extern "C"

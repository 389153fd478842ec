// sls_api.hip — the extern "C" boundary (include/sls_abi.h), host helpers,
// fused Adam (P6) and the device self-test.
#include <float.h>
#include <math.h>
#include <stdarg.h>
#include <string.h>

#include <mutex>

#include "sls_consumer_dev.hpp"
#include "sls_launch.hpp"
#include "../../include/sls_smooth_math.h"
#include "../../include/sls_cluster_math.h"

namespace sls {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// Diagnostic switches are per PROCESS (sls_common.hpp: DebugState): torch runs a backward node on its autograd
// device thread, not on the thread that called sls_debug_wave_cycles, so per-thread state would silently not reach
// sls_backward under loss.backward().  They are tuning aids only: the data path keeps no mutable state of its own.
DebugState &debug_state()
{
    static DebugState s;
    return s;
}

// ---------------------------------------------------------------------------
// per-kernel timing (HIP events on the launch stream)
// ---------------------------------------------------------------------------
static const char *kTimerNames[T_COUNT] = {
    "preprocess_fwd", "scan", "emit_keys", "sort_hist", "sort_rowscan", "sort_scatter", "tile_ranges",
    "render_fwd", "grec_memset", "render_bwd", "preprocess_bwd", "adam", "knn", "consumer", "resort", "bin_count", "bin_direct",
    "simp_cluster", "simp_faces", "simp_corners", "simp_place", "smooth_adjacency", "smooth_step"
};
constexpr int kTimerPool = 8192;
struct TimerState {
    bool enabled = false;
    int mode = 0;          // 1: every launch, 2: the two tile kernels only, 3: render_bwd only, 4: every 8th render_bwd
    int seen = 0;          // mode 4: render_bwd launches met since the mode was set
    int used = 0;
    int open = -1;         // index of the pair whose start was recorded and whose stop is pending
    int created = 0;
    hipEvent_t start[kTimerPool], stop[kTimerPool];
    int slot[kTimerPool];
};
// ONE recorder per process (allocated on first use), guarded by a mutex: a backward that torch's autograd engine
// runs on its own device thread records into the recorder the Python thread enabled (a per-thread recorder would
// silently miss render_bwd / preprocess_bwd in every autograd-driven mode).  Launches of one stream are enqueued
// in order, so begin/end pairs of different threads do not interleave inside a stream.
static TimerState *t_timer = nullptr;
static std::mutex g_timer_mutex;
static std::atomic<bool> g_timer_on{false};
#define g_timer (*t_timer)

static inline bool timer_wants(int slot)
{
    if (!t_timer || !g_timer.enabled) return false;
    if (g_timer.mode == 1) return true;
    if (g_timer.mode == 2) return slot == T_RENDER_FWD || slot == T_RENDER_BWD;
    return slot == T_RENDER_BWD;
}
// begin reserves an event pair and hands its index back through the ScopedTimer (slot field reused: -1 = untimed)
void timer_begin(int slot, hipStream_t st)
{
    if (!g_timer_on.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lk(g_timer_mutex);
    if (!timer_wants(slot) || g_timer.used >= g_timer.created) return;
    // mode 4 samples the launches: an event pair per launch costs the host a few microseconds of an iteration that
    // is host-bound, so a timed region that wants an undisturbed clock AND a live duration brackets one launch in 8
    if (g_timer.mode == 4 && (g_timer.seen++ & 7) != 0) return;
    g_timer.slot[g_timer.used] = slot;
    (void)hipEventRecord(g_timer.start[g_timer.used], st);
    g_timer.open = g_timer.used;
}
void timer_end(int slot, hipStream_t st)
{
    if (!g_timer_on.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lk(g_timer_mutex);
    if (!timer_wants(slot) || g_timer.used >= g_timer.created || g_timer.open != g_timer.used) return;
    (void)hipEventRecord(g_timer.stop[g_timer.used], st);
    g_timer.open = -1;
    ++g_timer.used;
}

// ---------------------------------------------------------------------------
// P6 fused Adam: every parameter tensor of the model in ONE launch.
// HBM-bound: 16 B read + 12 B written per element.
// ---------------------------------------------------------------------------
constexpr int kMaxAdamGroups = 8;
struct AdamArgs {
    SlsAdamGroup g[kMaxAdamGroups];
    int64_t unit_end[kMaxAdamGroups];   // prefix of ceil(numel/4) units
    int ngroups;
    AdamCoef c;
};

// void_flags (keyframe-parallel mode): two floats that rode the gradient all-reduce, > 0 if ANY rank
// voided the iteration (instance buffers too small / another reason); the reduced bits are also
// written to *status_word so that the caller's one status read sees them.
__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a, int64_t total_units,
                                                   const uint32_t *__restrict__ skip_flag,
                                                   const float *__restrict__ void_flags,
                                                   uint32_t *status_block, uint32_t *status_mirror)
{
    if (void_flags) {
        const uint32_t bits = (void_flags[0] > 0.0f ? 1u : 0u) | (void_flags[1] > 0.0f ? 2u : 0u);
        if (blockIdx.x == 0 && threadIdx.x == 0 && status_block) {
            status_block[1] = bits;                       // SlsMappingStatus.overflow: the group's verdict
            if (status_mirror) mirror_status_block(status_block, status_mirror, true, bits);
        }
        if (bits) return;
    }
    if (skip_flag && *skip_flag) return;   // e.g. the instance buffers overflowed: gradients are incomplete
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total_units; u += (int64_t)gridDim.x * 256) {
        int gi = 0;
#pragma unroll
        for (int k = 0; k < kMaxAdamGroups - 1; ++k)
            if (k < a.ngroups - 1 && u >= a.unit_end[k]) gi = k + 1;
        const SlsAdamGroup grp = a.g[gi];
        const int64_t e0 = (u - (gi ? a.unit_end[gi - 1] : 0)) * 4;
        const float step_size = grp.lr * __builtin_amdgcn_rcpf(a.c.bc1);   // (as the fused update in preprocess_bwd)
        const bool vec = (e0 + 4 <= grp.numel) &&
                         ((((uintptr_t)grp.param | (uintptr_t)grp.grad | (uintptr_t)grp.exp_avg | (uintptr_t)grp.exp_avg_sq) & 15) == 0);
        if (vec) {
            float4 p = *reinterpret_cast<float4 *>(grp.param + e0);
            const float4 g = *reinterpret_cast<const float4 *>(grp.grad + e0);
            float4 m = *reinterpret_cast<float4 *>(grp.exp_avg + e0);
            float4 v = *reinterpret_cast<float4 *>(grp.exp_avg_sq + e0);
            adam_one(p.x, g.x, m.x, v.x, step_size, a.c);
            adam_one(p.y, g.y, m.y, v.y, step_size, a.c);
            adam_one(p.z, g.z, m.z, v.z, step_size, a.c);
            adam_one(p.w, g.w, m.w, v.w, step_size, a.c);
            *reinterpret_cast<float4 *>(grp.param + e0) = p;
            *reinterpret_cast<float4 *>(grp.exp_avg + e0) = m;
            *reinterpret_cast<float4 *>(grp.exp_avg_sq + e0) = v;
        } else {
            for (int64_t e = e0; e < e0 + 4 && e < grp.numel; ++e) {
                float p = grp.param[e], m = grp.exp_avg[e], v = grp.exp_avg_sq[e];
                adam_one(p, grp.grad[e], m, v, step_size, a.c);
                grp.param[e] = p; grp.exp_avg[e] = m; grp.exp_avg_sq[e] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// device self-test of the wave64 primitives the kernels rely on
// ---------------------------------------------------------------------------
__global__ void selftest_kernel(int *out)
{
    const int lane = threadIdx.x & 63;
    int bad = 0;
    // DPP sum: lanes hold (lane+1) * 0.5 -> total 1040 at lane 63
    const float tot = wave_sum_to_lane63(0.5f * (float)(lane + 1));
    if (lane == 63 && tot != 1040.0f) bad |= 1;
    // asymmetric pattern: only lanes 5 and 40 non-zero
    const float t2 = wave_sum_to_lane63(lane == 5 ? 3.0f : (lane == 40 ? 11.0f : 0.0f));
    if (lane == 63 && t2 != 14.0f) bad |= 2;
    // ballot / popcount ranking
    const uint64_t bal = __ballot((lane % 3) == 0);
    if (__popcll(bal) != 22) bad |= 4;
    if (lane_id() != lane) bad |= 8;
    const uint64_t lt = (1ull << lane) - 1ull;
    if ((lane % 3) == 0 && (int)__popcll(bal & lt) != lane / 3) bad |= 16;
    // 16-way reduce-scatter of the backward tile kernel: x[k] = (lane+1)(k+1)/4; lane (pixel p, slot s) gets
    // component p summed over the 16 lanes of slot s
    v2f x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = mk2(0.25f * (float)((lane + 1) * (2 * k + 1)), 0.25f * (float)((lane + 1) * (2 * k + 2)));
    const float b16 = block_reduce16_pk(x, lane);
    if (b16 != (float)(124 + 4 * (lane & 3)) * (float)((lane >> 2) + 1)) bad |= 256;
    if (dpp_xor4((float)lane) != (float)(lane ^ 4)) bad |= 512;
    int xa, xb, ya, yb;
    const uint64_t mm = __ballot(lane == 10 || lane == 29 || lane == 52);   // (2,1) (5,3) (4,6)
    if (!mask_bbox8x8(mm, xa, xb, ya, yb) || xa != 2 || xb != 5 || ya != 1 || yb != 6) bad |= 128;
    if (bad) atomicOr(out, bad);
}

}  // namespace sls

using namespace sls;

extern "C" {

const char *sls_last_error(void) { return g_err; }
int sls_version(void) { return 100; }
int sls_tile_w(void) { return kTileW; }
int sls_tile_h(void) { return kTileH; }
int sls_rec_stride(void) { return SLS_REC_STRIDE; }
int sls_grec_stride(void) { return SLS_GREC_STRIDE; }

int sls_camera_from_matrices(const float *view, const float *proj, int H, int W, float scale_modifier,
                             SlsCamera *out)
{
    SLS_REQUIRE(view && proj && out, "null pointer");
    SLS_REQUIRE(H > 0 && W > 0, "image size must be positive");
    memset(out, 0, sizeof(*out));
    out->H = H; out->W = W;
    // K = proj[:3,:3]^T  (scene/cameras.py:47-50), row-major proj[r*4+c]
    const float k01 = proj[1 * 4 + 0], k10 = proj[0 * 4 + 1];
    SLS_REQUIRE(k01 == 0.0f && k10 == 0.0f, "skewed intrinsics are not supported");
    out->fx = proj[0 * 4 + 0];
    out->fy = proj[1 * 4 + 1];
    out->cx = proj[2 * 4 + 0];
    out->cy = proj[2 * 4 + 1];
    SLS_REQUIRE(out->fx != 0.0f && out->fy != 0.0f, "fx and fy must be non-zero");
    // p_view = R_vw p + t, R_vw = view[:3,:3]^T, t = view[3,:3]  (scene/cameras.py:43-46)
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out->Rvw[3 * r + c] = view[c * 4 + r];
    for (int c = 0; c < 3; ++c) out->tvw[c] = view[3 * 4 + c];
    out->scale_modifier = scale_modifier;
    out->near_cut = SLS_NEAR;
    out->far_cut = SLS_FAR;
    // D5: 360-degree image <=> |fx| * 2pi == W (within a pixel) and whole tiles per row
    const double period = fabs((double)out->fx) * 2.0 * 3.14159265358979323846;
    out->wrap = (fabs(period - (double)W) <= 1.0 && (W % kTileW) == 0) ? 1 : 0;
    return SLS_OK;
}

// rays of pixel (c, r) at image coordinate (c + oc, r + orow) for a principal point (cx, cy)
static void ray_tables_for(const SlsCamera *cam, double oc, double orow, double cx, double cy, float *col_cs, float *row_cs)
{
    for (int c = 0; c < cam->W; ++c) {
        const double a = ((double)c + oc - cx) / (double)cam->fx;
        col_cs[2 * c] = (float)cos(a);
        col_cs[2 * c + 1] = (float)sin(a);
    }
    for (int r = 0; r < cam->H; ++r) {
        const double e = ((double)r + orow - cy) / (double)cam->fy;
        row_cs[2 * r] = (float)cos(e);
        row_cs[2 * r + 1] = (float)sin(e);
    }
}

int sls_ray_tables(const SlsCamera *cam, float *col_cs, float *row_cs)
{
    SLS_REQUIRE(cam && col_cs && row_cs, "null pointer");
    // the rasterizer's own rays: the principal point the kernels use (make_devcam), rounded to float as there
    const DevCam dc = make_devcam(*cam);
    ray_tables_for(cam, 0.0, 0.0, (double)dc.cx, (double)dc.cy, col_cs, row_cs);
    return SLS_OK;
}

int sls_ray_tables_at(const SlsCamera *cam, float col_offset, float row_offset, float *col_cs, float *row_cs)
{
    SLS_REQUIRE(cam && col_cs && row_cs, "null pointer");
    ray_tables_for(cam, (double)col_offset, (double)row_offset, (double)cam->cx, (double)cam->cy, col_cs, row_cs);
    return SLS_OK;
}

}  // extern "C"

namespace sls {
int launch_adam(const SlsAdamGroup *groups, int ngroups, double beta1, double beta2, double eps, int64_t step,
                const uint32_t *skip_flag, hipStream_t stream, const float *void_flags, uint32_t *status_block,
                uint32_t *status_mirror)
{
    SLS_REQUIRE(groups && ngroups > 0 && ngroups <= kMaxAdamGroups, "1..8 groups");
    SLS_REQUIRE(step >= 1, "step is 1-based");
    AdamArgs a;
    memset(&a, 0, sizeof(a));
    int64_t units = 0;
    for (int i = 0; i < ngroups; ++i) {
        SLS_REQUIRE(groups[i].numel >= 0, "negative numel");
        SLS_REQUIRE(groups[i].numel == 0 || (groups[i].param && groups[i].grad && groups[i].exp_avg && groups[i].exp_avg_sq),
                    "null tensor");
        a.g[i] = groups[i];
        units += (groups[i].numel + 3) / 4;
        a.unit_end[i] = units;
    }
    for (int i = ngroups; i < kMaxAdamGroups; ++i) a.unit_end[i] = units;
    a.ngroups = ngroups;
    a.c = make_adam_coef(beta1, beta2, eps, step);
    if (units == 0 && !void_flags) return SLS_OK;   // (with void flags the verdict is still published)
    int64_t blocks = (units + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 256 * 8) blocks = 256 * 8;   // 8 blocks per CU, grid-stride beyond
    {
        ScopedTimer tm(T_ADAM, (hipStream_t)stream);
        hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, units, skip_flag,
                           void_flags, status_block, status_mirror);
    }
    SLS_LAUNCH_CHECK("adam_kernel");
    return SLS_OK;
}
}  // namespace sls

extern "C" {

int sls_adam_step(const SlsAdamGroup *groups, int ngroups, double beta1, double beta2, double eps, int64_t step,
                  void *stream)
{
    return launch_adam(groups, ngroups, beta1, beta2, eps, step, nullptr, (hipStream_t)stream, nullptr, nullptr, nullptr);
}

int sls_adam_step_guarded(const SlsAdamGroup *groups, int ngroups, double beta1, double beta2, double eps,
                          int64_t step, const uint32_t *skip_flag_dev, void *stream)
{
    return launch_adam(groups, ngroups, beta1, beta2, eps, step, skip_flag_dev, (hipStream_t)stream, nullptr, nullptr, nullptr);
}

int sls_adam_step_reduced(const SlsAdamGroup *groups, int ngroups, double beta1, double beta2, double eps,
                          int64_t step, const float *void_flags_dev, SlsMappingStatus *status_dev,
                          SlsMappingStatus *status_mirror, void *stream)
{
    SLS_REQUIRE(void_flags_dev, "null pointer");
    SLS_REQUIRE(!status_mirror || status_dev, "status_mirror needs status_dev");
    static_assert(sizeof(SlsMappingStatus) == 32, "the mirror copy moves 8 words");
    return launch_adam(groups, ngroups, beta1, beta2, eps, step, nullptr, (hipStream_t)stream, void_flags_dev,
                       (uint32_t *)status_dev, (uint32_t *)status_mirror);
}

size_t sls_consumer_scratch_bytes(int H, int W) { return (H > 0 && W > 0) ? consumer_scratch_bytes(H, W) : 0; }

int sls_consumer_fwd_bwd(int H, int W, const float *allmap, const float *gt_depth, const uint8_t *valid,
                         const float *col_cs_half, const float *row_cs_half, float depth_ratio,
                         float lambda_normal, float lambda_alpha, int n_valid, float *loss_sums,
                         float *dL_dallmap, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(H > 0 && W > 0 && n_valid >= 0, "bad size");
    SLS_REQUIRE(allmap && gt_depth && valid && col_cs_half && row_cs_half && loss_sums && dL_dallmap && scratch,
                "null pointer");
    ConsumerArgs c{};
    c.H = H; c.W = W; c.allmap = allmap; c.gt_depth = gt_depth; c.valid = valid; c.sums = loss_sums; c.dL_dallmap = dL_dallmap;
    c.col_h = (const float2 *)col_cs_half; c.row_h = (const float2 *)row_cs_half;
    c.depth_ratio = depth_ratio; c.lambda_n = lambda_normal; c.lambda_a = lambda_alpha;
    return launch_consumer(c, n_valid, scratch, scratch_bytes, false, (hipStream_t)stream, nullptr);
}

int sls_render_maps(int H, int W, const float *allmap, const float *view_rot9, const float *col_cs_half,
                    const float *row_cs_half, float depth_ratio, float *rend_normal, float *surf_depth,
                    float *surf_normal, void *stream)
{
    SLS_REQUIRE(H > 0 && W > 0, "bad size");
    SLS_REQUIRE(allmap && view_rot9 && col_cs_half && row_cs_half && rend_normal && surf_depth && surf_normal, "null pointer");
    return launch_render_maps(H, W, allmap, view_rot9, col_cs_half, row_cs_half, depth_ratio, rend_normal, surf_depth,
                              surf_normal, (hipStream_t)stream);
}

int sls_densify_weights(int H, int W, const float *image_depth, const uint8_t *valid, const float *rend_alpha,
                        float threshold_opacity, float *weights_out, uint32_t *stats_out, void *stream)
{
    SLS_REQUIRE(H > 0 && W > 0, "bad size");
    SLS_REQUIRE(image_depth && valid && weights_out && stats_out, "null pointer");
    return launch_densify_weights(H, W, image_depth, valid, rend_alpha, threshold_opacity, weights_out, stats_out,
                                  (hipStream_t)stream);
}

int sls_densify_rows(int n, int H, int W, const int64_t *pixels, const float *image_depth, const float *image_normal,
                     const float *col_cs_half, const float *row_cs_half, const float *cam_to_model16,
                     const float *model_T_frame16, float *xyz_out, float *quat_out, void *stream)
{
    SLS_REQUIRE(n >= 0 && H > 0 && W > 0, "bad size");
    if (n == 0) return SLS_OK;
    SLS_REQUIRE(pixels && image_depth && image_normal && col_cs_half && row_cs_half && cam_to_model16 && model_T_frame16 &&
                    xyz_out && quat_out, "null pointer");
    return launch_densify_rows(n, H, W, pixels, image_depth, image_normal, col_cs_half, row_cs_half, cam_to_model16,
                               model_T_frame16, xyz_out, quat_out, (hipStream_t)stream);
}

size_t sls_densify_draw_scratch_bytes(int H, int W) { return (H > 0 && W > 0) ? densify_draw_scratch_bytes(H, W) : 0; }

int sls_densify_draw(int H, int W, const float *image_depth, const uint8_t *valid, const float *rend_alpha,
                     float threshold_opacity, double percentage, uint64_t seed, uint32_t draw_index, float *weights_out,
                     int64_t *pixels_out, uint32_t *stats_out, uint32_t *stats_mirror, void *scratch, size_t scratch_bytes,
                     void *stream)
{
    SLS_REQUIRE(H > 0 && W > 0, "bad size");
    SLS_REQUIRE(image_depth && valid && weights_out && pixels_out && stats_out && scratch, "null pointer");
    SLS_REQUIRE(percentage >= 0.0 && percentage <= 1.0, "percentage outside [0, 1]");      // (false for a NaN too)
    if ((uint64_t)H * (uint64_t)W > SLS_DENSIFY_DRAW_MAX_PIXELS) {
        set_error("sls_densify_draw: %d x %d pixels, the selection serves at most %d (one workgroup, keys resident in L2); "
                  "draw with torch.multinomial over sls_densify_weights", H, W, SLS_DENSIFY_DRAW_MAX_PIXELS);
        return SLS_E_UNSUPPORTED;
    }
    SLS_REQUIRE(scratch_bytes >= densify_draw_scratch_bytes(H, W), "scratch smaller than sls_densify_draw_scratch_bytes(H, W)");
    SLS_REQUIRE(((uintptr_t)scratch & 15u) == 0, "scratch not 16-byte aligned");
    return launch_densify_draw(H, W, image_depth, valid, rend_alpha, threshold_opacity, percentage, seed, draw_index,
                               weights_out, pixels_out, stats_out, stats_mirror, scratch, (hipStream_t)stream);
}

size_t sls_surface_scratch_bytes(int H, int W) { return (H > 0 && W > 0) ? surface_scratch_bytes(H, W) : 0; }

int sls_surface_samples(int H, int W, const float *allmap, const float *col_cs_half, const float *row_cs_half,
                        const float *cam_to_world12, float min_opacity, float max_depth_dist, float depth_ratio,
                        int n_samples, uint64_t seed, uint32_t frame_id, float *points_out, float *normals_out,
                        int32_t *pixels_out, uint32_t *status_out, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(H > 0 && W > 0, "bad size");
    SLS_REQUIRE(n_samples >= 1, "n_samples < 1");
    SLS_REQUIRE(allmap && col_cs_half && row_cs_half && cam_to_world12 && points_out && normals_out && status_out && scratch,
                "null pointer");
    SLS_REQUIRE(min_opacity == min_opacity && max_depth_dist == max_depth_dist && depth_ratio == depth_ratio, "NaN threshold");
    if ((uint64_t)H * (uint64_t)W > SLS_SURFACE_MAX_PIXELS) {
        set_error("sls_surface_samples: %d x %d pixels, the sampler serves at most %d (the validity prefix lives in LDS)", H, W,
                  SLS_SURFACE_MAX_PIXELS);
        return SLS_E_UNSUPPORTED;
    }
    SLS_REQUIRE(scratch_bytes >= surface_scratch_bytes(H, W), "scratch smaller than sls_surface_scratch_bytes(H, W)");
    SLS_REQUIRE(((uintptr_t)scratch & 7u) == 0, "scratch not 8-byte aligned");
    return launch_surface_samples(H, W, allmap, col_cs_half, row_cs_half, cam_to_world12, min_opacity, max_depth_dist, depth_ratio,
                                  n_samples, seed, frame_id, points_out, normals_out, pixels_out, status_out, scratch,
                                  (hipStream_t)stream);
}

size_t sls_knn_scratch_bytes(int M) { return knn_scratch_bytes(M); }

int sls_knn_dist2(int M, const float *xyz, float *out, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(M >= 0, "negative M");
    if (M == 0) return SLS_OK;
    SLS_REQUIRE(xyz && out && scratch, "null pointer");
    return launch_knn(M, xyz, out, scratch, scratch_bytes, (hipStream_t)stream, -1);
}

int sls_wait_status_mirror(const void *mirror_host, uint32_t sentinel, void *stream)
{
    // The drop-in forward's status (R, void bits) arrives in the caller's pinned host block a few microseconds into the
    // binning; the caller must know it before it hands the image on.  Spun HERE (the binding releases the interpreter's
    // lock around a foreign call) with the CPU's pause hint; if the words have not arrived after ~2 ms of spinning the
    // stream is drained — a lost mirror write must not hang the caller.
    SLS_REQUIRE(mirror_host, "null pointer");
    const volatile uint32_t *w = (const volatile uint32_t *)mirror_host;
    for (int spin = 0; spin < 400000; ++spin) {
        if (w[7] != sentinel && w[0] != sentinel) { __atomic_thread_fence(__ATOMIC_ACQUIRE); return SLS_OK; }
        __builtin_ia32_pause();
    }
    SLS_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    if (w[7] != sentinel && w[0] != sentinel) return SLS_OK;
    set_error("the forward's status never reached its host mirror");
    return SLS_E_HIP;
}

int sls_knn_dist2_first(int M, int M_first, const float *xyz, float *out, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(M >= 0 && M_first >= 0 && M_first <= M, "bad sizes");
    if (M == 0 || M_first == 0) return SLS_OK;
    SLS_REQUIRE(xyz && out && scratch, "null pointer");
    return launch_knn(M, xyz, out, scratch, scratch_bytes, (hipStream_t)stream, M_first);
}

// What an entry point checks of the buffer it is lent — its scratch, or the ray casts' index: SLS_E_ARG unless it is
// 256-byte aligned, then SLS_E_SCRATCH unless it holds `need` bytes.  who: the entry point's name, as SLS_REQUIRE prints it
#define SLS_BUFFER_CHECK(who, what, ptr, have, need)                                                        \
    do {                                                                                                    \
        if (((uintptr_t)(ptr) & 255u) != 0) {                                                               \
            set_error("%s: " what " not 256-byte aligned", who);                                            \
            return SLS_E_ARG;                                                                               \
        }                                                                                                   \
        if ((have) < (size_t)(need)) {                                                                      \
            set_error("%s: " what " too small: %zu < %zu", who, (size_t)(have), (size_t)(need));            \
            return SLS_E_SCRATCH;                                                                           \
        }                                                                                                   \
    } while (0)
#define SLS_SCRATCH(need) SLS_BUFFER_CHECK(__func__, "scratch", scratch, scratch_bytes, need)

size_t sls_nn_scratch_bytes(int Mt, int Mq) { return nn_scratch_bytes(Mt, Mq); }

int sls_nn_query(int Mt, const float *target_xyz, int Mq, const float *query_xyz, float *out_dist2, int32_t *out_index,
                 void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(Mt >= 1, "Mt < 1: the target cloud is empty");
    SLS_REQUIRE(Mq >= 0, "negative Mq");
    if (Mq == 0) return SLS_OK;
    SLS_REQUIRE(target_xyz && query_xyz && out_dist2 && scratch, "null pointer");
    SLS_SCRATCH(nn_scratch_bytes(Mt, Mq));
    return launch_nn_query(Mt, target_xyz, Mq, query_xyz, out_dist2, out_index, scratch, (hipStream_t)stream);
}

int sls_nn_stats(int M, const float *dist2, float truncation, float threshold, int include_truncated, uint64_t *out_stats,
                 void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(M >= 0, "negative M");
    SLS_REQUIRE((dist2 || M == 0) && out_stats && scratch, "null pointer");
    SLS_REQUIRE(truncation == truncation && threshold == threshold, "NaN truncation or threshold");
    SLS_SCRATCH(SLS_NN_STATS_SCRATCH_BYTES);
    return launch_nn_stats(M, dist2, truncation, threshold, include_truncated, out_stats, scratch, (hipStream_t)stream);
}

size_t sls_mesh_distance_scratch_bytes(int V, int F, int Mq) { return mesh_distance_scratch_bytes(V, F, Mq); }

int sls_mesh_distance(int V, const float *vertices, int F, const int32_t *faces, int Mq, const float *query_xyz, float *out_dist2,
                      int32_t *out_face, float *out_closest, uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(V >= 1, "V < 1: the mesh has no vertex");
    SLS_REQUIRE(F >= 1, "F < 1: the mesh has no face");
    SLS_REQUIRE(Mq >= 0, "negative Mq");
    SLS_REQUIRE(vertices && faces && out_status && scratch && ((query_xyz && out_dist2) || Mq == 0), "null pointer");
    SLS_SCRATCH(mesh_distance_scratch_bytes(V, F, Mq));
    return launch_mesh_distance(V, vertices, F, faces, Mq, query_xyz, out_dist2, out_face, out_closest, out_status, scratch,
                                (hipStream_t)stream);
}

int sls_error_colors(int M, const float *dist2, float truncation, uint8_t *out_rgb, void *stream)
{
    SLS_REQUIRE(M >= 0, "negative M");
    SLS_REQUIRE((dist2 && out_rgb) || M == 0, "null pointer");
    SLS_REQUIRE(truncation > 0.0f && truncation <= 3.4028234e38f, "truncation must be finite and > 0");
    return launch_error_colors(M, dist2, truncation, out_rgb, (hipStream_t)stream);
}

size_t sls_mesh_rayindex_bytes(int V, int F) { return mesh_rayindex_bytes(V, F); }

int sls_mesh_rayindex_build(int V, const float *vertices, int F, const int32_t *faces, void *index, size_t index_bytes,
                            uint32_t *out_status, void *stream)
{
    SLS_REQUIRE(V >= 1, "V < 1: the mesh has no vertex");
    SLS_REQUIRE(F >= 1, "F < 1: the mesh has no face");
    SLS_REQUIRE(vertices && faces && index && out_status, "null pointer");
    SLS_BUFFER_CHECK(__func__, "index", index, index_bytes, mesh_rayindex_bytes(V, F));
    return launch_mesh_rayindex_build(V, vertices, F, faces, index, out_status, (hipStream_t)stream);
}

int sls_mesh_raycast(int V, const float *vertices, int F, const int32_t *faces, const void *index, size_t index_bytes, int Mr,
                     const float *origins, const float *directions, float t_min, float t_max, float *out_t, int32_t *out_face,
                     float *out_uv, uint32_t *out_status, void *stream)
{
    SLS_REQUIRE(V >= 1, "V < 1: the mesh has no vertex");
    SLS_REQUIRE(F >= 1, "F < 1: the mesh has no face");
    SLS_REQUIRE(Mr >= 0, "negative Mr");
    SLS_REQUIRE(vertices && faces && index && out_status && ((origins && directions && out_t) || Mr == 0), "null pointer");
    SLS_REQUIRE(((uintptr_t)index & 255u) == 0, "index not 256-byte aligned");   // (in its place before the range tests;
    SLS_REQUIRE(t_min >= 0.0f, "t_min is NaN or negative");                      // SLS_BUFFER_CHECK repeats it, then the size)
    SLS_REQUIRE(t_max >= t_min, "t_max is NaN or below t_min");
    SLS_BUFFER_CHECK(__func__, "index", index, index_bytes, mesh_rayindex_bytes(V, F));
    RaycastLaunch a{};
    a.V = V; a.vertices = vertices; a.F = F; a.faces = faces; a.index = index;
    a.Mr = Mr; a.origins = origins; a.directions = directions; a.t_min = t_min; a.t_max = t_max;
    a.out_t = out_t; a.out_face = out_face; a.out_uv = out_uv; a.out_status = out_status;
    return launch_mesh_raycast(a, (hipStream_t)stream);
}

size_t sls_mesh_pseudonormals_scratch_bytes(int V, int F) { return mesh_pseudonormals_scratch_bytes(V, F); }

int sls_mesh_pseudonormals(int V, const float *vertices, int F, const int32_t *faces, float *out_face_normals,
                           float *out_edge_normals, float *out_vertex_normals, uint32_t *out_status, void *scratch,
                           size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(V >= 1 && V <= SLS_MESH_MAX_VERTICES, "V < 1 or above SLS_MESH_MAX_VERTICES");
    SLS_REQUIRE(F >= 1 && F <= SLS_MESH_MAX_TRIANGLES, "F < 1 or above SLS_MESH_MAX_TRIANGLES");
    SLS_REQUIRE(vertices && faces && out_face_normals && out_edge_normals && out_vertex_normals && out_status && scratch,
                "null pointer");
    SLS_SCRATCH(mesh_pseudonormals_scratch_bytes(V, F));
    return launch_mesh_pseudonormals(V, vertices, F, faces, out_face_normals, out_edge_normals, out_vertex_normals, out_status,
                                     scratch, (hipStream_t)stream);
}

size_t sls_mesh_signed_distance_scratch_bytes(int V, int F, int Mq) { return mesh_signed_distance_scratch_bytes(V, F, Mq); }

int sls_mesh_signed_distance(int V, const float *vertices, int F, const int32_t *faces, const float *face_normals,
                             const float *edge_normals, const float *vertex_normals, int Mq, const float *query_xyz,
                             float *out_sdist, int32_t *out_face, float *out_closest, uint8_t *out_feature, uint32_t *out_status,
                             void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(V >= 1, "V < 1: the mesh has no vertex");
    SLS_REQUIRE(F >= 1, "F < 1: the mesh has no face");
    SLS_REQUIRE(Mq >= 0, "negative Mq");
    SLS_REQUIRE(vertices && faces && face_normals && edge_normals && vertex_normals && out_status && scratch &&
                ((query_xyz && out_sdist) || Mq == 0), "null pointer");
    SLS_SCRATCH(mesh_signed_distance_scratch_bytes(V, F, Mq));
    SignedDistanceLaunch a{};
    a.V = V; a.vertices = vertices; a.F = F; a.faces = faces;
    a.face_n = face_normals; a.edge_n = edge_normals; a.vertex_n = vertex_normals;
    a.Mq = Mq; a.query_xyz = query_xyz;
    a.out_sdist = out_sdist; a.out_face = out_face; a.out_closest = out_closest; a.out_feature = out_feature;
    a.out_status = out_status; a.scratch = scratch;
    return launch_mesh_signed_distance(a, (hipStream_t)stream);
}

int sls_signed_stats(int M, const float *sdist, float truncation, uint64_t *out_words, void *scratch, size_t scratch_bytes,
                     void *stream)
{
    SLS_REQUIRE(M >= 0, "negative M");
    SLS_REQUIRE((sdist || M == 0) && out_words && scratch, "null pointer");
    SLS_REQUIRE(truncation == truncation, "NaN truncation");
    SLS_SCRATCH(SLS_NN_STATS_SCRATCH_BYTES);
    return launch_signed_stats(M, sdist, truncation, out_words, scratch, (hipStream_t)stream);
}

int sls_signed_error_colors(int M, const float *sdist, float truncation, uint8_t *out_rgb, void *stream)
{
    SLS_REQUIRE(M >= 0, "negative M");
    SLS_REQUIRE((sdist && out_rgb) || M == 0, "null pointer");
    SLS_REQUIRE(truncation > 0.0f && truncation <= 3.4028234e38f, "truncation must be finite and > 0");
    return launch_signed_error_colors(M, sdist, truncation, out_rgb, (hipStream_t)stream);
}

size_t sls_nn_k_scratch_bytes(int Mt, int Mq, int k) { return nn_k_scratch_bytes(Mt, Mq, k); }

int sls_nn_query_k(int Mt, const float *target_xyz, int Mq, const float *query_xyz, int k, float *out_dist2, int32_t *out_index,
                   double *out_mean, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(Mt >= 1, "Mt < 1: the target cloud is empty");
    SLS_REQUIRE(Mq >= 0, "negative Mq");
    SLS_REQUIRE(k >= 1 && k <= SLS_NN_K_MAX, "k outside [1, SLS_NN_K_MAX]");
    if (Mq == 0) return SLS_OK;
    SLS_REQUIRE(target_xyz && query_xyz && scratch, "null pointer");
    SLS_SCRATCH(nn_k_scratch_bytes(Mt, Mq, k));
    return launch_nn_query_k(Mt, target_xyz, Mq, query_xyz, k, SLS_NN_K_MAX, out_dist2, out_index, out_mean, nullptr, scratch, (hipStream_t)stream);
}

size_t sls_outlier_scratch_bytes(int M, int k) { return outlier_scratch_bytes(M, k); }

// what the two filters check alike, behind their own parameter
static int outlier_check(const char *who, int M, const float *xyz, const float *normals, int k, float *out_normals,
                         uint64_t *out_status, void *scratch, size_t scratch_bytes, void *stream, bool *done)
{
    *done = true;
    if (M == 0) {
        if (out_status) SLS_HIP_CHECK(hipMemsetAsync(out_status, 0, SLS_OUTLIER_STATUS_WORDS * sizeof(uint64_t), (hipStream_t)stream));
        return SLS_OK;
    }
    if (!(xyz && out_status && scratch)) { set_error("%s: null pointer", who); return SLS_E_ARG; }
    if (out_normals && !normals) { set_error("%s: out_normals without normals", who); return SLS_E_ARG; }
    SLS_BUFFER_CHECK(who, "scratch", scratch, scratch_bytes, outlier_scratch_bytes(M, k));
    *done = false;
    return SLS_OK;
}

int sls_outlier_statistical(int M, const float *xyz, const float *normals, int k, double std_ratio, float *out_xyz,
                            float *out_normals, int32_t *out_index, uint64_t *out_status, void *scratch, size_t scratch_bytes,
                            void *stream)
{
    SLS_REQUIRE(M >= 0, "negative M");
    SLS_REQUIRE(k >= 1 && k <= SLS_NN_K_MAX, "k outside [1, SLS_NN_K_MAX]");
    SLS_REQUIRE(std_ratio > 0.0 && std_ratio <= DBL_MAX, "std_ratio is not a finite number > 0");
    bool done;
    const int rc = outlier_check("sls_outlier_statistical", M, xyz, normals, k, out_normals, out_status, scratch, scratch_bytes,
                                 stream, &done);
    if (rc || done) return rc;
    return launch_outlier_statistical(M, xyz, normals, k, std_ratio, out_xyz, out_normals, out_index, out_status, scratch,
                                      (hipStream_t)stream);
}

int sls_outlier_radius(int M, const float *xyz, const float *normals, int nb_points, float radius, float *out_xyz,
                       float *out_normals, int32_t *out_index, uint64_t *out_status, void *scratch, size_t scratch_bytes,
                       void *stream)
{
    SLS_REQUIRE(M >= 0, "negative M");
    SLS_REQUIRE(nb_points >= 0 && nb_points <= SLS_NN_K_MAX - 1, "nb_points outside [0, SLS_NN_K_MAX - 1]");
    SLS_REQUIRE(radius > 0.0f && radius <= FLT_MAX, "radius is not a finite number > 0");
    bool done;
    const int rc = outlier_check("sls_outlier_radius", M, xyz, normals, nb_points + 1, out_normals, out_status, scratch,
                                 scratch_bytes, stream, &done);
    if (rc || done) return rc;
    return launch_outlier_radius(M, xyz, normals, nb_points, radius, out_xyz, out_normals, out_index, out_status, scratch,
                                 (hipStream_t)stream);
}

size_t sls_cloud_dbscan_scratch_bytes(int M) { return cloud_dbscan_scratch_bytes(M); }
size_t sls_cloud_select_scratch_bytes(int M) { return cloud_select_scratch_bytes(M); }

int sls_cloud_dbscan(int M, const float *xyz, float eps, int min_points, int32_t *out_labels, int32_t *out_counts,
                     uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(M >= 0, "negative M");
    SLS_REQUIRE(eps > 0.0f && eps <= FLT_MAX, "eps is not a finite number > 0");
    SLS_REQUIRE(sls_cluster_eps_ok(eps), "eps * eps is not finite");
    SLS_REQUIRE(min_points >= 1, "min_points < 1");
    SLS_REQUIRE(out_status, "null pointer");
    if (M > 0) {
        SLS_REQUIRE(xyz && out_labels && out_counts && scratch, "null pointer");
        SLS_SCRATCH(cloud_dbscan_scratch_bytes(M));
    }
    return launch_cloud_dbscan(M, xyz, eps, min_points, out_labels, out_counts, out_status, scratch, (hipStream_t)stream);
}

int sls_cloud_select(int M, const float *xyz, const float *normals, const int32_t *labels, const int32_t *counts,
                     const uint32_t *cluster_status, int keep, int min_cluster_points, float *out_xyz, float *out_normals,
                     int32_t *out_index, uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(M >= 0, "negative M");
    SLS_REQUIRE(out_status, "null pointer");
    if (M > 0) {
        SLS_REQUIRE(xyz && labels && counts && cluster_status && scratch, "null pointer");
        SLS_REQUIRE(!(out_normals && !normals), "out_normals without normals");
        SLS_SCRATCH(cloud_select_scratch_bytes(M));
    }
    return launch_cloud_select(M, xyz, normals, labels, counts, cluster_status, keep, min_cluster_points, out_xyz, out_normals,
                               out_index, out_status, scratch, (hipStream_t)stream);
}

size_t sls_cloud_normals_scratch_bytes(int M, int k) { return cloud_normals_scratch_bytes(M, k); }

int sls_cloud_normals(int M, const float *xyz, int k, float radius, const float *viewpoint3, float *out_normals,
                      int32_t *out_count, float *out_eigenvalues, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(M >= 0, "negative M");
    SLS_REQUIRE(k >= 1 && k <= SLS_NORMALS_NN_MAX, "k outside [1, SLS_NORMALS_NN_MAX]");
    SLS_REQUIRE(radius > 0.0f, "radius is not a number > 0 (+inf: the k nearest at any distance)");
    if (M == 0) return SLS_OK;
    SLS_REQUIRE(xyz && viewpoint3 && out_normals && scratch, "null pointer");
    SLS_SCRATCH(cloud_normals_scratch_bytes(M, k));
    return launch_cloud_normals(M, xyz, k, radius, viewpoint3, out_normals, out_count, out_eigenvalues, scratch,
                                (hipStream_t)stream);
}

size_t sls_ground_scratch_bytes(int M) { return ground_scratch_bytes(M); }

int sls_ground_segment(int M, const float *xyz, const SlsGroundParams *prm, uint8_t *out_label, int32_t *out_bin,
                       double *out_planes, int32_t *out_info, uint32_t *out_status, void *scratch, size_t scratch_bytes,
                       void *stream)
{
    const auto positive = [](float v) { return v > 0.0f && v <= FLT_MAX; };
    SLS_REQUIRE(M >= 0, "negative M");
    SLS_REQUIRE(prm && out_status, "null pointer (prm, out_status)");
    SLS_REQUIRE(positive(prm->min_range) && positive(prm->max_range), "min_range, max_range: not finite numbers > 0");
    SLS_REQUIRE(prm->min_range < prm->max_range, "min_range >= max_range");
    SLS_REQUIRE(positive(prm->sensor_height), "sensor_height is not a finite number > 0");
    SLS_REQUIRE(positive(prm->th_seeds) && positive(prm->th_dist) && positive(prm->uprightness_thr) && positive(prm->noise_margin),
                "th_seeds, th_dist, uprightness_thr, noise_margin: not finite numbers > 0");
    for (int c = 0; c < 4; ++c)
        SLS_REQUIRE(positive(prm->elevation_thr[c]) && positive(prm->flatness_thr[c]),
                    "elevation_thr, flatness_thr: not finite numbers > 0");
    SLS_REQUIRE(prm->num_iter >= 1 && prm->num_iter <= 8, "num_iter outside [1, 8]");
    SLS_REQUIRE(prm->num_lpr >= 1, "num_lpr < 1");
    SLS_REQUIRE(prm->num_min_pts >= 3, "num_min_pts < 3");
    if (M > 0) {
        SLS_REQUIRE(xyz && out_label && scratch, "null pointer (xyz, out_label, scratch)");
        SLS_SCRATCH(ground_scratch_bytes(M));
    }
    return launch_ground_segment(M, xyz, *prm, out_label, out_bin, out_planes, out_info, out_status, scratch, (hipStream_t)stream);
}

size_t sls_cloud_icp_scratch_bytes(int Ms, int Mt) { return cloud_icp_scratch_bytes(Ms, Mt); }

int sls_cloud_icp(int Ms, const float *source_xyz, int Mt, const float *target_xyz, const float *target_normals,
                  const SlsIcpParams *prm, const double *init_pose12, uint64_t *out_status, double *out_system,
                  int32_t *out_index, float *out_dist2, void *scratch, size_t scratch_bytes, void *stream)
{
    const auto non_negative = [](double v) { return v >= 0.0 && v <= DBL_MAX; };
    SLS_REQUIRE(Ms >= 0, "negative Ms");
    SLS_REQUIRE(Mt >= 1, "Mt < 1: the target cloud is empty");
    SLS_REQUIRE(prm && init_pose12 && out_status && target_xyz && scratch && (source_xyz || Ms == 0), "null pointer");
    SLS_REQUIRE(prm->method == SLS_ICP_PLANE || prm->method == SLS_ICP_POINT, "unknown method");
    SLS_REQUIRE(prm->method == SLS_ICP_POINT || target_normals, "the plane method needs target_normals");
    SLS_REQUIRE(prm->max_distance > 0.0f && prm->max_distance <= FLT_MAX, "max_distance is not a finite number > 0");
    SLS_REQUIRE(non_negative(prm->damping) && non_negative(prm->eps_rot) && non_negative(prm->eps_trans),
                "damping, eps_rot, eps_trans: not finite numbers >= 0");
    SLS_REQUIRE(prm->iterations >= 0 && prm->iterations <= SLS_ICP_MAX_ITERATIONS, "iterations outside [0, 1000]");
    SLS_REQUIRE(prm->min_inliers >= 0, "negative min_inliers");
    for (int k = 0; k < 12; ++k) SLS_REQUIRE(fabs(init_pose12[k]) <= DBL_MAX, "init_pose12 holds a value that is not finite");
    SLS_SCRATCH(cloud_icp_scratch_bytes(Ms, Mt));
    return launch_cloud_icp(Ms, source_xyz, Mt, target_xyz, target_normals, *prm, init_pose12, out_status, out_system, out_index,
                            out_dist2, scratch, (hipStream_t)stream);
}

size_t sls_voxel_scratch_bytes(int M) { return voxel_scratch_bytes(M); }

int sls_voxel_downsample(int M, const float *xyz, double voxel_size, float *out_xyz, int32_t *out_count, uint32_t *out_status,
                         void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(M >= 0, "negative M");
    SLS_REQUIRE(voxel_size > 0.0 && voxel_size <= DBL_MAX, "voxel_size is not a finite number > 0");
    if (M == 0) {
        if (out_status) SLS_HIP_CHECK(hipMemsetAsync(out_status, 0, 4 * sizeof(uint32_t), (hipStream_t)stream));
        return SLS_OK;
    }
    SLS_REQUIRE(xyz && out_xyz && out_status && scratch, "null pointer");
    SLS_SCRATCH(voxel_scratch_bytes(M));
    return launch_voxel_downsample(M, xyz, voxel_size, out_xyz, out_count, out_status, scratch, (hipStream_t)stream);
}

size_t sls_mesh_sample_scratch_bytes(int V, int F, int n_samples) { return mesh_sample_scratch_bytes(V, F, n_samples); }

int sls_mesh_sample(int V, const float *vertices, int F, const int32_t *faces, const float *crop_box, int n_samples,
                    uint64_t seed, float *out_xyz, int32_t *out_face, uint32_t *out_status, void *scratch,
                    size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(V >= 0 && F >= 0, "negative V or F");
    SLS_REQUIRE(n_samples >= 0, "negative n_samples");
    if (n_samples == 0) {
        if (out_status) SLS_HIP_CHECK(hipMemsetAsync(out_status, 0, 4 * sizeof(uint32_t), (hipStream_t)stream));
        return SLS_OK;
    }
    SLS_REQUIRE((vertices || V == 0) && (faces || F == 0) && out_xyz && out_status && scratch, "null pointer");
    SLS_SCRATCH(mesh_sample_scratch_bytes(V, F, n_samples));
    return launch_mesh_sample(V, vertices, F, faces, crop_box, n_samples, seed, out_xyz, out_face, out_status, scratch,
                              (hipStream_t)stream);
}

size_t sls_tsdf_blocks_scratch_bytes(int M) { return tsdf_blocks_scratch_bytes(M); }

// voxel_size and trunc finite and > 0, and the margin trunc + voxel_size within one block
static bool tsdf_grid_ok(double voxel_size, double trunc)
{
    return voxel_size > 0.0 && voxel_size <= DBL_MAX && trunc > 0.0 && trunc <= DBL_MAX && trunc + voxel_size <= 8.0 * voxel_size;
}
static bool tsdf_origin_ok(const double *o) { return o && fabs(o[0]) <= DBL_MAX && fabs(o[1]) <= DBL_MAX && fabs(o[2]) <= DBL_MAX; }

int sls_tsdf_blocks(int M, const float *xyz, double voxel_size, double trunc, const double *origin3, int capacity,
                    int32_t *out_blocks, uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(M >= 0 && M <= SLS_TSDF_MAX_POINTS, "M negative or above SLS_TSDF_MAX_POINTS");
    SLS_REQUIRE(capacity >= 0, "negative capacity");
    SLS_REQUIRE(tsdf_grid_ok(voxel_size, trunc), "voxel_size and trunc must be finite and > 0 with trunc + voxel_size <= 8 voxel_size");
    SLS_REQUIRE(tsdf_origin_ok(origin3), "origin3 is null or not finite");
    if (M == 0) {
        if (out_status) {
            SLS_HIP_CHECK(hipMemsetAsync(out_status, 0, 3 * sizeof(uint32_t), (hipStream_t)stream));
            SLS_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(out_status + 3), 1, 1, (hipStream_t)stream));
        }
        return SLS_OK;
    }
    SLS_REQUIRE(xyz && (out_blocks || capacity == 0) && out_status && scratch, "null pointer");
    SLS_SCRATCH(tsdf_blocks_scratch_bytes(M));
    return launch_tsdf_blocks(M, xyz, voxel_size, trunc, origin3, capacity, out_blocks, out_status, scratch, (hipStream_t)stream);
}

int sls_tsdf_integrate(const SlsCamera *cam, int B, const int32_t *blocks, float *tsdf, float *weight, const float *allmap,
                       double voxel_size, double trunc, const double *origin3, float min_opacity, float max_depth_dist,
                       float depth_ratio, void *stream)
{
    SLS_REQUIRE(cam, "null pointer");
    SLS_REQUIRE(B >= 0 && B <= SLS_TSDF_MAX_BLOCKS, "B negative or above SLS_TSDF_MAX_BLOCKS");
    SLS_REQUIRE(cam->H > 0 && cam->W > 0 && (uint64_t)cam->H * (uint64_t)cam->W <= 0x7FFFFFFFull, "bad image size");
    SLS_REQUIRE(tsdf_grid_ok(voxel_size, trunc), "voxel_size and trunc must be finite and > 0 with trunc + voxel_size <= 8 voxel_size");
    SLS_REQUIRE(tsdf_origin_ok(origin3), "origin3 is null or not finite");
    SLS_REQUIRE(min_opacity == min_opacity && max_depth_dist == max_depth_dist && depth_ratio == depth_ratio, "NaN threshold");
    if (B == 0) return SLS_OK;
    SLS_REQUIRE(blocks && tsdf && weight && allmap, "null pointer");
    return launch_tsdf_integrate(*cam, B, blocks, tsdf, weight, allmap, voxel_size, trunc, origin3, min_opacity, max_depth_dist,
                                 depth_ratio, (hipStream_t)stream);
}

int sls_tsdf_extract_count(int B, const int32_t *blocks, const float *tsdf, const float *weight, float min_weight,
                           uint32_t *counts, uint32_t *prefix, uint32_t *out_status, void *stream)
{
    SLS_REQUIRE(B >= 0 && B <= SLS_TSDF_MAX_BLOCKS, "B negative or above SLS_TSDF_MAX_BLOCKS");
    SLS_REQUIRE(min_weight == min_weight, "NaN min_weight");
    SLS_REQUIRE(out_status && (B == 0 || (blocks && tsdf && weight && counts && prefix)), "null pointer");
    return launch_tsdf_extract_count(B, blocks, tsdf, weight, min_weight, counts, prefix, out_status, (hipStream_t)stream);
}

int sls_tsdf_extract_emit(int B, const int32_t *blocks, const float *tsdf, const float *weight, float min_weight,
                          double voxel_size, const double *origin3, const uint32_t *prefix, uint32_t T, float *triangles_out,
                          void *stream)
{
    SLS_REQUIRE(B >= 0 && B <= SLS_TSDF_MAX_BLOCKS, "B negative or above SLS_TSDF_MAX_BLOCKS");
    SLS_REQUIRE(min_weight == min_weight, "NaN min_weight");
    SLS_REQUIRE(voxel_size > 0.0 && voxel_size <= DBL_MAX, "voxel_size is not a finite number > 0");
    SLS_REQUIRE(tsdf_origin_ok(origin3), "origin3 is null or not finite");
    if (B == 0 || T == 0u) return SLS_OK;
    SLS_REQUIRE(blocks && tsdf && weight && prefix && triangles_out, "null pointer");
    return launch_tsdf_extract_emit(B, blocks, tsdf, weight, min_weight, voxel_size, origin3, prefix, T, triangles_out,
                                    (hipStream_t)stream);
}

size_t sls_poisson_splat_scratch_bytes(int M, int B) { return poisson_splat_scratch_bytes(M, B); }
size_t sls_poisson_solve_scratch_bytes(int B) { return poisson_solve_scratch_bytes(B); }
size_t sls_poisson_density_scratch_bytes(int B) { return poisson_density_scratch_bytes(B); }

int sls_poisson_splat(int M, const float *xyz, const float *normals, int B, const int32_t *blocks, double voxel_size,
                      const double *origin3, float *out_field, uint32_t *out_status, void *scratch, size_t scratch_bytes,
                      void *stream)
{
    SLS_REQUIRE(M >= 0 && M <= SLS_TSDF_MAX_POINTS, "M negative or above SLS_TSDF_MAX_POINTS");
    SLS_REQUIRE(B >= 0 && B <= SLS_TSDF_MAX_BLOCKS, "B negative or above SLS_TSDF_MAX_BLOCKS");
    SLS_REQUIRE(voxel_size > 0.0 && voxel_size <= DBL_MAX, "voxel_size is not a finite number > 0");
    SLS_REQUIRE(tsdf_origin_ok(origin3), "origin3 is null or not finite");
    if (M == 0) {
        if (out_status) {
            SLS_HIP_CHECK(hipMemsetAsync(out_status, 0, 3 * sizeof(uint32_t), (hipStream_t)stream));
            SLS_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(out_status + 3), 1, 1, (hipStream_t)stream));
        }
        return SLS_OK;
    }
    SLS_REQUIRE(xyz && normals && out_status && scratch && (B == 0 || (blocks && out_field)), "null pointer");
    SLS_SCRATCH(poisson_splat_scratch_bytes(M, B));
    return launch_poisson_splat(M, xyz, normals, B, blocks, voxel_size, origin3, out_field, out_status, scratch, (hipStream_t)stream);
}

int sls_poisson_solve(int B, const int32_t *blocks, const float *field, double alpha, int iterations, double tol,
                      float *out_chi, uint64_t *out_status, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(B >= 0 && B <= SLS_TSDF_MAX_BLOCKS, "B negative or above SLS_TSDF_MAX_BLOCKS");
    SLS_REQUIRE(alpha > 0.0 && alpha <= DBL_MAX, "alpha is not a finite number > 0");
    SLS_REQUIRE(tol >= 0.0 && tol <= DBL_MAX, "tol is not a finite number >= 0");
    SLS_REQUIRE(iterations >= 0 && iterations <= SLS_POISSON_MAX_ITERATIONS, "iterations outside [0, 1000]");
    SLS_REQUIRE(out_status, "null pointer (out_status)");
    if (B > 0) {
        SLS_REQUIRE(blocks && field && out_chi && scratch, "null pointer");
        SLS_SCRATCH(poisson_solve_scratch_bytes(B));
    }
    return launch_poisson_solve(B, blocks, field, alpha, iterations, tol, out_chi, out_status, scratch, (hipStream_t)stream);
}

int sls_poisson_density(int B, const int32_t *blocks, const float *field, int sweeps, float *out_density, void *scratch,
                        size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(B >= 0 && B <= SLS_TSDF_MAX_BLOCKS, "B negative or above SLS_TSDF_MAX_BLOCKS");
    SLS_REQUIRE(sweeps >= 0 && sweeps <= SLS_POISSON_MAX_SWEEPS, "sweeps outside [0, 64]");
    if (B == 0) return SLS_OK;
    SLS_REQUIRE(blocks && field && out_density && scratch, "null pointer");
    SLS_SCRATCH(poisson_density_scratch_bytes(B));
    return launch_poisson_density(B, blocks, field, sweeps, out_density, scratch, (hipStream_t)stream);
}

size_t sls_mesh_weld_scratch_bytes(int n_rows) { return mesh_weld_scratch_bytes(n_rows); }
size_t sls_mesh_clusters_scratch_bytes(int T) { return mesh_clusters_scratch_bytes(T); }
size_t sls_mesh_filter_scratch_bytes(int V, int T) { return mesh_filter_scratch_bytes(V, T); }
size_t sls_mesh_vertex_normals_scratch_bytes(int V, int T) { return mesh_normals_scratch_bytes(V, T); }
size_t sls_mesh_simplify_scratch_bytes(int V, int T) { return mesh_simplify_scratch_bytes(V, T); }
size_t sls_mesh_adjacency_scratch_bytes(int V, int T) { return mesh_adjacency_scratch_bytes(V, T); }
size_t sls_mesh_smooth_scratch_bytes(int V, int T) { return mesh_smooth_scratch_bytes(V, T); }
size_t sls_mesh_boundary_loops_scratch_bytes(int V, int T) { return mesh_fill_scratch_bytes(V, T); }
size_t sls_mesh_fill_holes_scratch_bytes(int V, int T) { return mesh_fill_scratch_bytes(V, T); }

// status words: `zeros` zeros, then `value` (optional), then the 1 that says "written"
static int mesh_empty_status(uint32_t *out_status, int zeros, int has_value, uint32_t value, hipStream_t st)
{
    if (!out_status) return SLS_OK;
    if (zeros) SLS_HIP_CHECK(hipMemsetAsync(out_status, 0, zeros * sizeof(uint32_t), st));
    if (has_value) SLS_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(out_status + zeros), (int)value, 1, st));
    SLS_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(out_status + zeros + has_value), 1, 1, st));
    return SLS_OK;
}

int sls_mesh_weld(int n_rows, const float *soup, float *out_vertices, int32_t *out_index, uint32_t *out_status, void *scratch,
                  size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(n_rows >= 0 && (int64_t)n_rows <= 3 * (int64_t)SLS_MESH_MAX_TRIANGLES, "n_rows negative or above 3 SLS_MESH_MAX_TRIANGLES");
    if (n_rows == 0) return mesh_empty_status(out_status, 3, 0, 0u, (hipStream_t)stream);
    SLS_REQUIRE(soup && out_vertices && out_index && out_status && scratch, "null pointer");
    SLS_SCRATCH(mesh_weld_scratch_bytes(n_rows));
    return launch_mesh_weld(n_rows, soup, out_vertices, out_index, out_status, scratch, (hipStream_t)stream);
}

int sls_mesh_clusters(int T, const int32_t *faces, int V, int32_t *out_labels, int32_t *out_counts, uint32_t *out_status,
                      void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(T >= 0 && T <= SLS_MESH_MAX_TRIANGLES, "T negative or above SLS_MESH_MAX_TRIANGLES");
    SLS_REQUIRE(V >= 0 && V <= SLS_MESH_MAX_VERTICES, "V negative or above SLS_MESH_MAX_VERTICES");
    if (T == 0) return mesh_empty_status(out_status, 5, 0, 0u, (hipStream_t)stream);
    SLS_REQUIRE(faces && out_labels && out_counts && out_status && scratch, "null pointer");
    SLS_SCRATCH(mesh_clusters_scratch_bytes(T));
    return launch_mesh_clusters(T, faces, V, out_labels, out_counts, out_status, scratch, (hipStream_t)stream);
}

int sls_mesh_filter(int V, const float *vertices, int T, const int32_t *faces, const int32_t *labels, const int32_t *counts,
                    const uint32_t *cluster_status, int keep_clusters, int min_triangles, float *out_vertices,
                    int32_t *out_faces, int32_t *out_vmap, uint32_t *out_status, void *scratch, size_t scratch_bytes,
                    void *stream)
{
    SLS_REQUIRE(T >= 0 && T <= SLS_MESH_MAX_TRIANGLES, "T negative or above SLS_MESH_MAX_TRIANGLES");
    SLS_REQUIRE(V >= 0 && V <= SLS_MESH_MAX_VERTICES, "V negative or above SLS_MESH_MAX_VERTICES");
    if (V == 0 || T == 0) return mesh_empty_status(out_status, 2, 1, min_triangles > 0 ? (uint32_t)min_triangles : 0u, (hipStream_t)stream);
    SLS_REQUIRE(vertices && faces && labels && counts && cluster_status && out_vertices && out_faces && out_status && scratch,
                "null pointer");
    SLS_SCRATCH(mesh_filter_scratch_bytes(V, T));
    return launch_mesh_filter(V, vertices, T, faces, labels, counts, cluster_status, keep_clusters, min_triangles, out_vertices,
                              out_faces, out_vmap, out_status, scratch, (hipStream_t)stream);
}

int sls_mesh_vertex_normals(int V, const float *vertices, int T, const int32_t *faces, float *out_normals, void *scratch,
                            size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(T >= 0 && T <= SLS_MESH_MAX_TRIANGLES, "T negative or above SLS_MESH_MAX_TRIANGLES");
    SLS_REQUIRE(V >= 0 && V <= SLS_MESH_MAX_VERTICES, "V negative or above SLS_MESH_MAX_VERTICES");
    if (V == 0) return SLS_OK;
    SLS_REQUIRE(out_normals && (T == 0 || (vertices && faces && scratch)), "null pointer");
    if (T > 0) SLS_SCRATCH(mesh_normals_scratch_bytes(V, T));
    return launch_mesh_vertex_normals(V, vertices, T, faces, out_normals, scratch, (hipStream_t)stream);
}

int sls_mesh_simplify(int V, const float *vertices, int T, const int32_t *faces, double voxel_size, int contraction,
                      double regularisation, float *out_vertices, int32_t *out_faces, int32_t *out_vmap, uint32_t *out_status,
                      void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(T >= 0 && T <= SLS_MESH_MAX_TRIANGLES, "T negative or above SLS_MESH_MAX_TRIANGLES");
    SLS_REQUIRE(V >= 0 && V <= SLS_MESH_MAX_VERTICES, "V negative or above SLS_MESH_MAX_VERTICES");
    SLS_REQUIRE(voxel_size > 0.0 && voxel_size <= DBL_MAX, "voxel_size must be finite and > 0");
    SLS_REQUIRE(contraction == 0 || contraction == 1, "contraction must be 0 (average) or 1 (quadric)");
    SLS_REQUIRE(regularisation >= 0.0 && regularisation <= DBL_MAX, "regularisation must be finite and >= 0");
    if (V == 0 || T == 0) {                         // no triangle is kept: every vertex leaves
        if (out_vmap && V > 0) SLS_HIP_CHECK(hipMemsetAsync(out_vmap, 0xFF, sizeof(int32_t) * (size_t)V, (hipStream_t)stream));
        return mesh_empty_status(out_status, 7, 0, 0u, (hipStream_t)stream);
    }
    SLS_REQUIRE(vertices && faces && out_vertices && out_faces && out_status && scratch, "null pointer");
    SLS_SCRATCH(mesh_simplify_scratch_bytes(V, T));
    return launch_mesh_simplify(V, vertices, T, faces, voxel_size, contraction, regularisation, out_vertices, out_faces, out_vmap,
                                out_status, scratch, (hipStream_t)stream);
}

int sls_mesh_adjacency(int V, int T, const int32_t *faces, int32_t *out_offsets, int32_t *out_neighbours, uint8_t *out_boundary,
                       uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(T >= 0 && T <= SLS_MESH_MAX_TRIANGLES, "T negative or above SLS_MESH_MAX_TRIANGLES");
    SLS_REQUIRE(V >= 0 && V <= SLS_MESH_MAX_VERTICES, "V negative or above SLS_MESH_MAX_VERTICES");
    if (V == 0 || T == 0) {                         // no edge: every row is empty
        SLS_REQUIRE(V == 0 || (out_offsets && out_boundary), "null pointer");
        if (out_offsets) SLS_HIP_CHECK(hipMemsetAsync(out_offsets, 0, sizeof(int32_t) * ((size_t)V + 1), (hipStream_t)stream));
        if (V > 0) SLS_HIP_CHECK(hipMemsetAsync(out_boundary, 0, (size_t)V, (hipStream_t)stream));
        return mesh_empty_status(out_status, 7, 0, 0u, (hipStream_t)stream);
    }
    SLS_REQUIRE(faces && out_offsets && out_neighbours && out_boundary && out_status && scratch, "null pointer");
    SLS_SCRATCH(mesh_adjacency_scratch_bytes(V, T));
    return launch_mesh_adjacency(V, T, faces, out_offsets, out_neighbours, out_boundary, out_status, scratch, (hipStream_t)stream);
}

int sls_mesh_smooth(int V, const float *vertices, int T, const int32_t *faces, int method, int weights, int iterations, double lambda,
                    double mu, int fix_boundary, float *out_vertices, uint32_t *out_status, void *scratch, size_t scratch_bytes,
                    void *stream)
{
    SLS_REQUIRE(T >= 0 && T <= SLS_MESH_MAX_TRIANGLES, "T negative or above SLS_MESH_MAX_TRIANGLES");
    SLS_REQUIRE(V >= 0 && V <= SLS_MESH_MAX_VERTICES, "V negative or above SLS_MESH_MAX_VERTICES");
    SLS_REQUIRE(method == SLS_SMOOTH_SIMPLE || method == SLS_SMOOTH_LAPLACIAN || method == SLS_SMOOTH_TAUBIN,
                "method must be 0 (simple), 1 (laplacian) or 2 (taubin)");
    SLS_REQUIRE(weights == SLS_SMOOTH_UNIFORM || weights == SLS_SMOOTH_INVERSE_DISTANCE, "weights must be 0 (uniform) or 1 (inverse distance)");
    SLS_REQUIRE(iterations >= 0, "iterations must be >= 0");
    SLS_REQUIRE(fabs(lambda) <= DBL_MAX && fabs(mu) <= DBL_MAX, "lambda and mu must be finite");
    SLS_REQUIRE(!(vertices && out_vertices == vertices), "out_vertices must not be vertices");
    if (V == 0 || T == 0) {                         // no vertex is live: every one is copied
        SLS_REQUIRE(V == 0 || (vertices && out_vertices), "null pointer");
        if (V > 0)
            SLS_HIP_CHECK(hipMemcpyAsync(out_vertices, vertices, 3 * sizeof(float) * (size_t)V, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return mesh_empty_status(out_status, 7, 0, 0u, (hipStream_t)stream);
    }
    SLS_REQUIRE(vertices && faces && out_vertices && out_status && scratch, "null pointer");
    SLS_SCRATCH(mesh_smooth_scratch_bytes(V, T));
    return launch_mesh_smooth(V, vertices, T, faces, method, weights, iterations, lambda, mu, fix_boundary, out_vertices, out_status,
                              scratch, (hipStream_t)stream);
}

int sls_mesh_boundary_loops(int V, int T, const int32_t *faces, const uint32_t *in_counts, int32_t *out_halfedges, int32_t *out_loop,
                            int32_t *out_loop_edges, uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(T >= 0 && T <= SLS_MESH_MAX_TRIANGLES, "T negative or above SLS_MESH_MAX_TRIANGLES");
    SLS_REQUIRE(V >= 0 && V <= SLS_MESH_MAX_VERTICES, "V negative or above SLS_MESH_MAX_VERTICES");
    if (V == 0 || T == 0)                           // no half-edge
        return launch_mesh_fill_empty(V, nullptr, T, nullptr, in_counts, 0, nullptr, 0, nullptr, out_status, (hipStream_t)stream);
    SLS_REQUIRE(faces && out_halfedges && out_loop && out_loop_edges && out_status && scratch, "null pointer");
    SLS_SCRATCH(mesh_fill_scratch_bytes(V, T));
    return launch_mesh_boundary_loops(V, T, faces, in_counts, out_halfedges, out_loop, out_loop_edges, out_status, scratch,
                                      (hipStream_t)stream);
}

int sls_mesh_fill_holes(int V, const float *vertices, int T, const int32_t *faces, const uint32_t *in_counts, int max_edges,
                        double max_size, int cap_vertices, float *out_vertices, int cap_triangles, int32_t *out_faces,
                        uint32_t *out_status, void *scratch, size_t scratch_bytes, void *stream)
{
    SLS_REQUIRE(T >= 0 && T <= SLS_MESH_MAX_TRIANGLES, "T negative or above SLS_MESH_MAX_TRIANGLES");
    SLS_REQUIRE(V >= 0 && V <= SLS_MESH_MAX_VERTICES, "V negative or above SLS_MESH_MAX_VERTICES");
    SLS_REQUIRE(max_edges >= 3, "max_edges must be >= 3");
    SLS_REQUIRE(max_size >= 0.0 && max_size <= DBL_MAX, "max_size must be finite and >= 0");
    SLS_REQUIRE(cap_vertices >= V && cap_vertices <= SLS_MESH_MAX_VERTICES, "cap_vertices below V or above SLS_MESH_MAX_VERTICES");
    SLS_REQUIRE(cap_triangles >= T && cap_triangles <= SLS_MESH_MAX_TRIANGLES, "cap_triangles below T or above SLS_MESH_MAX_TRIANGLES");
    SLS_REQUIRE(!(vertices && out_vertices == vertices), "out_vertices must not be vertices");
    SLS_REQUIRE(!(faces && out_faces == faces), "out_faces must not be faces");
    if (V == 0 || T == 0) {                         // no half-edge: the live rows are copied, the faces padded
        SLS_REQUIRE((V == 0 || (vertices && out_vertices)) && (T == 0 || faces) && (cap_triangles == 0 || out_faces), "null pointer");
        return launch_mesh_fill_empty(V, vertices, T, faces, in_counts, 1, out_vertices, cap_triangles, out_faces, out_status,
                                      (hipStream_t)stream);
    }
    SLS_REQUIRE(vertices && faces && out_vertices && out_faces && out_status && scratch, "null pointer");
    SLS_SCRATCH(mesh_fill_scratch_bytes(V, T));
    return launch_mesh_fill_holes(V, vertices, T, faces, in_counts, max_edges, max_size, cap_vertices, out_vertices, cap_triangles,
                                  out_faces, out_status, scratch, (hipStream_t)stream);
}

int sls_mark_visible(const SlsCamera *cam, int N, const float *means3D, uint8_t *visible, void *stream)
{
    SLS_REQUIRE(cam && N >= 0, "bad argument");
    if (N == 0) return SLS_OK;
    SLS_REQUIRE(means3D && visible, "null pointer");
    return launch_mark_visible(make_devcam(*cam), N, means3D, visible, (hipStream_t)stream);
}

int sls_debug_wave_cycles(uint32_t *fwd_cycles, uint32_t *bwd_cycles)
{
    debug_state().dbg_fwd_cycles = fwd_cycles;
    debug_state().dbg_bwd_cycles = bwd_cycles;
    return SLS_OK;
}

int sls_debug_variant(int fwd, int bwd)
{
    // (kept for binary compatibility: the 8x2 pixel blocks are the only tile kernels, so there is nothing to set)
    SLS_REQUIRE((fwd < 0 || fwd == 3) && (bwd < 0 || bwd == 3),
                "tile-kernel variant: only 3 (8x2 pixel blocks) exists; the 4x4 variant 2 was removed (negative: no change)");
    return SLS_OK;
}

int sls_timing_slots(void) { return T_COUNT; }
const char *sls_timing_name(int slot) { return (slot >= 0 && slot < T_COUNT) ? kTimerNames[slot] : ""; }

int sls_timing_enable(int on)
{
    std::lock_guard<std::mutex> lk(g_timer_mutex);
    if (!t_timer) {
        if (!on) return SLS_OK;
        t_timer = new TimerState();
    }
    if (on && g_timer.created == 0) {
        for (int i = 0; i < kTimerPool; ++i) {
            if (hipEventCreate(&g_timer.start[i]) != hipSuccess || hipEventCreate(&g_timer.stop[i]) != hipSuccess) break;
            g_timer.created = i + 1;
        }
    }
    g_timer.enabled = on != 0;
    g_timer.mode = on;
    g_timer.used = 0;
    g_timer.seen = 0;
    g_timer.open = -1;
    g_timer_on.store(on != 0, std::memory_order_relaxed);
    return SLS_OK;
}

int sls_timing_collect(double *total_ms, int64_t *counts)
{
    SLS_REQUIRE(total_ms && counts, "null pointer");
    for (int s = 0; s < T_COUNT; ++s) { total_ms[s] = 0.0; counts[s] = 0; }
    std::lock_guard<std::mutex> lk(g_timer_mutex);
    if (!t_timer) return SLS_OK;
    for (int i = 0; i < g_timer.used; ++i) {
        SLS_HIP_CHECK(hipEventSynchronize(g_timer.stop[i]));
        float ms = 0.0f;
        SLS_HIP_CHECK(hipEventElapsedTime(&ms, g_timer.start[i], g_timer.stop[i]));
        total_ms[g_timer.slot[i]] += (double)ms;
        counts[g_timer.slot[i]] += 1;
    }
    const int dropped = (g_timer.used >= g_timer.created) ? 1 : 0;
    g_timer.used = 0;
    g_timer.open = -1;
    return dropped ? 1 : SLS_OK;   // 1: pool exhausted, later launches were not timed
}

int sls_selftest(void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    int *d = nullptr;
    SLS_HIP_CHECK(hipMalloc(&d, sizeof(int)));   // test-only entry point: the one place the library allocates
    int h = 0;
    hipError_t e = hipMemsetAsync(d, 0, sizeof(int), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(selftest_kernel, dim3(2), dim3(128), 0, st, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d);
    if (e != hipSuccess) {
        set_error("selftest: %s", hipGetErrorString(e));
        return SLS_E_HIP;
    }
    if (h != 0) {
        set_error("selftest: wave primitive mismatch, flags 0x%x", h);
        return SLS_E_HIP;
    }
    return SLS_OK;
}

}  // extern "C"

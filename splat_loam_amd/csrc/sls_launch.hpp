// sls_launch.hpp — the internal prototypes: every function one translation unit of libsls_hip.so defines and another
// calls is declared HERE and nowhere else; the defining file and every caller include this header.  No default
// arguments.  The wide launchers take one plain struct each: value-initialise it at the call site (`XLaunch a{};`) and
// fill it by field name — a zero / null field means "option off".  What a caller reads back stays a parameter.
#pragma once
#include "sls_common.hpp"

namespace sls {

struct ConsumerArgs;    // sls_consumer_dev.hpp

// The tile backward can walk its blocks most expensive first (8x2 blocks, XCD-interleaved tile mapping) — the one rule
// for "this image has a launch order", for the hand-over buffer and for the callers' block_order buffers alike
inline bool launch_order_possible(int T) { return T % 32 == 0 && kTileW == 16 && kTileH == 16; }

// ---- sls_radix.hip: the radix sorter -------------------------------------------------------------------------------
size_t sort_scratch_bytes(uint64_t cap);
// of which the count table + digit totals; behind them the list of (surfel, block mask) pairs and the 64-bit instances
// it is sorted from
size_t sort_core_bytes(uint64_t cap);
uint2 *sort_bmask_buffer(void *scratch, uint64_t cap);
uint64_t *sort_wide_buffer(void *scratch, uint64_t cap);
int sort_passes(int nbits);     // passes of the sorter over nbits key bits
int radix_sort_pairs_u32(uint32_t *keys, uint32_t *vals, uint32_t *keys_tmp, uint32_t *vals_tmp,
                         const uint32_t *count_ptr, uint32_t cap, int nbits, void *scratch, size_t scratch_bytes,
                         int *result_in_tmp, hipStream_t st);
// the same sorter on 64-bit keys (sls_cloud.hip: the 63-bit voxel keys)
int radix_sort_pairs_u64(uint64_t *keys, uint32_t *vals, uint64_t *keys_tmp, uint32_t *vals_tmp,
                         const uint32_t *count_ptr, uint32_t cap, int nbits, void *scratch, size_t scratch_bytes,
                         int *result_in_tmp, hipStream_t st);
// ... with what the depth order and the tile sort (sls_sort.hip) ask of it:
struct RadixOptions {
    uint2 *ranges_out; int nranges;     // single-pass sorts only: [start, end) of every key value < nranges ((0,0): absent)
    bool drop_sorted_keys;              // the last pass writes the permuted values only
    int base_shift;                     // the digits start at this bit; vals == null: the value is the key's low base_shift bits
    BlockMaskArgs bm;                   // 64-bit keys, single pass: (value, block mask) pairs to bm.out instead of the values
};
constexpr RadixOptions kNoRadixOptions = { nullptr, 0, false, 0, { nullptr, 1, 1.0f, 1 } };     // = radix_sort_pairs_*
int radix_sort_options_u32(uint32_t *keys, uint32_t *vals, uint32_t *keys_tmp, uint32_t *vals_tmp,
                           const uint32_t *count_ptr, uint32_t cap, int nbits, void *scratch, size_t scratch_bytes,
                           int *result_in_tmp, hipStream_t st, const RadixOptions &opt);
int radix_sort_options_u64(uint64_t *keys, uint32_t *vals, uint64_t *keys_tmp, uint32_t *vals_tmp,
                           const uint32_t *count_ptr, uint32_t cap, int nbits, void *scratch, size_t scratch_bytes,
                           int *result_in_tmp, hipStream_t st, const RadixOptions &opt);
// One pass of `bits`-bit digits (8 .. 11) over the EMISSION's chunks, which counted their digits themselves (cnt: 2^bits
// rows of nchunks words): row scan + scatter, no histogram launch.  chunk c = items [chunk_start[c], chunk_start[c + 1]);
// the values go to vals_out (or the pairs to bm.out), the sorted keys are not written.
struct EmitChunkSort {
    const uint32_t *vals; uint32_t *vals_out;       // vals null: the value is (key & packed_val_mask)
    const uint32_t *chunk_start; uint32_t cap; int shift, bits;
    uint32_t *cnt, *totals; int nchunks;
    uint2 *ranges_out; int nranges; uint32_t packed_val_mask; BlockMaskArgs bm;
};
int tile_sort_emit_chunks_u32(const uint32_t *keys, const EmitChunkSort &a, hipStream_t st);
int tile_sort_emit_chunks_u64(const uint64_t *keys, const EmitChunkSort &a, hipStream_t st);
// its row scan alone (the direct binning): every row of a table of rows x nchunks words scanned exclusively in place
int sort_rowscan_rows(uint32_t *cnt, int rows, int nchunks, uint32_t *totals, uint32_t cap, hipStream_t st);

// ---- sls_sort.hip: depth order, binning ----------------------------------------------------------------------------
// What the depth-order stage hands to the binning that follows it
struct ScanHandoff {
    const uint32_t *block_sums;     // sums of tiles_touched over 256-blocks of depth-order positions (the emission
                                    // finishes the scan itself; null: it reads precomputed offsets)
    int resort_windows;             // > 0: the order was repaired, check these window edges (resort_verify)
    const uint64_t *resort_edges;
    int counted;                    // direct binning: the repair's merge already filled the count table
};

constexpr int kDirectChunk = 1024;     // depth positions per chunk of the direct binning (= the repair's window)
constexpr int kDirectMaxBins = 512;    // tiles it serves

// Direct binning (sls_sort.hip): the count table over chunks of 1024 depth positions and the per-position records
struct DirectBin {
    uint32_t *cnt;          // count table cnt[tile][chunk]: bins x nchunks words
    uint32_t *totals;       // bins words
    uint2 *serec;           // optional: per depth position the surfel's emission record {rectangle in one word, block box}
    int bins, nchunks, pos0;    // pos0: first depth position of chunk 0 (0, or -512: the repair's shifted windows)
    int stride;             // words per row of cnt (>= nchunks; a multiple of kDirectGroup with the coarse table: a group's
                            // counts of one tile are then one aligned 64-byte line)
    // optional (sls_mapping_step): coarse[group][tile] = the tile's instances in the chunks of group g (kDirectGroup
    // chunks each), summed with atomics by the counting kernels and ZEROED by the iteration's first kernel.  With it
    // bin_direct sums what lies in front of its chunk itself — the groups in front + the chunks of its own group — and
    // the row-scan launch disappears (one dependent launch less); cnt then keeps the RAW counts.
    uint32_t *coarse;
};
constexpr int kDirectGroup = 16;

size_t order_scratch_bytes(int N);
// where preprocess writes the depth sort's input (keys, identity permutation, N on the device) and the repair its pairs
void depth_order_key_buffers(int N, void *scratch, uint32_t *order, uint32_t **keys, uint32_t **vals0, uint32_t **n_dev);
uint64_t *resort_comp_buffer(int N, void *scratch);
bool bin_direct_possible(const DevCam &cam, int N, uint32_t cap);
DirectBin make_direct_bin(const DevCam &cam, int N, void *sort_scratch, uint2 *serec, bool repaired, bool coarse);
size_t direct_coarse_words(const DevCam &cam, int N);

// Depth order of the surfels (keys written by preprocess) + scan of tiles_touched in that order
struct DepthOrderScan {
    int N; const uint32_t *tiles; uint32_t *order, *offsets, *total_out;
    void *scratch; size_t scratch_bytes;
    int reuse_order;            // > 0: `order` holds the camera's previous permutation, repaired in so many rounds ...
    uint32_t *fail_flag;        // ... with failure reported here (null: sorted from scratch)
    bool window_sort_done;      // step A of the repair already ran, merged into the preprocess launch
    const DirectBin *direct;    // the direct binning follows (with handoff: the repair's last merge fills its count table)
    const int4 *erec_box; int GX;
};
// handoff (optional, out): the binning finishes — or does not need — the scan of tiles_touched
int launch_depth_order_scan(const DepthOrderScan &a, hipStream_t st, ScanHandoff *handoff);

// Emission in depth order + stable sort by tile + ranges
struct BinSortLaunch {
    int N;
    const uint32_t *count_ptr; uint32_t cap;    // device R; host-side capacity of the buffers
    const uint32_t *order; const int32_t *rect; const uint32_t *tiles; const uint64_t *tile_mask; const int32_t *erec;
    const float *depth; const uint32_t *offsets;
    uint32_t *tkeys, *vals, *tkeys_tmp, *vals_tmp;      // cap u32 each (ping-pong)
    void *scratch; size_t scratch_bytes;
    uint32_t *ranges; uint64_t *keys64_out; uint32_t *overflow;
    const ScanHandoff *handoff; uint32_t *total_out;
    const uint32_t *sbox; int bmask_mode;       // block boxes + SlsMappingConfig.block_masks (0 auto, 1 always, 2 never)
};
// out: *sorted_in_tmp (which value array holds the list), *bmask_out (optional; the list as (surfel, block mask) pairs,
// null where that is not possible)
int launch_bin_sort(const DevCam &cam, const BinSortLaunch &a, hipStream_t st, int *sorted_in_tmp, const uint2 **bmask_out);

// order (+ erec_box, or rect + sbox) -> sorted list, ranges, R
struct BinDirectLaunch {
    int N; uint32_t cap;
    DirectBin db; bool counted;     // counted: the count table was filled by the repair's merge
    const uint32_t *order; const int32_t *erec_box; const int32_t *rect; const uint32_t *sbox;
    void *scratch; uint32_t *vals_out, *ranges, *total_out, *overflow;
    int resort_windows; const uint64_t *resort_edges; int bmask_mode;
    uint32_t *status_mirror;        // pinned host memory: the status block, early (sls_forward_ws)
};
int launch_bin_direct(const DevCam &cam, const BinDirectLaunch &a, hipStream_t st, const uint2 **bmask_out);

// ---- sls_preprocess.hip --------------------------------------------------------------------------------------------
struct PreFwdLaunch {
    int N;
    int raw; float smax, pen; float *reg_out;   // raw parameters + the scale regulariser (RegArgs)
    const float *means, *scales, *rots, *opac;
    float *rec; int32_t *radii, *rect; uint32_t *tiles; float *depth;
    uint32_t *order_keys, *order_vals, *n_dev;  // depth_order_key_buffers
    uint32_t *status_clear;                     // the iteration's status block, zeroed by this first kernel
    const float *col_cs, *row_cs; uint64_t *tile_mask;
    int32_t *erec; int erec_box;                // emission records; 1: in the form the direct binning gathers
    const uint32_t *resort_prev_order; uint64_t *resort_comp;   // both: the repair's window sort rides in this launch
    uint32_t *sbox;
    uint32_t *zero_words; int n_zero_words;     // the direct binning's coarse table, zeroed here
};
int launch_preprocess_fwd(const DevCam &cam, const PreFwdLaunch &a, hipStream_t st);

// One struct for the single-keyframe and the batched backward of the projection
struct PreBwdLaunch {
    int N;
    int raw; float smax, pen;                   // (a batch always runs on raw parameters)
    const float *means, *scales, *rots, *opac;  // written only by the fused Adam update of the caller's own tensors
    float *dmeans, *dscales, *drots, *dopac; const PoseOut *pose;
    const int32_t *radii; const float *grec; const AdamFuse *fuse;      // one keyframe; a batch has them in its BatchFuse
};
int launch_preprocess_bwd(const DevCam &cam, const PreBwdLaunch &a, hipStream_t st);
int launch_preprocess_bwd_batch(const PreBwdLaunch &a, const BatchFuse &bf, hipStream_t st);
int launch_mark_visible(const DevCam &cam, int N, const float *means, uint8_t *visible, hipStream_t st);

// ---- sls_render_block.hip ------------------------------------------------------------------------------------------
size_t block_mask_bytes(uint64_t cap, int T);
struct RenderFwdLaunch {
    const uint32_t *ranges, *vals; const float *rec, *col_cs, *row_cs;
    float *allmap, *pix_state; uint32_t *pix_contrib, *tile_consumed; bool consumed_zeroed;
    uint64_t *block_masks;          // the hand-over buffer: the blocks' compact lists for the backward
    bool lean; uint32_t *block_cost;    // lean: no median / distortion planes
    const uint2 *bmask;             // the list as (surfel, block mask) pairs: dense rounds
    bool order_in_handover;         // + the backward's launch order into the hand-over buffer (the staged API)
};
int launch_render_fwd(const DevCam &cam, const RenderFwdLaunch &a, hipStream_t st);

struct RenderBwdLaunch {
    const uint32_t *ranges, *vals; int vals_stride;     // vals_stride (required): 1 plain list, 2 (surfel, block mask) pairs
    const float *rec, *col_cs, *row_cs, *pix_state; const uint32_t *pix_contrib; const float *dL_dallmap;
    float *grec; uint8_t *touched; bool lean;
    const uint64_t *block_masks; int block_masks_shape; // the producer's tag of the compact lists: walked only for 3
    const ConsumerArgs *fused_consumer; bool consumer_b_inline;     // the loss stage's kernel C (and B) inside this one
    uint32_t *det_max; unsigned long long *det_acc;                 // deterministic accumulation, two launches ...
    const uint8_t *det_prev; const uint32_t *det_gex; uint32_t *det_flag;   // ... or one, with predicted scales
    const uint32_t *block_order; uint32_t order_tag;    // the caller's launch order, or ...
    bool order_in_handover;                             // ... the one the staged forward left in the hand-over buffer
};
int launch_render_bwd(const DevCam &cam, const RenderBwdLaunch &a, hipStream_t st);

// ---- sls_consumer.hip ----------------------------------------------------------------------------------------------
size_t consumer_scratch_bytes(int H, int W);
// in: the kernels' own argument struct, the caller's fields filled by name (sizes, weights, inputs, sums, dL_dallmap, the
// launch-order passenger); the launcher adds the derived ones.  no_launch: kernel B too runs inside the tile backward.
// args_out_skip_c (optional, out): the complete arguments for the tile backward, which then does kernel C's work
int launch_consumer(const ConsumerArgs &in, int n_valid, void *scratch, size_t scratch_bytes, bool no_launch, hipStream_t st,
                    ConsumerArgs *args_out_skip_c);
int launch_render_maps(int H, int W, const float *allmap, const float *rot9, const float *col_h, const float *row_h,
                       float depth_ratio, float *rend_normal, float *surf_depth, float *surf_normal, hipStream_t st);
int launch_densify_weights(int H, int W, const float *depth, const uint8_t *valid, const float *alpha, float thr, float *w_out,
                           uint32_t *stats, hipStream_t st);
int launch_densify_rows(int n, int H, int W, const int64_t *pix, const float *depth, const float *normal, const float *col_h,
                        const float *row_h, const float *c2w, const float *mTf, float *xyz, float *quat, hipStream_t st);

// ---- sls_densify.hip, sls_surface.hip, sls_knn.hip, sls_exchange.hip, sls_api.hip ----------------------------------
size_t densify_draw_scratch_bytes(int H, int W);
int launch_densify_draw(int H, int W, const float *depth, const uint8_t *valid, const float *alpha, float thr, double percentage,
                        uint64_t seed, uint32_t draw_index, float *w_out, int64_t *pixels_out, uint32_t *stats,
                        uint32_t *stats_mirror, void *scratch, hipStream_t st);
size_t surface_scratch_bytes(int H, int W);
int launch_surface_samples(int H, int W, const float *allmap, const float *col_h, const float *row_h, const float *M,
                           float min_opacity, float max_depth_dist, float depth_ratio, int n_samples, uint64_t seed,
                           uint32_t frame_id, float *points, float *normals, int32_t *pixels, uint32_t *status, void *scratch,
                           hipStream_t st);
size_t knn_scratch_bytes(int M);
int launch_knn(int M, const float *xyz, float *out, void *scratch, size_t scratch_bytes, hipStream_t st, int Mq);   // Mq < 0: all
size_t nn_scratch_bytes(int Mt, int Mq);
// (both: the arguments are checked by the caller, sls_api.hip — sizes, pointers, scratch size and alignment)
int launch_nn_query(int Mt, const float *target_xyz, int Mq, const float *query_xyz, float *out_dist2, int32_t *out_index,
                    void *scratch, hipStream_t st);
// the k nearest (sls_knn.hip).  Every output may be null; out_last_key: the k-th key of every query's list.  k_max: the
// caller's own limit, SLS_NN_K_MAX everywhere but in sls_normals.hip (SLS_NORMALS_NN_MAX = 2 * SLS_NN_K_MAX).  Beyond
// SLS_NN_K_MAX the list is found in two passes: out_mean must be null and out_last_key [Mq] must be given — it carries the
// 32nd key from the first pass to the second and holds that key afterwards.  The scratch does not depend on k:
// nn_scratch_bytes(Mt, Mq)
size_t nn_k_scratch_bytes(int Mt, int Mq, int k);
int launch_nn_query_k(int Mt, const float *target_xyz, int Mq, const float *query_xyz, int k, int k_max, float *out_dist2,
                      int32_t *out_index, double *out_mean, uint64_t *out_last_key, void *scratch, hipStream_t st);
// One target index queried many times (sls_icp.hip): nn_index_target builds it once, scratch laid out as for
// launch_nn_query(Mt, .., Mq, ..); the caller's own kernel then writes, per round, the Mq queries' curve codes
// (curve_code(.., bbox, key_bits), sls_geom.hpp) to qkeys and the identity to qvals, and nn_index_query sorts them,
// gathers the queries from query_xyz and searches.  Mq >= 1.
struct NnIndexRef {
    const uint32_t *bbox, *tkeys;
    uint32_t *qkeys, *qvals;
    int key_bits;
};
int nn_index_target(int Mt, const float *target_xyz, int Mq, void *scratch, hipStream_t st, NnIndexRef *ref);
int nn_index_query(int Mt, int Mq, const float *query_xyz, const NnIndexRef &ref, float *out_dist2, int32_t *out_index, void *scratch,
                   hipStream_t st);
// The host side of the point index, for the files that build one of their own or sort queries along its curve
// (sls_meshdist.hip, sls_cluster.hip).  The scratch of an index (every array 256-byte aligned) ...
struct KnnScratch {
    uint32_t *bbox;
    uint32_t *keys, *keys_tmp;
    uint32_t *vals, *vals_tmp;
    float4 *pts, *boxes, *subboxes;
    void *sort;
    size_t sort_bytes, total;
};
// ... and of a two-cloud query: the target's index (its sorter scratch sized for the larger cloud), then the queries' buffers
struct NnScratch {
    KnnScratch t;
    uint32_t *qkeys, *qkeys_tmp, *qvals, *qvals_tmp;
    float4 *qpts;
    size_t total;
};
// what a two-cloud launcher holds before its query kernel
struct NnFront {
    NnScratch s;
    const uint32_t *tkeys, *qkeys;      // the sorted codes of the targets and of the queries
    const float4 *qpts;
};
KnnScratch knn_layout(int M, void *base, int sort_items);       // sort_items: what the sorter's scratch, the last piece, is sized for
NnScratch nn_layout(int Mt, int Mq, void *base);
int knn_key_bits(int M);                                        // small clouds are sorted on 21 code bits, the others on 30
// bounding cube, Hilbert codes, sort, points in curve order, boxes and sub-boxes.  M2: the item count of a second sort that
// follows (bbox[7]).  *which: where the sorted (code, index) pairs ended up
int knn_build(int M, const float *xyz, const KnnScratch &s, int key_bits, uint32_t M2, hipStream_t st, int *which);
// the queries' codes in the cube of an index (a point outside is clamped to the border cells) and the identity ...
int nn_query_codes(int Mq, const float *query_xyz, const uint32_t *bbox, uint32_t *qkeys, uint32_t *qvals, int key_bits, hipStream_t st);
// ... and behind codes that are in f->s.qkeys / qvals: the sort (Mt decides the key bits) and the gather in curve order
int nn_front_sorted_queries(int Mt, int Mq, const float *query_xyz, hipStream_t st, NnFront *f);
// ---- sls_metrics.hip: the sums and the colours of an array of distances, unsigned or signed (checked by sls_api.hip) --
int launch_nn_stats(int M, const float *dist2, float truncation, float threshold, int include_truncated, uint64_t *out_stats,
                    void *scratch, hipStream_t st);
int launch_signed_stats(int M, const float *sdist, float truncation, uint64_t *out_words, void *scratch, hipStream_t st);
int launch_error_colors(int M, const float *dist2, float truncation, uint8_t *out_rgb, hipStream_t st);
int launch_signed_error_colors(int M, const float *sdist, float truncation, uint8_t *out_rgb, hipStream_t st);
// ---- sls_meshdist.hip: the nearest triangle of a mesh, the same sweep over an index of triangles (the arguments are
// checked by the caller, sls_api.hip).  Mq == 0: only the status is written
size_t mesh_distance_scratch_bytes(int V, int F, int Mq);
int launch_mesh_distance(int V, const float *vertices, int F, const int32_t *faces, int Mq, const float *query_xyz,
                         float *out_dist2, int32_t *out_face, float *out_closest, uint32_t *out_status, void *scratch,
                         hipStream_t st);
// the index of triangles behind it, which the ray caster shares (TriItem: sls_sweep.hpp).  The
// caller lays the arrays out: F words each of keys / vals and their ping-pong copies, F items, 2 float4 per box of 256 and
// per sub-box of 32, 8 words of bbox, the sorter's scratch for F items
struct TriItem;
struct TriIndexBuild {
    uint32_t *bbox, *keys, *keys_tmp, *vals, *vals_tmp;
    TriItem *items; float4 *boxes, *subboxes;
    void *sort; size_t sort_bytes;
};
int tri_index_build(int V, const float *vertices, int F, const int32_t *faces, const TriIndexBuild &b, uint32_t count2,
                    uint32_t *out_status, uint32_t word3, bool counts_only, hipStream_t st, int *which);
// ---- sls_raycast.hip: first hits of rays against a mesh (the arguments are checked by the caller, sls_api.hip) -------
size_t mesh_rayindex_bytes(int V, int F);
int launch_mesh_rayindex_build(int V, const float *vertices, int F, const int32_t *faces, void *index, uint32_t *out_status,
                               hipStream_t st);
// Mr == 0: only the status is written.  out_face and out_uv may be null
struct RaycastLaunch {
    int V; const float *vertices; int F; const int32_t *faces; const void *index;
    int Mr; const float *origins, *directions; float t_min, t_max;
    float *out_t; int32_t *out_face; float *out_uv; uint32_t *out_status;
};
int launch_mesh_raycast(const RaycastLaunch &a, hipStream_t st);
// ---- sls_signdist.hip: the signed distance to a mesh (the arguments are checked by the caller, sls_api.hip) ---------
size_t mesh_pseudonormals_scratch_bytes(int V, int F);
int launch_mesh_pseudonormals(int V, const float *vertices, int F, const int32_t *faces, float *out_face_normals,
                              float *out_edge_normals, float *out_vertex_normals, uint32_t *out_status, void *scratch, hipStream_t st);
size_t mesh_signed_distance_scratch_bytes(int V, int F, int Mq);
// Mq == 0: only the status is written.  out_face, out_closest and out_feature may be null
struct SignedDistanceLaunch {
    int V; const float *vertices; int F; const int32_t *faces; const float *face_n, *edge_n, *vertex_n;
    int Mq; const float *query_xyz;
    float *out_sdist; int32_t *out_face; float *out_closest; uint8_t *out_feature; uint32_t *out_status; void *scratch;
};
int launch_mesh_signed_distance(const SignedDistanceLaunch &a, hipStream_t st);
// ---- sls_icp.hip (the arguments are checked by the caller, sls_api.hip; init_pose12: host memory) ------------------
size_t cloud_icp_scratch_bytes(int Ms, int Mt);
int launch_cloud_icp(int Ms, const float *source_xyz, int Mt, const float *target_xyz, const float *target_normals,
                     const SlsIcpParams &prm, const double *init_pose12, uint64_t *out_status, double *out_system,
                     int32_t *out_index, float *out_dist2, void *scratch, hipStream_t st);
// ---- sls_outlier.hip (the arguments are checked by the caller, sls_api.hip) ----------------------------------------
size_t outlier_scratch_bytes(int M, int k);
int launch_outlier_statistical(int M, const float *xyz, const float *normals, int k, double std_ratio, float *out_xyz,
                               float *out_normals, int32_t *out_index, uint64_t *out_status, void *scratch, hipStream_t st);
int launch_outlier_radius(int M, const float *xyz, const float *normals, int nb_points, float radius, float *out_xyz,
                          float *out_normals, int32_t *out_index, uint64_t *out_status, void *scratch, hipStream_t st);
// ---- sls_cluster.hip (the arguments are checked by the caller, sls_api.hip; M == 0: only the status is written) ----
size_t cloud_dbscan_scratch_bytes(int M);
int launch_cloud_dbscan(int M, const float *xyz, float eps, int min_points, int32_t *out_labels, int32_t *out_counts,
                        uint32_t *out_status, void *scratch, hipStream_t st);
size_t cloud_select_scratch_bytes(int M);
int launch_cloud_select(int M, const float *xyz, const float *normals, const int32_t *labels, const int32_t *counts,
                        const uint32_t *cluster_status, int keep, int min_cluster_points, float *out_xyz, float *out_normals,
                        int32_t *out_index, uint32_t *out_status, void *scratch, hipStream_t st);
// ---- sls_normals.hip (the arguments are checked by the caller, sls_api.hip; viewpoint3: host memory) ---------------
size_t cloud_normals_scratch_bytes(int M, int k);
int launch_cloud_normals(int M, const float *xyz, int k, float radius, const float *viewpoint3, float *out_normals,
                         int32_t *out_count, float *out_eigenvalues, void *scratch, hipStream_t st);
// ---- sls_ground.hip (the arguments are checked by the caller, sls_api.hip; M == 0: only the status is written) -----
size_t ground_scratch_bytes(int M);
int launch_ground_segment(int M, const float *xyz, const SlsGroundParams &prm, uint8_t *out_label, int32_t *out_bin,
                          double *out_planes, int32_t *out_info, uint32_t *out_status, void *scratch, hipStream_t st);
// ---- sls_cloud.hip (the arguments are checked by the caller, sls_api.hip) ------------------------------------------
size_t voxel_scratch_bytes(int M);
int launch_voxel_downsample(int M, const float *xyz, double voxel_size, float *out_xyz, int32_t *out_count, uint32_t *out_status,
                            void *scratch, hipStream_t st);
size_t mesh_sample_scratch_bytes(int V, int F, int n_samples);
int launch_mesh_sample(int V, const float *vertices, int F, const int32_t *faces, const float *crop_box, int n_samples,
                       uint64_t seed, float *out_xyz, int32_t *out_face, uint32_t *out_status, void *scratch, hipStream_t st);
// ---- sls_tsdf.hip (the arguments are checked by the caller, sls_api.hip) -------------------------------------------
size_t tsdf_blocks_scratch_bytes(int M);
int launch_tsdf_blocks(int M, const float *xyz, double voxel_size, double trunc, const double *origin, int capacity,
                       int32_t *out_blocks, uint32_t *out_status, void *scratch, hipStream_t st);
int launch_tsdf_integrate(const SlsCamera &cam, int B, const int32_t *blocks, float *tsdf, float *weight, const float *allmap,
                          double voxel_size, double trunc, const double *origin, float min_opacity, float max_depth_dist,
                          float depth_ratio, hipStream_t st);
int launch_tsdf_extract_count(int B, const int32_t *blocks, const float *tsdf, const float *weight, float min_weight,
                              uint32_t *counts, uint32_t *prefix, uint32_t *status, hipStream_t st);
int launch_tsdf_extract_emit(int B, const int32_t *blocks, const float *tsdf, const float *weight, float min_weight,
                             double voxel_size, const double *origin, const uint32_t *prefix, uint32_t T, float *triangles,
                             hipStream_t st);
// ---- sls_poisson.hip (the arguments are checked by the caller, sls_api.hip; origin: host memory) -------------------
size_t poisson_splat_scratch_bytes(int M, int B);
int launch_poisson_splat(int M, const float *xyz, const float *normals, int B, const int32_t *blocks, double voxel_size,
                         const double *origin, float *out_field, uint32_t *out_status, void *scratch, hipStream_t st);
size_t poisson_solve_scratch_bytes(int B);
int launch_poisson_solve(int B, const int32_t *blocks, const float *field, double alpha, int iterations, double tol, float *out_chi,
                         uint64_t *out_status, void *scratch, hipStream_t st);
size_t poisson_density_scratch_bytes(int B);
int launch_poisson_density(int B, const int32_t *blocks, const float *field, int sweeps, float *out_density, void *scratch, hipStream_t st);
// ---- sls_mesh.hip (the arguments are checked by the caller, sls_api.hip) -------------------------------------------
size_t mesh_weld_scratch_bytes(int64_t n_rows);
int launch_mesh_weld(int n_rows, const float *soup, float *out_vertices, int32_t *out_index, uint32_t *out_status, void *scratch,
                     hipStream_t st);
size_t mesh_clusters_scratch_bytes(int T);
int launch_mesh_clusters(int T, const int32_t *faces, int V, int32_t *out_labels, int32_t *out_counts, uint32_t *out_status,
                         void *scratch, hipStream_t st);
size_t mesh_filter_scratch_bytes(int V, int T);
int launch_mesh_filter(int V, const float *vertices, int T, const int32_t *faces, const int32_t *labels, const int32_t *counts,
                       const uint32_t *cluster_status, int keep_clusters, int min_triangles, float *out_vertices, int32_t *out_faces,
                       int32_t *out_vmap, uint32_t *out_status, void *scratch, hipStream_t st);
size_t mesh_normals_scratch_bytes(int V, int T);
int launch_mesh_vertex_normals(int V, const float *vertices, int T, const int32_t *faces, float *out_normals, void *scratch,
                               hipStream_t st);
// its sort of the 3 T corners by vertex (T >= 1; scratch: mesh_normals_scratch_bytes), which sls_signdist.hip shares
int mesh_corner_sort(int V, int T, const int32_t *faces, void *scratch, const uint32_t **keys, const uint32_t **vals, hipStream_t st);
// ---- sls_simplify.hip (the arguments are checked by the caller, sls_api.hip) ---------------------------------------
size_t mesh_simplify_scratch_bytes(int V, int T);
int launch_mesh_simplify(int V, const float *vertices, int T, const int32_t *faces, double voxel_size, int contraction,
                         double regularisation, float *out_vertices, int32_t *out_faces, int32_t *out_vmap, uint32_t *out_status,
                         void *scratch, hipStream_t st);
// ---- sls_smooth.hip (the arguments are checked by the caller, sls_api.hip) -----------------------------------------
size_t mesh_adjacency_scratch_bytes(int V, int T);
int launch_mesh_adjacency(int V, int T, const int32_t *faces, int32_t *out_offsets, int32_t *out_neighbours, uint8_t *out_boundary,
                          uint32_t *out_status, void *scratch, hipStream_t st);
size_t mesh_smooth_scratch_bytes(int V, int T);
int launch_mesh_smooth(int V, const float *vertices, int T, const int32_t *faces, int method, int weights, int iterations,
                       double lambda, double mu, int fix_boundary, float *out_vertices, uint32_t *out_status, void *scratch,
                       hipStream_t st);

// ---- sls_fill.hip (the arguments are checked by the caller, sls_api.hip) -------------------------------------------
size_t mesh_fill_scratch_bytes(int V, int T);
int launch_mesh_boundary_loops(int V, int T, const int32_t *faces, const uint32_t *in_counts, int32_t *out_halfedges, int32_t *out_loop,
                               int32_t *out_loop_edges, uint32_t *out_status, void *scratch, hipStream_t st);
int launch_mesh_fill_holes(int V, const float *vertices, int T, const int32_t *faces, const uint32_t *in_counts, int max_edges,
                           double max_size, int cap_vertices, float *out_vertices, int cap_triangles, int32_t *out_faces,
                           uint32_t *out_status, void *scratch, hipStream_t st);
int launch_mesh_fill_empty(int V, const float *vertices, int T, const int32_t *faces, const uint32_t *in_counts, int fills,
                           float *out_vertices, int cap_triangles, int32_t *out_faces, uint32_t *out_status, hipStream_t st);
int launch_touched_bitmap(int N, const uint8_t *touched, const float *scaling_raw, float smax, float pen,
                          const uint32_t *status_block, uint64_t *bitmap, hipStream_t st);
int launch_adam(const SlsAdamGroup *groups, int ngroups, double beta1, double beta2, double eps, int64_t step,
                const uint32_t *skip_flag, hipStream_t stream, const float *void_flags, uint32_t *status_block,
                uint32_t *status_mirror);

}  // namespace sls

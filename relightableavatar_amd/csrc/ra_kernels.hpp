// Launchers of the non-MLP kernels (ra_hdq.hip, ra_trace.hip).
#pragma once
#include "ra_common.hpp"
#include "ra_lpips_pack.hpp"

// where the query points of a pass come from
struct RaySet {
    int mode;             // 0: x[i];  1: o[i] + t[i] d[i];  2: o[pix[i]] + t[i] ldir[light[i]]
    const float* x;       // mode 0: n x 3
    const float* o;       // mode 1: n x 3; mode 2: n_pix x 3
    const float* d;       // mode 1: n x 3
    const float* t;       // modes 1,2: n
    const int* pix;       // mode 2
    const int* light;     // mode 2
    const float* ldir;    // mode 2: n_lights x 3 (unit)
    const int* n_dev;     // optional device-side count (<= n launched); nullptr -> n
    const unsigned char* skip;   // optional: ray i did not move since its last query -> its sdf[i] is still valid, do not re-query
    // optional: the three nearest vertices every query of this pass finds are written here (3 ints per ray), and — with hint_valid — read
    // first: the neighbours a ray found one tracing iteration ago give its bounds at the new point at once (3 distance evaluations instead
    // of a seed search + a 32-candidate leaf scan dense in insertions, in EVERY wave of a split workgroup); any vertex is a valid
    // candidate, so the result stays the exact 3-NN
    int* nn_hint;
    int hint_valid;
    // optional, for a loop's FIRST pass: start from another pass's neighbours — query i reads the triplet hint_src[3 * hint_src_index[i]]
    // (the shadow rays of a hit pixel start next to the point whose neighbours the surface trace found last).  Takes precedence over
    // nn_hint as the source; nn_hint is still written.
    const int* hint_src;
    const int* hint_src_index;
};

struct HdqOut {
    float* sdf;           // n: coarse signed distance (smpl_sdf after the abs rule)
    int* fine_count;      // device counter, ZERO on entry (a fresh one per pass: ra_api.cpp next_fine_counter)
    int* fine_idx;        // slot -> point
    float* bpts;          // slot x 3
    float* mats;          // slot x 24 or nullptr
    // optional second fine list (the key-light tier, ra_config.key_light_share): fine points of rays towards a light with key[light] != 0
    // (RaySet mode 2) are compacted into fine_idx2 / bpts2 through fine_count2 instead — the list the compensated kernel answers
    const unsigned char* key;   // nullable: n_lights flags
    int* fine_count2;
    int* fine_idx2;
    float* bpts2;
    float* raw_zero;      // nullable: n x raw_C rows that non-fine points zero (Network.forward's zeros outside dist_th)
    int raw_C;
    // debug (nullable): per point
    float* dbg_sdf_batch; // n x 3
    int* dbg_nn_batch;    // n x 3
    float* dbg_d2;        // n x 3 (filtered)
    float* dbg_tpts;      // slot-ordered? no: per point n x 3 (only fine points written)
    float* dbg_bpts;      // n x 3
    float* dbg_mats;      // n x 24
    DevCounters* counters; // nullable
};

void launch_vert_blend(const float* weights, const float* A, const float* big_A, int n_verts, int n_bones, float* vertA,
                       hipStream_t s);
void launch_pack_verts(const float* pverts, int n_verts, float4* out, hipStream_t s);
void launch_fold_bias(const float* W, int ld, int col0, int ncond, const float* cond, const float* bias, float* out,
                      hipStream_t s);   // out[r] = bias[r] + sum_c W[r*ld + col0 + c] * cond[c], r < 256
// per-frame build of the vertex box structure (bbox, Morton codes, ranks, boxes: two launches); n_verts <= 16384
// order: scratch of n_verts ints (the vertices' Morton order, recomputed every frame)
void launch_bvh_build(const float4* pverts4, int n_verts, int* order, float* leaves, float4* sbox, int n_leaves, int n_supers, hipStream_t s);
int bvh_leaf_count(int n_verts);
int bvh_super_count(int n_leaves);
void launch_hdq_coarse(const FrameState& fr, const RaySet& rs, int n, float th, float blend_radius, const HdqOut& out,
                       hipStream_t s, bool geodesic = true);

struct TraceState {       // SoA per ray
    float *t, *d0, *dt, *st, *ot, *cd, *occ, *off, *rlx;
    const float *near_, *far_;
    const float* tan_i;   // per ray (mode 1) or per light (mode 2) or nullptr -> scalar
    const int* light;     // mode 2
    unsigned char* stuck; // ray did not move in the last update (t clamped at far / near): the next query would repeat the last one
};
void launch_trace_init(const TraceState& ts, int n, const int* n_dev, const ra_trace_params& p, hipStream_t s);

void launch_trace_update(const TraceState& ts, const float* sdf, int n, const int* n_dev, int iter,
                         const ra_trace_params& p, hipStream_t s);

// surface pass epilogue: surf/depth/acc, hit compaction (hit_count: zeroed here unless counter_is_zero), slot_of_ray[r] = -1 for every ray
void launch_surface_finish(const float* ray_o, const float* ray_d, const float* st, const float* occ, int P, float* surf,
                           float* depth, float* acc, int* hit_idx, int* hit_count, hipStream_t s, int* slot_of_ray = nullptr,
                           bool counter_is_zero = false);
// slot_of_ray[hit_idx[k]] = k for the (possibly re-ordered) hit list
void launch_slot_index(const int* hit_idx, const int* hit_count, int P, int* slot_of_ray, hipStream_t s);
// every requested output map of a chunk in ONE launch: per ray either its hit slot's values (optionally times acc) or zeros
struct MapJob { const float* src; float* dst; int C; int premul; int src_full; };
constexpr int RA_MAX_MAP_JOBS = 16;
struct EmitMaps { MapJob job[RA_MAX_MAP_JOBS]; long long end[RA_MAX_MAP_JOBS]; int n_jobs; const int* slot_of_ray; const float* acc; const int* perm; int P; };
void launch_emit_maps(const EmitMaps& m, hipStream_t s);
// 3 (S) samples per hit pixel: x = surf + z * view
void launch_surface_samples(const float* surf, const float* ray_d, const int* hit_idx, const int* hit_count, int P, int S,
                            float range, float* x, float* v, int* n_out, hipStream_t s);
// per hit pixel: composite S samples of raw (C channels, last = occ), normalise, split
struct SurfaceMaps {      // per hit slot
    float *cpts, *bpts, *resd, *norm, *albedo, *rough, *rgb;
    float* valbedo;       // nullable: clipped albedo before cfg.albedo_multiplier (ret.volume_albedo, :646)
};
void launch_surface_composite(const float* raw, int C, int S, const int* hit_count, int P, int relight, const ra_config& cfg,
                              const SurfaceMaps& m, hipStream_t s);

// shadow rays
constexpr int RA_MAX_BOXES = 32;
struct ShadowGen {
    const float* surf;    // P x 3 (full ray indexing)
    const float* norm;    // hit-slot x 3
    const float* acc;     // P
    const int* hit_idx;   // slot -> ray
    const int* hit_count;
    const float* ldir;    // L x 3 unit light directions
    float bbox[6];
    // several render chunks of the reference in ONE launch (the ground pass): ray r belongs to chunk j with box_start[j] <= r < box_start[j + 1]
    // and is clipped against boxes[j] — the box the reference's in-place growth (sphere_tracing_renderer.py:1054-1056) had reached at that
    // chunk, computed by the caller with the same float arithmetic.  n_boxes <= 1: every ray uses bbox.
    int n_boxes;
    float boxes[RA_MAX_BOXES][6];
    int box_start[RA_MAX_BOXES + 1];
    const int* perm;      // nullable: the rays were re-ordered (Morton sort) — ray r is the caller's ray perm[r], which is what box_start counts
    float near_offset;
    int L;
    int no_visibility, local_visibility;
    int split_wide_groups;   // a group of 64 hit slots wider than 15 cm emits its rays half by half (the human layer; see shadow_gen_kernel)
    // out
    float* lvis;          // slot x L
    float* ldot;          // slot x L
    int* ray_pix;         // ray -> full ray index (origin = surf[pix])
    int* ray_light;
    int* ray_slot;        // ray -> slot*L + light (where occ lands)
    float *near_, *far_;
    int* ray_count;
};
// key[l] = light l holds at least the fraction max(share, 4 / L) of a probe's power under any of the frame's probes — the kmax lights with
// the largest such share at most.  smax (L floats): every light's largest share so far; accumulate: the n probes join those of earlier calls
void launch_key_lights(const float* probes, int n, int ph, int pw, const float* ldir, const float* area, int L, float share, int kmax,
                       int accumulate, float* smax, unsigned char* key, hipStream_t s);
void launch_gather_shard_rays(const long long* idx, int n, const float* ro, const float* rd, const float* nr, const float* fr, float* so, float* sd,
                              float* sn, float* sf, hipStream_t s);
void launch_scatter_rows(const float* src, const long long* src_idx, const long long* dst_idx, long long n, int C, float* dst, hipStream_t s);
void launch_shadow_gen(const ShadowGen& g, int P, hipStream_t s, bool counter_is_zero = false);
void launch_debug_aabb(const float* o, const float* d, int n, const float* bbox6, float* nr, float* fr, hipStream_t s);
void launch_debug_brdf(const float* p2l, const float* p2c, const float* nrm, const float* alb, const float* rough, int L, int N, const ra_config& cfg,
                       float* out, hipStream_t s);
// reorder the hit list so that 64 consecutive hit pixels have neighbouring surface points (radix sort by Morton key)
size_t sort_hits_temp_bytes(int P);
int launch_sort_hits(const float* surf, const float* acc, int P, const float* bbox_min, unsigned* keys_in, unsigned* keys_out,
                     int* vals_in, int* hit_idx_out, void* temp, size_t temp_bytes, hipStream_t s);
void launch_shadow_scatter(const float* occ, const int* ray_slot, const int* ray_count, int max_rays, float* lvis, hipStream_t s);

struct ShadeIn {
    const float* ray_o;   // indexed by ray (idx != null) or by slot
    const float* surf;    // same indexing
    const int* idx;       // slot -> ray or nullptr (identity)
    const int* count;     // device count or nullptr -> n
    int n;
    const float *norm, *albedo, *rough;   // per slot
    const float *lvis, *ldot;             // slot x L
    const float *light_xyz, *light_area;  // L x 3, L
    int L;
    const float* probes;  // n_probes x h x w x 3
    int n_probes, ph, pw;
    int want_spec;
    float *rgb, *shade, *spec;            // n_probes x n x 3 (slot indexed)
};
void launch_shade(const ShadeIn& in, const ra_config& cfg, hipStream_t s);

// backward of the re-shade (ra_shade_bwd.hip): d rgb -> d albedo, d roughness, d probes; pixel indexed, all P pixels live
constexpr int SHADE_BWD_MAX_GRID = 768;          // workgroups (= partial slabs) at most; the grid depends on P alone
constexpr size_t SHADE_BWD_LDS_BYTES = 65536;    // LDS budget of the probe tiles of one launch
struct ShadeBwd {
    const float *ray_o, *surf, *norm, *albedo, *rough;   // P x 3 / P
    const float* lvis;                                    // P x L
    const float *light_xyz, *light_area; int L;
    const float* probes; int n_probes, ph, pw;            // any number of probes: several launches
    const float* d_rgb;                                   // n_probes x P x 3
    int P;
    float *d_albedo, *d_rough, *d_probes;                 // P x 3, P, n_probes x ph x pw x 3; nullable; overwritten
    float* slabs;                                         // shade_bwd_grid(P) x shade_bwd_probes_per_launch(ph, pw) x (ph pw 3) floats (needed with d_probes)
};
int shade_bwd_grid(int P);
int shade_bwd_probes_per_launch(int ph, int pw);          // 0: one probe's tile does not fit the LDS budget
void launch_shade_bwd(const ShadeBwd& a, const ra_config& cfg, hipStream_t s);

// the material heads on cached features, forward and weight gradient (ra_heads.hip); theta / d_theta: the flat layout of ra_heads_param_count
constexpr int HEADS_PARAMS = 99332;
constexpr int HEADS_MAX_GRID = 128;              // workgroups (= partial slabs of HEADS_PARAMS floats) at most; the grid depends on n alone
constexpr int HEADS_CHUNK = 32768;               // points the tape holds (a multiple of the 64-point tile); longer calls run in chunks
constexpr size_t HEADS_TAPE_BYTES_PER_TILE = 163840;      // f16 activations and scaled deltas of a 64-point tile, both heads
constexpr size_t HEADS_W16_BYTES = 2 * 66048 * 2;         // the f16 images of the weights
struct HeadsIO {
    const float *theta, *feat;                            // HEADS_PARAMS; n x 256
    int n;
    float *albedo, *rough;                                // forward: n x 3, n (nullable)
    const float *d_albedo, *d_rough;                      // backward: n x 3, n (nullable: that head's slice of d_theta is zeroed)
    float* d_theta;                                       // backward: HEADS_PARAMS
    void* w16;                                            // scratch: HEADS_W16_BYTES
    unsigned* amax;                                       // scratch (backward): 2
    void* tape;                                           // scratch (backward): HEADS_TAPE_BYTES_PER_TILE per tile of min(n, HEADS_CHUNK) points
    float* slabs;                                         // scratch (backward): heads_grid(n) x HEADS_PARAMS
};
int heads_grid(int n);
void launch_heads_forward(const HeadsIO& io, const ra_config& cfg, hipStream_t s);
void launch_heads_backward(const HeadsIO& io, const ra_config& cfg, hipStream_t s);

// Gaussian-histogram entropy of an n x 3 sample and its gradient (ra_entropy.hip); scratch: entropy_scratch_doubles(n) doubles
constexpr int ENTROPY_MAX_GRID = 256;            // workgroups (= partial slabs) at most; the grid depends on n alone
int entropy_grid(int n);
size_t entropy_scratch_doubles(int n);
void launch_gaussian_entropy(const float* x, int n, const float* d_value, float* value, float* d_x, double* scratch, hipStream_t s);

// MSE, PSNR, SSIM of one image pair (ra_metrics.hip); scratch: metrics_scratch_bytes(H, W, pix != nullptr) bytes
struct MetricsIO {
    const float *pred, *gt;                               // P x 3
    const long long* pix;                                 // nullable: the maps hold all H*W pixels
    int P;
    const unsigned char* mask;                            // H*W, read with crop_to_mask
    int H, W;
    float bg, data_range;
    int mse_over_rays, crop_to_mask;
    double* out;                                          // 4: mse, psnr, ssim, windows
    void* scratch;
};
size_t metrics_scratch_bytes(int H, int W, bool ray_list);
void launch_image_metrics(const MetricsIO& io, hipStream_t s);

// LPIPS (AlexNet) of one image pair (ra_lpips.hip); scratch: lpips_scratch_bytes(H, W, pix != nullptr) bytes
struct LpipsIO {
    const float *pred, *gt;                               // P x 3
    const long long* pix;                                 // nullable: the maps hold all H*W pixels
    int P;
    const unsigned char* mask;                            // H*W, read with crop_to_mask
    int H, W;
    float bg;
    int crop_to_mask;
    double* out;                                          // 6: the value, the five per-tap terms
    void* scratch;
    const float* arena;                                   // the packed weights on the device (ra_lpips_pack.hpp: lpips_arena())
    LpipsArena off;
};
size_t lpips_scratch_bytes(int H, int W, bool ray_list);
void launch_lpips(const LpipsIO& io, hipStream_t s);
// one image (io.pred == io.gt: H*W x 3, no ray list, no crop; H, W >= LPIPS_MIN_SIDE): the post-ReLU activations of one tap in (C, h, w) order
void launch_lpips_features(const LpipsIO& io, int tap, float* out, hipStream_t s);
void lpips_feature_shape(int H, int W, int tap, int* C, int* h, int* w);

// Exact closest point on a triangle mesh (ra_mesh.hip): a flat box structure over Morton-sorted faces, swept with wave-uniform control flow
constexpr int MESH_LEAF = 32;                    // face records per leaf
constexpr int MESH_FAN = 8;                      // leaves per group
constexpr int MESH_REC = 12;                     // floats per face record: a.xyz b.xyz c.xyz, the original face id (int bits; -1: no face), 2 unused
constexpr int MESH_MAX_FACES = 1 << 24;
constexpr int MESH_SORT_MIN = 64;                // queries of at most one wave of points are never sorted
struct MeshView {
    const float* recs;      // n_leaves x MESH_LEAF records
    const float* lbox;      // n_leaves x 6 (lo, hi): the leaf's valid faces, widened by the rounding of a computed closest point
    const float* gbox;      // n_groups x 6
    int n_faces, n_leaves, n_groups;
};
struct MeshBuild {          // scratch of one build, all on the device
    int* faces;             // n_faces x 3
    unsigned* bb;           // 6 words: the centroids' box as order-preserving integers
    unsigned *keys, *keys_sorted;
    int *vals, *vals_sorted;
    void* temp;
    size_t temp_bytes;
};
struct MeshQuery {
    const float* pts;
    int n, brute;
    const int* perm;        // nullable: thread i answers point perm[i]
    float *d2, *closest, *bary;
    int* face;
};
inline int mesh_leaf_count(int n_faces) { return (n_faces + MESH_LEAF - 1) / MESH_LEAF; }
inline int mesh_group_count(int n_leaves) { return (n_leaves + MESH_FAN - 1) / MESH_FAN; }
size_t mesh_sort_temp_bytes(int n);
int launch_mesh_build(const float* verts, const MeshBuild& b, const MeshView& m, float* recs, float* lbox, float* gbox, hipStream_t s);
// Morton order of the query points (non-finite points last): perm[i] = caller index of the i-th point
int launch_mesh_sort_points(const float* pts, int n, const MeshBuild& b, hipStream_t s);
void launch_mesh_closest(const MeshView& m, const MeshQuery& q, hipStream_t s);

// Generalised winding number over a mesh's own face records (ra_winding.hip): one lane per point, faces summed in stored order
constexpr int WIND_BLOCK = 64;                   // points per workgroup: one wave
constexpr int WIND_CHUNK = 1024;                 // face records per chunk, a constant: a chunk's float64 sum starts from 0, chunk sums add in chunk order
constexpr int WIND_SPLIT_TILES = 2048;           // fewer point tiles than this: one workgroup per (tile, chunk) and a combining pass ...
constexpr long long WIND_SPLIT_MAX = 1ll << 24;  // ... as long as points x chunks float64 partial sums stay within this count (128 MiB)
inline int wind_chunk_count(int n_leaves) { return (int)(((long long)n_leaves * MESH_LEAF + WIND_CHUNK - 1) / WIND_CHUNK); }
// partial: nullptr = the one-pass kernel; else chunks x n float64 of scratch = the split launch (the same bits)
void launch_mesh_winding(const MeshView& m, const float* pts, int n, double* partial, float* out, hipStream_t s);
// The same sweep with the gradient in the point (ra_winding_grad.hip): winding (nullable, n) and grad (n x 3); the same tiles and chunks.
// partial: nullptr = the one-pass kernel; else chunks x 4 x n float64 of scratch = the split launch (the same bits)
void launch_mesh_winding_grad(const MeshView& m, const float* pts, int n, double* partial, float* winding, float* grad, hipStream_t s);

// Ray-mesh intersection over a mesh's box structure, and the dense ray x triangle pairs (ra_raycast.hip)
constexpr int RAY_BLOCK = 64;                    // rays per workgroup: one wave
constexpr int RAY_PAIR_BLOCK = 256;              // pairs per workgroup of the dense kernel
constexpr long long RAY_MAX_PAIRS = 1ll << 31;   // the dense kernel answers fewer pairs than this
struct RayQuery {
    const float *o, *d;     // n x 3 each
    int n, brute;
    const int* perm;        // nullable: thread i answers ray perm[i]
    float *t, *uv;          // nullable outputs; count != nullptr also turns the pruning by t off
    int *face, *count;
};
void launch_mesh_raycast(const MeshView& m, const RayQuery& q, hipStream_t s);
void launch_ray_tri_pairs(const float* o, const float* d, int n, const float* tris, int f, float* u, float* v, float* t, hipStream_t s);

// Mesh connectivity and Taubin smoothing (ra_topo.hip)
constexpr int TOPO_BLOCK = 256;                  // half-edges / edges / vertices per workgroup of the build kernels
constexpr int TOPO_SMOOTH_BLOCK = 256;           // (vertex, channel) results per workgroup of the smoothing and dilation kernels
constexpr int TOPO_MAX_FACES = (1 << 29) / 3;    // 3 F half-edges and their scratch stay far inside int32
constexpr int TOPO_MAX_CHANNELS = 64;
enum { TOPO_BAD = 0, TOPO_E = 1, TOPO_MAX_NBR = 2, TOPO_MAX_OUT = 3, TOPO_MAX_COUNT = 4, TOPO_STAT_INTS = 5 };      // the one read-back of a build
struct TopoView {           // all device arrays, owned by the ra_topo; HE = 3 n_faces
    int n_faces, n_verts, n_edges;
    const int *vert, *twin, *edge;      // HE each
    const int *edges, *counts;          // E x 2, E
    const int *ehe_start, *ehe;         // E + 1, HE: the half-edges of an edge, ascending
    const int *nbr_start, *nbr;         // V + 1, 2 E: the neighbours of a vertex, ascending
    const int *out_start, *out_he;      // V + 1, HE: the half-edges that leave a vertex, ascending
};
struct TopoBuild {          // outputs (the ra_topo's buffers, E-sized ones at their upper bound HE) and the scratch of one build
    const int* faces;
    int n_faces, n_verts;
    int *vert, *twin, *edge, *edges, *counts, *ehe_start, *ehe, *nbr_start, *nbr, *out_start, *out_he;
    unsigned long long *keys, *keys_sorted;
    int *slots, *head, *off, *deg, *odeg, *fill, *stat;
    void* temp;
    size_t temp_bytes;
};
size_t topo_temp_bytes(int n_faces, int n_verts);
int launch_topo_build(const TopoBuild& b, hipStream_t s);
// one Taubin pass: dst = src + c * (mean of the neighbours - src) on the rows with move[v] != 0 (move == nullptr: all), others copied
void launch_topo_smooth_pass(const TopoView& t, const float* src, int C, const unsigned char* move, float c, float* dst, hipStream_t s);
void launch_topo_mark_rows(const long long* inds, int n_inds, int n_verts, unsigned char* move, hipStream_t s);
void launch_topo_dilate_pass(const TopoView& t, const unsigned char* src, unsigned char* dst, hipStream_t s);
// one Loop step (ra_mesh_subdivide).  Positions: (V + E) x C rows from V x C, weights = the (w_self, beta) pairs per valence.
void launch_loop_positions(const TopoView& t, const float* src, int C, const float* weights, float* dst, hipStream_t s);
// The child's connectivity by index arithmetic: every array of `child` (sized for 4 F faces, V + E vertices, 2 E + 3 F edges) from the
// parent's; faces_out (nullable) receives the 4 F x 3 faces.  deg (V' + 1, zero on entry), fill (V', zero on entry), scratch_stat
// (TOPO_STAT_INTS) and temp are scratch.  No sort, no read-back.
struct TopoChild {
    int *vert, *twin, *edge, *edges, *counts, *ehe_start, *ehe, *nbr_start, *nbr, *out_start, *out_he;
    int *deg, *fill, *scratch_stat;
    void* temp;
    size_t temp_bytes;
};
int launch_topo_child(const TopoView& t, const TopoChild& c, int* faces_out, hipStream_t s);

// Mesh fitting (ra_fit.hip): the operator M = I + lambda L on a topology's neighbour lists and its conjugate-gradient solve, normals, the
// ICP residual, the AdamUniform step
constexpr int FIT_BLOCK = 256;                   // vertices of one channel per workgroup of the solve; rows per workgroup of the residual
constexpr int FIT_MAX_CHANNELS = TOPO_MAX_CHANNELS;
enum { FIT_STOP_NONE = 0, FIT_STOP_CONVERGED = 1, FIT_STOP_ZERO = 2, FIT_STOP_NAN = 3, FIT_STOP_BREAKDOWN = 4 };
struct FitState { double rz, alpha, beta, bb, relres; int stop, iters; };      // of one channel, on the device
struct FitInfo { int iters, stop; double relres; };                            // what ra_topo_diffuse_solve reports per channel
struct FitSolve {
    const int *nbr_start, *nbr;
    int n_verts, C, n_tiles;        // n_tiles = workgroups per channel
    const float *b, *x0;            // x0 nullable: 0
    double lambda, tol;
    double *x, *r, *z, *p0, *p1, *q;        // C x n_verts each (channel-major)
    double* diag;                   // n_verts: M's diagonal, the Jacobi preconditioner
    double* part;                   // 3 x C x n_tiles partial sums
    FitState* st;                   // C
};
struct IcpJob {
    const float *pts, *pt_normals, *face_normals, *d2, *closest;
    const int* face;
    int n, n_faces, n_tiles;
    float dist_th, angle_th;
    unsigned char* keep;            // n
    double* part;                   // 2 x n_tiles
};
void launch_fit_apply(const TopoView& t, const float* x, int C, double lambda, float* out, hipStream_t s);
void launch_fit_solve(const FitSolve& f, int max_iter, float* out, FitInfo* info, hipStream_t s);
void launch_mesh_normals(const TopoView& t, const float* verts, float* fn, float* area, float* vn, hipStream_t s);
void launch_icp_residual(const IcpJob& j, double* sums, float* grad, hipStream_t s);
void launch_adam_uniform(float* param, const float* grad, float* g1, float* g2, long long n, unsigned* scratch, double lr, double b1, double b2, double c1,
                         double c2, hipStream_t s);

// Cloth energies (ra_cloth.hip): StVK stretch per face, dihedral bending per hinge (addressed by edge id), gravity, inertia
constexpr int CLOTH_BLOCK = 256;                 // (row, face) / (row, edge) / (row, vertex) elements per workgroup
constexpr int CLOTH_CHUNK = 2048;                // consecutive elements of one row per workgroup of an energy sum
struct ClothBuild {
    const float *rest, *vm;         // V x 3 rest positions, n_vm x 2 material coordinates
    const int* fm;                  // F x 3 into vm, checked
    float density;
    float *frec, *f_area, *dm, *dm_inv;     // F x 8 records, F, F x 4, F x 4
    int *hrec, *h_faces, *h_verts;          // E x 8 records, E x 2, E x 2 (-1: no hinge)
    float *mass, *inv_mass;                 // V
    int *vh, *vh_count;                     // 9 F (the segment of vertex v starts at 3 out_start[v]), V
};
struct ClothJob {
    const float* x;                 // B x V x 3
    int B, n_faces, n_edges, n_verts, terms;
    float thickness, mu, lambda, bending, gravity;
    const float* frec;
    const int* hrec;
    const float* mass;
    const int *vh, *vh_count;
    float *e_face, *e_hinge, *e_vert;       // B x F, B x E, B x V element energies
    float *g_face, *g_hinge;                // B x F x 9, B x E x 18 corner gradients (only with grad)
    double* part;                           // B x chunks of the largest element count
    float* grad;                            // nullable: B x V x 3
};
struct InertiaJob {
    const float *mass, *x_next, *x_curr, *v_curr;
    int rows, V, has_accel;
    float dt, accel[3];
    float* el;                      // rows x V
    double* part;
    float *g_next, *g_curr, *g_vel; // nullable
};
void launch_cloth_check_fm(const int* fm, int n_faces, int n_vm, int* bad, hipStream_t s);
void launch_cloth_build(const TopoView& t, const ClothBuild& b, hipStream_t s);
void launch_cloth_energy(const TopoView& t, const ClothJob& j, double* energy, hipStream_t s);
void launch_cloth_inertia(const InertiaJob& j, double* value, hipStream_t s);

// Mesh rasterisation (ra_raster.hip): face records, (tile, face) binning, one wave per 8 x 8 tile; attribute interpolation; both backwards
constexpr int RASTER_BLOCK = 256;                // (view, face) / (pixel, channel) / (view, vertex) elements per workgroup; the tile and face passes use one wave
constexpr int RASTER_MAX_FACES = 1 << 24;        // a face id fits the low 24 bits of a (tile, face) key, and survives a float
constexpr int RASTER_MAX_CHANNELS = 64;
struct RasterJob {
    const float* pos;               // B x V x 4 clip-space positions
    const int* faces;               // F x 3, checked by the set-up kernel
    int B, V, F, H, W;
    float4* recs;                   // B x F x 5: the face records (ra_raster_rules.hpp)
    unsigned long long *counts, *off;       // B F + 1 each: tiles per (view, face) and their exclusive sum; counts == nullptr: no binning
    unsigned long long *keys, *keys_sorted; // the (tile, face) pairs
    int* stat;                      // 2: the pair count (saturated), the index flag; zero on entry
    void* temp;
    size_t temp_bytes;
    float *uv, *zw;                 // B x H x W x 2, B x H x W
    int* face;                      // B x H x W
};
struct InterpJob {
    const float* attr;              // V x A, or B x V x A with per_view
    const int* faces;               // F x 3
    const float* uv;
    const int* face;
    int B, V, F, H, W, A, per_view;
    float* out;                     // B x H x W x A (forward only)
};
struct RasterBwdJob {
    const float *pos, *uv, *duv;    // B x V x 4, B x H x W x 2 twice
    int B, H, W;
    float* dpos;                    // B x V x 4
};
size_t raster_temp_bytes(long long n_scan, long long n_sort);
int launch_raster_setup(const RasterJob& j, hipStream_t s);
int launch_raster_tiles(const RasterJob& j, long long n_pairs, hipStream_t s);
void launch_interpolate(const InterpJob& j, hipStream_t s);
int launch_raster_pixel_sort(const int* face, int B, int F, int H, int W, unsigned long long* keys, unsigned long long* keys_sorted, void* temp,
                             size_t temp_bytes, hipStream_t s);
void launch_interpolate_backward(const InterpJob& j, const TopoView& t, const unsigned long long* keys_sorted, const float* dout, float* g_face, float* dattr,
                                 float* duv, hipStream_t s);
void launch_rasterize_backward(const RasterBwdJob& j, const TopoView& t, const unsigned long long* keys_sorted, float* g_face, hipStream_t s);

// scatter hit-slot maps into full-ray outputs (zeros elsewhere), optional premultiplication by acc
// src_full: src is indexed by ray (like dst) instead of by hit slot
void launch_scatter_maps(const int* hit_idx, const int* hit_count, int P, int premultiply, const float* acc_full,
                         const float* src, int C, float* dst, int src_full, const int* perm, hipStream_t s);
// Morton-sort the primary rays of a chunk by their entry point and gather them into so/sd/sn/sf; perm[i] = caller index of sorted ray i
int launch_sort_rays(const float* ro, const float* rd, const float* nr, const float* fr, int P, const float* bbox_min, unsigned* keys_in,
                     unsigned* keys_out, int* vals_in, int* perm, void* temp, size_t temp_bytes, float* so, float* sd, float* sn, float* sf,
                     hipStream_t s, float near_min = -3.0e38f, float far_max = 3.0e38f);
void launch_accumulate(const int* count, unsigned long long* dst, hipStream_t s);

// volume path
void launch_volume_samples(const float* ray_o, const float* ray_d, const float* near_, const float* far_, int P, int S,
                           float* x, float* v, hipStream_t s);
void launch_volume_composite(const float* raw, int C, const float* near_, const float* far_, int P, int S, float bg,
                             const ra_render_out& out, const int* perm, hipStream_t s);
void launch_fill(float* p, size_t n, float v, hipStream_t s);
void launch_iota(int* idx, int n, int* count, hipStream_t s);      // idx[i] = i, *count = n
void launch_gather_rows(const int* hit_idx, const int* hit_count, int P, const float* src, int C, float* dst, hipStream_t s);   // row k of dst = row hit_idx[k] of src, k < *hit_count
// per point: w2b = big_A_bw @ affine_inverse(A_bw) @ affine_inverse([R|Th]) (or its affine_inverse) from the blended rows of the coarse level
void launch_bigpose_compose(const float* mats, const float* d2, int n, float blend_radius, const float* R, const float* Th, int invert, float* out,
                            hipStream_t s);
void launch_light_dirs(const float* xyz, int L, float* ldir, hipStream_t s);

// N2: ray generation + AABB culling (ra_trace.hip)
struct RayCam { double Kinv[9]; double R[9]; double T[3]; double o[3]; float bmin[3]; float bmax[3]; int H, W; const float* bdev; };   // bdev: the box as 6 device floats (takes precedence)
size_t gen_rays_temp_bytes(int n_pixels);
int launch_gen_rays(const RayCam& cam, unsigned char* mask, int* pix_idx, int* count_dev, void* temp, size_t temp_bytes,
                    float* ray_o, float* ray_d, float* near, float* far, hipStream_t s);

// N1: ground-plane pass (ra_trace.hip)
struct GroundIn {
    const float *ray_o, *ray_d, *acc;     // P
    int P;
    float n[3], orig[3], albedo[3];
    int attach_envmap;
    float env_r, shading_multiplier;
};
// t, surf, clipped depth for every pixel; hit list = pixels with acc > 0; per-slot normal array filled with n
void launch_ground_hit(const GroundIn& g, float* t, float* surf, float* depth, float* norm_slots, int* hit_idx, int* hit_count, hipStream_t s);
struct GroundShade {
    GroundIn g;
    const float* t; const float* surf;
    const int* hit_idx; const int* hit_count;
    const float* lvis;                    // slot x L
    const float *ldir, *light_area; int L;
    const float* probe; int ph, pw;
    float *rgb, *albedo, *shade, *spec;   // P x 3 (full indexing), nullable
    float *lvis_out, *ldot_out;           // P x L (full indexing, pre-zeroed), nullable: what the novel-light re-shade consumes
};
void launch_ground_shade(const GroundShade& in, const ra_config& cfg, hipStream_t s);
struct GroundReshade {                    // novel_light_sphere_tracing.render_ground (:70-99)
    const float *ray_d, *albedo_map;      // P x 3
    const float *lvis, *ldot;             // P x L
    const float *ldir, *light_area; int L;
    const float* probes; int n_probes, ph, pw;
    const float* images; int ih, iw;      // nullable
    int attach_envmap, P;
    float *rgb, *albedo, *shade, *spec;   // n_probes x P x 3, nullable
};
void launch_ground_reshade(const GroundReshade& in, hipStream_t s);

// N4: envmap rotation + light-probe inset (ra_trace.hip)
void launch_grow_bounds(float* wbounds6, float margin, hipStream_t s);
void launch_shift_envmap(const float* img, int H, int W, int C, float shift, float* out, hipStream_t s);
struct ProbeInset { float axes[9]; int H, W, uH, uW, ph, pw; };     // axes: columns = right, -front, -down (gen_light_dir)
void launch_light_probe(const ProbeInset& p, const float* probe, float* rgb, hipStream_t s);
void launch_blend_ground(const float* ground, const float* human, const long long* inds, const float* acc, int F, int P, int C, float* dst,
                         hipStream_t s);

// N3: per-frame body state (ra_trace.hip)
void launch_bone_transforms(const float* staged, int J, float* A, float* joints, float* RT, hipStream_t s);
void launch_lbs_verts(const float* tverts, const float* weights, const float* A, const float* big_A, const float* R, const float* Th,
                      int n_verts, int n_bones, float* tpose, float* pverts, float* wverts, hipStream_t s);
void launch_vert_normals(const float* verts, const int* faces, const int* adj_start, const int* adj, int n_verts, float* normals, hipStream_t s);
void launch_bounds(const float* pts, int n, float padding, float* bounds6, hipStream_t s);


// N4: map -> image normalisations (ra_image.hip)
struct ImageJob {
    int type, P;
    const float *a, *b, *acc;             // main map (P x 3 or P), second map (Residual: bpts), acc (P, nullable -> 1)
    const long long* pix;                 // pixel of every ray (nullable -> identity: full-frame maps)
    const float* stats;                   // device: [k-th smallest, k-th largest] where the type needs a percentile
    float cam_R[9], tbounds[6];
    float min_clip, bg;
    int normalize, tonemap;
    float *image, *alpha;                 // H*W x 3, H*W (nullable)
};
size_t image_sort_temp_bytes(long long n);
int launch_percentiles(const float* vals, long long n, const float* acc_flags, int k, float* scratch_a, float* scratch_b, unsigned char* flag,
                       int* count_dev, void* temp, size_t temp_bytes, float* stats, hipStream_t s);
void launch_diff(const float* a, const float* b, long long n, float* o, hipStream_t s);
void launch_compose_image(const ImageJob& j, long long n_pixels, hipStream_t s);

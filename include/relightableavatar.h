/*
 * relightableavatar.h — C ABI of the MI355X-native render hot path (librelightableavatar_hip.so).
 *
 * The reference (zju3dv/RelightableAvatar) is pure Python and has no FFI of its own; the drop-in
 * boundary is its plugin API: make_network / make_renderer / Renderer.render(batch)
 * (lib/networks/make_network.py:4-7, lib/networks/renderer/make_renderer.py:5-8).  The Python
 * classes in relightableavatar_amd/{networks,renderer} keep that API and bind these entry points
 * with ctypes (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions:
 *  - plain pointers and sizes only; every float* is fp32; "dev" = device (HBM) pointer,
 *    "host" = host pointer.  stream is a hipStream_t passed as void* (torch's current stream);
 *    every launch goes on it, no hidden synchronisation except where stated.
 *  - every function returns 0 on success, non-zero on error; ra_last_error() gives the message
 *    (thread-local).  The library never calls abort().
 *  - all mutable state lives in the opaque ra_ctx (packed weights, frame state, scratch arenas,
 *    work counters).  One ctx per device; a ctx is not thread-safe, distinct ctxs are independent.
 *  - batch size B is 1 (base.yaml:74 test.batch_size 1); arrays are passed without the batch dim.
 */
#ifndef RELIGHTABLEAVATAR_H
#define RELIGHTABLEAVATAR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RA_ABI_VERSION 9
#define RA_N_LIGHTS_MAX 512 /* env_h * env_w = 16 * 32 (lib/config/config.py:111-112) */

typedef struct ra_ctx ra_ctx;

const char* ra_last_error(void);
int ra_abi_version(void);

/* ---- lifetime -------------------------------------------------------------------------- */
int ra_ctx_create(ra_ctx** out, int device);
int ra_ctx_destroy(ra_ctx* ctx);

/* ---- constants the reference reads from its global cfg (lib/config/config.py) ------------ */
typedef struct ra_config {
    int   xyz_res, sdf_res, view_res;         /* 10, 8, 4   (configs/base.yaml:47-49)            */
    int   n_bones;                            /* 52  -> cond_dim = 3 * n_bones                    */
    int   relight;                            /* 1: RelightableAvatar heads, 0: AniSDF colour net */
    float resd_limit;                         /* 0.05 (config.py:224)                             */
    float blend_radius;                       /* 0.075 (config.py:191)                            */
    float albedo_slope, albedo_bias;          /* 1.0, 0.0  (config.py:407-408)                    */
    float roughness_slope, roughness_bias;    /* 0.9, 0.09 (config.py:409-410)                    */
    float fresnel_f0;                         /* 0.02 (config.py:89)                              */
    float shading_albedo;                     /* 0.8  (config.py:394)                             */
    float albedo_multiplier;                  /* 1.0                                              */
    int   lambert_only, glossy_only;          /* ablation switches (config.py:48-49)              */
    int   tonemapping;                        /* cfg.tonemapping_rendering                        */
    float bg_brightness;                      /* 0.0                                              */
    int   mlp_f16;                            /* element type of the fused MLP kernels: 1 = IEEE half, 0 = bfloat16 (same MFMA rate) */
    int   query_skip;                         /* 1 (default): rays that did not move since their last distance query / shadow rays whose
                                                 visibility reached 0 keep their last distance instead of being queried again — exact
                                                 (frames are bit-identical with 0), the reference re-queries them (sphere_tracing_renderer.py:144-205) */
    int   k4_batch_slots;                     /* full queries per forward+backward launch pair (bounds the activation tape: 4.9 KB per slot);
                                                 0 = default (1 Mi slots = 5 GB) */
    int   trace_precision;                    /* arithmetic of the distance queries INSIDE tracing loops.  The reference computes everything in
                                                 fp32; f16 MFMA operands leave the distance 5e-5 rms off, which flips the phase of the surface trace's
                                                 limit cycles on ~1 % of the pixels (sphere_tracing_renderer.py:176-197: hit test, sign-change
                                                 interpolation).  1 (default): the surface trace (16 iterations, 2 % of a relit frame's fine queries)
                                                 runs in COMPENSATED arithmetic — f16 hi + lo operand pairs, three MFMAs per k-step, fp32 accumulate:
                                                 1.3e-7 rms from a float64 evaluation, as good as fp32 itself — the shadow rays stay on plain 16-bit
                                                 operands; 0: plain operands everywhere (round 3's behaviour); 2: compensated everywhere, also
                                                 ra_hdq_sdf / ra_observed_sdf and the shadow rays (validation; 3x the MFMA work) */
    float clip_near, clip_far;                /* 0.02, 10.0: the volume renderer's near.clip(min=clip_near), far.clip(max=clip_far)
                                                 (base_renderer.py:120-121; config.py clip_near / clip_far), applied by ra_render_volume_chunk */
    int   only_visibility;                    /* cfg.only_visibility (sphere_tracing_renderer.py:516-519, 720-723; debugging option): the cosine
                                                 of every light is 1 and the probe's radiance the mean of its channels — in the shading of
                                                 ra_render_sphere_chunk and ra_render_ground_chunk (the three channels of `shade` are then equal:
                                                 the reference's map has one) */
    int   vis_shade_map;                      /* what the `shade` output of ra_render_sphere_chunk / ra_render_ground_chunk holds: 0 the shading
                                                 (:749-751), 1 the mean light visibility (cfg.vis_lvis_map, :537, :756), 2 the mean cosine
                                                 (cfg.vis_ldot_map, :538, :757; the reference applies it after vis_lvis_map, so it wins) */
    int   use_geodesic_filter;                /* 1 (default, cfg.use_geodesic_filter): geodesic_knn (sample_utils.py:103-162) — per-neighbour
                                                 signed distances, neighbours farther than dist_th from the closest one ON THE CANONICAL BODY
                                                 replaced by it; 0: knn_with_filter (:164-194) — distance sqrt(mean d^2) with the sign of
                                                 max_k sign((x - v_k) . n_k), the three neighbours as found */
    float key_light_share;                    /* 0.0078 (default: four times the mean share of 512 lights); with trace_precision 1: the
                                                 light-visibility rays towards the frame's KEY LIGHTS are traced in compensated arithmetic like the
                                                 surface trace.  A light is a key light when it holds at least this fraction of a probe's power
                                                 (radiance x solid angle) — and at least 4 / L — under any of the frame's probes; the 48 lights with
                                                 the largest share at most, which bounds the tier's cost at ~10 % of the shadow rays.  A DFSS penumbra value is d * sharp / (2 t) (sphere_tracing_renderer.py:157-179): it
                                                 amplifies the 5e-5 distance error of plain f16 operands up to 500 x per light.  Summed over 512 lights
                                                 of comparable power the errors average out; under a key light that holds most of the power they do
                                                 not (the reference-made hard cases of tests/golden/switches.npz: max |err| 1.2e-2 .. 4.4e-2).  The
                                                 key lights are 0-3 % of the lights (a sun, a window; none under an overcast sky).  0: no key-light tier (round 5's behaviour) */
} ra_config;
/* A zero-initialised ra_config is NOT the default configuration (trace_precision 0 = plain operands, clip_far 0, ...): start from
 * ra_default_config() — the values documented above — and override.  ra_set_config rejects trace_precision outside 0..2,
 * clip_far <= clip_near (or NaN), vis_shade_map outside 0..2 and a negative key_light_share. */
int ra_default_config(ra_config* out);
int ra_set_config(ra_ctx* ctx, const ra_config* cfg);

/* ---- weights: one call per state_dict entry (SURVEY.md section 8b "weights on disk") ------
 * name is the reference's state_dict key, data a HOST fp32 array of `numel` elements in
 * torch's row-major layout.  ra_finalize_weights folds weight_norm (W = g*v/|v|, net_utils.py:
 * 1326-1327), folds 1/sqrt(2) of the SDF skip (net_utils.py:1345-1346), pads to MFMA tiles,
 * converts to bf16 fragment order and uploads.  Replaces load_network()+nn.Module parameters
 * (lib/utils/net_utils.py:1514-1584). */
int ra_set_weight(ra_ctx* ctx, const char* name, const float* host_data, size_t numel);
int ra_finalize_weights(ra_ctx* ctx, void* stream);
/* 1 when the cooperative 4-wave distance kernel for launches of <= 8 Ki points (K3CC, csrc/ra_k3cc.hpp) passed its self-test against the
 * plain compensated kernel on this device at ra_finalize_weights (bit for bit; tested once per process and device) and is in use; 0: the
 * context launches K3C's 4-wave tiles instead (slower small launches, same results) — or has no weights yet. */
int ra_k3cc_enabled(const ra_ctx* ctx);

/* ---- per-frame SMPL state: the batch keys world_to_bigpose consumes
 * (lib/networks/deform/base_network.py:238-336; schema lib/datasets/base_dataset.py:337-397).
 * All dev pointers.  pverts, weights, A, big_A, poses and cond_fix are consumed by ra_set_frame (async on stream: vertex blend,
 * BVH build, bias folds); R, Th, pnorm and tverts are read IN PLACE by every later query of the frame, so the caller keeps them
 * alive and unchanged until the next ra_set_frame (the Python binding holds references).  cond_fix = train_motion.poses[:,
 * fix_material] (base_network.py:501-503), may be NULL for the relight network. */
typedef struct ra_frame {
    const float* R;        /* 3x3   */
    const float* Th;       /* 3     */
    const float* poses;    /* n_bones*3 (cond)            */
    const float* cond_fix; /* n_bones*3 or NULL            */
    const float* A;        /* n_bones x 4 x 4             */
    const float* big_A;    /* n_bones x 4 x 4             */
    const float* pverts;   /* n_verts x 3                 */
    const float* pnorm;    /* n_verts x 3                 */
    const float* tverts;   /* n_verts x 3                 */
    const float* weights;  /* n_verts x n_bones           */
    int n_verts;
} ra_frame;
int ra_set_frame(ra_ctx* ctx, const ra_frame* frame, void* stream);

/* ---- operators -------------------------------------------------------------------------- */
/* Network.inference_world_distance_field (base_network.py:365-387): hierarchical distance
 * query. x: n x 3 world points -> sdf: n. */
int ra_hdq_sdf(ra_ctx* ctx, const float* x_dev, int n, float dist_th, int smooth_transition,
               float* sdf_dev, void* stream);

/* Network.inference_observed_distance_field with filtering=False (base_network.py:389-449): x are big-pose points,
 * sdf = SDF(x + resd(x, pose)) -> sdf: n.  Runs the production distance-query kernel (K3) without the coarse level.  The
 * filtered variant is the hierarchical query above on a frame whose posed body IS the template (pverts = tverts, A = I). */
int ra_observed_sdf(ra_ctx* ctx, const float* bpts_dev, int n, float* sdf_dev, void* stream);

/* Network.world_to_bigpose_transform / bigpose_to_world_transform (base_network.py:338-363): per point the 4x4
 * w2b = big_A_bw @ affine_inverse(A_bw) @ affine_inverse([R | Th]) with the blended bone transforms of the point's 3 nearest
 * vertices of the ctx's CURRENT frame (no distance filtering); invert != 0 returns affine_inverse(w2b) instead.  R (9) and
 * Th (3) are device pointers to the world <- pose transform used in the composition: the backward variant searches the
 * template (caller sets a frame with pverts = tverts, R = I, Th = 0) but composes with the real frame's R, Th.
 * affine_inverse transposes the 3x3 block (blend_utils.py:11-15) also for blended, non-rigid matrices, as the reference does.
 * out: n x 16 row-major. */
int ra_bigpose_transform(ra_ctx* ctx, const float* x_dev, int n, const float* R_dev, const float* Th_dev, int invert,
                         float* out_dev, void* stream);

/* Network.forward in eval mode (relight_network.py:91-104 / base_network.py:496-515).
 * x, v: n x 3 (v may be NULL for the relight network); raw: n x ra_raw_channels(), zeros for
 * points farther than dist_th from the body.  Channels: relight [cpts3,bpts3,resd3,albedo3,
 * roughness1,norm3,occ1] = 17; AniSDF [cpts3,bpts3,resd3,norm3,rgb3,occ1] = 16. */
int ra_raw_channels(const ra_ctx* ctx);
int ra_forward(ra_ctx* ctx, const float* x_dev, const float* v_dev, int n, float dist_th,
               float* raw_dev, void* stream);

/* sphere_tracing (sphere_tracing_renderer.py:20-216, mode 'hdq') over n rays.
 * tan_i_dev: per-ray sharpness (soft shadow) or NULL -> scalar tan_i.  Outputs may be NULL. */
typedef struct ra_trace_params {
    int   iters;            /* 16 surface / 4 shadow                                   */
    float tan_i;            /* cfg.sphere_tracing.tan_i = 1000 (hard)                  */
    float tan_i_multiplier; /* 1                                                       */
    float relax, offset, eps;
    int   shadow_skip_iter; /* 1                                                       */
    int   clay_book;        /* !cfg.no_claybook                                        */
    int   soft_shadow;
    float dist_th;          /* HDQ threshold forwarded to the distance query           */
} ra_trace_params;
int ra_sphere_trace(ra_ctx* ctx, const float* ray_o, const float* ray_d, const float* near_,
                    const float* far_, const float* tan_i_dev, int n, const ra_trace_params* p,
                    float* surf, float* occ, float* st, float* ot, void* stream);

/* ---- renderers: one chunk of rays (chunkify, net_utils.py:291-359) ------------------------ */
typedef struct ra_render_out { /* all dev, all optional (NULL = not wanted); P rays        */
    float* rgb;        /* P x 3                                                         */
    float* acc;        /* P                                                             */
    float* depth;      /* P                                                             */
    float* surf;       /* P x 3                                                         */
    float* norm;       /* P x 3                                                         */
    float* albedo;     /* P x 3   (relight)                                             */
    float* roughness;  /* P       (relight)                                             */
    float* shade;      /* P x 3   (relight)                                             */
    float* spec;       /* P x 3   (relight, cfg.vis_specular_map)                        */
    float* cpts;       /* P x 3                                                         */
    float* bpts;       /* P x 3                                                         */
    float* resd;       /* P x 3                                                         */
    float* ray_o;      /* P x 3   origins of hit rays, zeros elsewhere                  */
    float* lvis;       /* P x 512 (cfg.vis_novel_light)                                 */
    float* ldot;       /* P x 512 (cfg.vis_novel_light)                                 */
    /* render_human's per-hit leftovers (sphere_tracing_renderer.py:616-650), as full-ray maps (zeros on misses, NOT premultiplied);
     * the caller compacts them to the hit rays */
    float* raw;               /* P x (n_samples * C): the network's raw channels of the n_samples surface samples (C = ra_raw_channels) */
    float* volume_albedo;     /* P x 3   composited albedo, clipped, before cfg.albedo_multiplier (relight)                 */
    float* volume_roughness;  /* P       composited roughness, clipped (relight)                                            */
} ra_render_out;

typedef struct ra_sphere_params {
    ra_trace_params surface;   /* cfg.sphere_tracing                                     */
    ra_trace_params shadow;    /* cfg.obj_lvis (iter 4, offset .01, dist_th .125)         */
    float shadow_near_offset;  /* cfg.obj_lvis.near_offset = 0.02                        */
    float dist_th;             /* cfg.dist_th for the material query                     */
    float surf_sample_range;   /* 0.005                                                  */
    int   n_samples;           /* 3                                                      */
    int   relighting;          /* cfg.relighting                                         */
    int   no_visibility, local_visibility;
    int   premultiply;         /* alpha_output_ (sphere_tracing_renderer.py:454-460,1113) */
    /* Several of the reference's render chunks in ONE call (the reference's chunks bound ITS memory; rays are independent): ray r of this
     * call belongs to chunk j with box_start[j] <= r < box_start[j + 1] and its shadow rays are clipped against boxes[6 j .. 6 j + 5] — the
     * box the reference's in-place growth (:1020-1022) had reached at that chunk, computed by the caller with the same float arithmetic.
     * Nothing else of render_human depends on the box, so the pixels are those of chunk-by-chunk rendering, bit for bit, and a frame of
     * several chunks runs ONE 16-iteration surface loop instead of one per chunk.  n_boxes <= 1: every ray uses `bbox`.  At most 32 boxes;
     * box_start[0] = 0, box_start[n_boxes] = P, ascending (host arrays). */
    int   n_boxes;
    const float* boxes;
    const int*   box_start;
} ra_sphere_params;

/* sphere_tracing_renderer.Renderer.get_pixel_value -> render_human (:551-784, :981-1039) for one
 * chunk.  bbox: 6 floats (min xyz, max xyz) = batch.wbounds AFTER the caller applied the
 * per-chunk margin growth (quirk: :1020-1022).  probe: env_h2 x env_w2 x 3 linear radiance
 * (the learned 32x64 map or a novel 16x32 probe); light_xyz/area/sharp: 512 lights. */
int ra_render_sphere_chunk(ra_ctx* ctx, const float* ray_o, const float* ray_d, const float* near_,
                           const float* far_, int P, const float* bbox_host6,
                           const float* probe_dev, int probe_h, int probe_w,
                           const ra_sphere_params* p, const ra_render_out* out, void* stream);

/* One rank's rays out of the frame's (pixels dealt in 8 x 8 tiles): out_*[i] = *[idx[i]] for the four per-ray arrays of a
 * batch (ray_o / ray_d: 3 floats per ray; near / far: 1), idx: n int64 ray indices (device).  No context: any device, any time.
 * Replaces the four index_select launches of the host framework in the per-frame path of a sharded job. */
int ra_gather_rays(int device, const long long* idx_dev, int n, const float* ray_o, const float* ray_d, const float* near_, const float* far_,
                   float* out_o, float* out_d, float* out_near, float* out_far, void* stream);

/* ... and the un-interleave after the frame all_gather: dst[dst_idx[i]] = src[src_idx[i]] for n rows of C floats (rank r, slot j -> the
 * j-th pixel owned by r; the index vectors are the shard plan's, ra_shard_plan). */
int ra_scatter_rows(int device, const float* src_dev, const long long* src_idx_dev, const long long* dst_idx_dev, long long n, int C,
                    float* dst_dev, void* stream);

/* Marks the start of one top-level render (Renderer.render: every chunk call of one frame follows).  The library numbers a frame's render
 * calls from ra_set_frame to match each with the counts the same call found in an earlier frame (launch-variant hints: a pure speed aid);
 * a caller that renders the SAME frame state again and again without ra_set_frame (a cached frame, a turntable of cameras) calls this
 * instead, or its calls run out of numbered slots after 64 and lose their hints.  Optional; never changes results. */
int ra_begin_render(ra_ctx* ctx);

/* The key lights of the current frame (ra_config.key_light_share), named by the caller: n probes of probe_h x probe_w x 3 (device) — every
 * probe the frame's cached visibility will be shaded with.  ra_render_sphere_chunk / ra_render_ground_chunk derive the key lights from the
 * probe they shade with; a renderer that traces once and re-shades under OTHER probes afterwards (novel_light_sphere_tracing.py:163-213:
 * ra_reshade, ra_reshade_ground) calls this before the frame's render calls, once per probe size (accumulate = 1 adds to the flags of the
 * call before), and with n = 0 after them (back to per-call key lights).  No counterpart in the reference, whose arithmetic is fp32 throughout. */
int ra_set_key_probes(ra_ctx* ctx, const float* probes_dev, int n, int probe_h, int probe_w, int accumulate, void* stream);

/* The positions of the ctx's lights, moved by the caller: the reference's relight network returns light_xyz_ + randn * cfg.light_xyz_noise_std
 * in training mode (relight_network.py:79-84; one draw per render call, sphere_tracing_renderer.py:1029), and that draw feeds the
 * shadow-ray directions (normalize(xyz), :285), the cosine (:292) and surf2light of the probe lookup and the BRDF (:715-728).
 * xyz_dev: n_lights x 3 fp32 (device); NULL restores the loaded light_xyz_.  Stream-ordered: the positions are copied into the ctx's own
 * buffer on `stream` and the unit directions recomputed behind the copy; the caller's buffer is read on the stream and never kept.
 * light_area and light_sharp do not move (the reference jitters positions only).  From here on EVERY consumer of the ctx follows the new
 * positions until they are set again: the visibility stage of ra_render_sphere_chunk / ra_render_ground_chunk and ra_light_visibility,
 * the key-light derivation, ra_reshade, ra_reshade_backward, ra_reshade_ground, ra_debug_lvis.  Key-light flags named through
 * ra_set_key_probes were derived from the old directions: the call DROPS them, exactly as ra_set_key_probes(n = 0) does (name them again
 * after the move if the frame needs them).  ra_finalize_weights restores the loaded positions.  Errors: a ctx without finalised relight
 * weights, or without a light set. */
int ra_set_light_xyz(ra_ctx* ctx, const float* xyz_dev, void* stream);

/* light_visibility (sphere_tracing_renderer.py:265-344) for given surface points of the CURRENT frame, exactly as ra_render_sphere_chunk
 * runs it (the same stage, fed the caller's list of points instead of a chunk's hit slots), under the ctx's current light positions
 * (ra_set_light_xyz).  surf, norm: n x 3; acc: n — e.g. a rendered frame's surf / norm / acc maps; bbox_host6: the shadow rays' box
 * (batch.wbounds as the frame's render left it).  Of `params` it reads shadow, shadow_near_offset, no_visibility and local_visibility
 * and nothing else.  rows_dev: NULL -> all n points, outputs n x n_lights; else n_rows DISTINCT int32 indices into the n points in any
 * order: only those are traced and the outputs are compact n_rows x n_lights, row k belonging to point rows_dev[k] (bit-identical to
 * that row of the full call).  probe_dev (probe_h x probe_w x 3): the key lights (ra_config.key_light_share) are derived from it, as
 * ra_render_sphere_chunk derives them from the probe it shades with; NULL: every ray runs in the plain tier, unless ra_set_key_probes
 * named the key lights.  lvis, ldot: pixel-major, the layout ra_reshade reads.  Asynchronous on stream; n == 0 or n_rows == 0 returns 0
 * and writes nothing.  The call takes no launch-variant hint slot and does not renumber the render calls' hints: a render after it runs
 * the kernels it would have run.  With a gate (ra_set_gate) it takes its turn like the stage inside a render call. */
int ra_light_visibility(ra_ctx* ctx, const float* surf, const float* norm, const float* acc, int n, const int* rows_dev, int n_rows,
                        const float* bbox_host6, const float* probe_dev, int probe_h, int probe_w, const ra_sphere_params* params,
                        float* lvis, float* ldot, void* stream);

/* base_renderer.Renderer.get_pixel_value (base_renderer.py:53-113): uniform samples,
 * Network.forward per sample, alpha compositing.  near / far as the dataset delivers them: the renderer's clip
 * (base_renderer.py:120-121) is applied here (ra_config.clip_near / clip_far).  Every array of `out` is written for every ray. */
int ra_render_volume_chunk(ra_ctx* ctx, const float* ray_o, const float* ray_d, const float* near_,
                           const float* far_, int P, int n_samples, float dist_th,
                           const ra_render_out* out, void* stream);

/* novel_light_sphere_tracing.render_human (:21-66): re-shade cached maps under n_probes probes
 * in one pass.  probes: n_probes x h x w x 3. Outputs n_probes x P x 3 each (may be NULL). */
int ra_reshade(ra_ctx* ctx, const float* ray_o, const float* surf, const float* norm,
               const float* albedo, const float* roughness, const float* lvis, const float* ldot,
               int P, const float* probes_dev, int n_probes, int probe_h, int probe_w,
               float* rgb, float* shade, float* spec, void* stream);

/* Backward of ra_reshade with respect to albedo, roughness and the probes — the relighting stage's gradient (relight_trainer.py:113-118:
 * geometry frozen, light visibility under no_grad, the image loss reaches the shading sum only).  d_rgb: n_probes x P x 3, the gradient
 * with respect to the tone-mapped rgb that ra_reshade returns.  d_albedo: P x 3, summed over the probes (the Lambert term; exactly 0
 * under glossy_only).  d_roughness: P, summed over probes and channels (through rough^4 in D and G; exactly 0 under lambert_only).
 * d_probes: n_probes x probe_h x probe_w x 3 (the bilinear taps of the probe lookup, transposed, summed over pixels and lights).
 * Conventions are torch autograd's on render_human (:21-66): the sRGB clip passes gradient for 0 <= lin <= 1 only, an operand that
 * safe_divide clamps gets none, chi factors and the clips of l.n / v.n are constants; surf, norm, ray_o, lvis and ldot are constants
 * (ldot is not read: cancel_cosine).  lambert_only / glossy_only come from the ctx config.  Any output may be NULL; outputs are
 * overwritten, not accumulated into.  P == 0 or n_probes == 0 returns 0 and writes nothing.  A probe must fit the kernel's LDS tile:
 * probe_h * probe_w <= 5461 (16 x 32 and 32 x 64 do).  Asynchronous on stream; allocates ctx scratch on the first call of a size only.
 * Every output is bit-identical from run to run, and a probe's gradient does not depend on which other probes share the call. */
int ra_reshade_backward(ra_ctx* ctx, const float* ray_o, const float* surf, const float* norm,
                        const float* albedo, const float* roughness, const float* lvis, const float* ldot, int P,
                        const float* probes_dev, int n_probes, int probe_h, int probe_w,
                        const float* d_rgb, float* d_albedo, float* d_roughness, float* d_probes, void* stream);

/* The material heads of the relighting stage on cached surface features: forward and weight gradient (relight_network.py:45-47,91-104:
 * albedo_network 256 -> 128 -> 128 -> 3, roughness_network 256 -> 128 -> 128 -> 1, Softplus(beta = 100), output slope * sigmoid + bias with
 * the slopes and biases of the ctx config).  With ra_reshade_backward this closes the chain photograph -> d_albedo / d_roughness -> head
 * weights on the device (relight_trainer.py:113-118 trains exactly these two networks and the probe; geometry is frozen).
 *
 * Parameters are ONE flat fp32 device vector theta of ra_heads_param_count() = 99 332 floats in torch's own row-major layout:
 *   albedo_network.linears.0.weight (128 x 256), .0.bias (128), .1.weight (128 x 128), .1.bias (128), .2.weight (3 x 128), .2.bias (3),
 *   then roughness_network likewise with .2.weight (1 x 128), .2.bias (1).
 * d_theta has the same layout.  Width 128 and depth 2 are compiled in.  Writing fitted weights back needs no call of its own: download
 * theta, split it into the twelve state_dict keys, ra_set_weight them and ra_finalize_weights again.
 *
 * The kernels always use f16 operands with fp32 accumulation, whatever ra_config.mlp_f16 says (bf16 operands leave the weight gradient
 * 7-13 x noisier).  The deltas of the backward pass are normalised per call and per head by a power of two found on the device and
 * unscaled in fp32: the result is linear in the incoming gradient down to gradients of 1e-12 and below.
 *
 * ra_heads_get_params: the heads as loaded by ra_set_weight, in the flat layout (a set-up call: it waits for its copy on stream).
 * ra_heads_forward:    feat (n x 256) -> albedo (n x 3), roughness (n); either output may be NULL.
 * ra_heads_backward:   d_albedo (n x 3), d_roughness (n) -> d_theta.  Either gradient may be NULL: its head's slice of d_theta is written
 *                      as zeros, and the other head's slice is bit-identical to what it is with both given.  The forward is recomputed.
 * ra_bigpose_features: the K4 forward on big-pose points of the CURRENT frame (channels 3:6 of ra_render_out.raw), returning the 256
 *                      features as the heads see them inside the renderer (f16 values); bit-identical to ra_debug_mlp's feat.
 *
 * Asynchronous on stream; outputs are overwritten; n == 0 returns 0 and writes nothing; a null required input is the error "null input",
 * a ctx that is not a relight ctx with weights the error "relight ctx".  Scratch is allocated on the first call of a size only.  No float
 * atomics: partial sums go to one slab per workgroup and are added in slab order, the grid depends on n alone, two identical calls are
 * bit-identical. */
size_t ra_heads_param_count(const ra_ctx* ctx);
int ra_heads_get_params(ra_ctx* ctx, float* theta_dev, void* stream);
int ra_heads_forward(ra_ctx* ctx, const float* theta_dev, const float* feat_dev, int n, float* albedo_dev, float* rough_dev, void* stream);
int ra_heads_backward(ra_ctx* ctx, const float* theta_dev, const float* feat_dev, int n,
                      const float* d_albedo_dev, const float* d_rough_dev, float* d_theta_dev, void* stream);
int ra_bigpose_features(ra_ctx* ctx, const float* bpts_dev, int n, float* feat_dev, void* stream);

/* The regularisers of the relighting stage (relight_trainer.py:70-91): what its optimisation adds to the image loss.
 *
 * ra_canonical_features: the 256 features of the signed-distance network on CANONICAL points (n x 3), the input of the jitter outputs
 *   albedo_jitter / roughness_jitter = heads(signed_distance_network.feat(cpts + noise)) (relight_network.py:107-118).  No residual
 *   deformation in front and no pose condition: it needs the weights of a relight ctx and NO frame.  feat (n x 256) has the format of
 *   ra_bigpose_features — the values the heads read, rounded to the ctx's operand type (ra_config.mlp_f16), stored as fp32 — and for
 *   cpts = channels 0:3 of ra_render_out.raw (the full query's own fp32 bpts + resd) it equals ra_bigpose_features(bpts) bit for bit.
 *   feat_dev may point into a larger buffer (the second half of a 2n x 256 buffer whose first half holds cached features: one
 *   ra_heads_forward / ra_heads_backward call then covers both).
 *
 * ra_gaussian_entropy: gaussian_entropy (loss_utils.py:51-76) of x (n x 3, e.g. albedo) and its gradient under torch autograd's
 *   conventions.  15 bins on [0, 1] (the reference's defaults, the only ones its trainer uses) are compiled in.  Per channel:
 *   m = mean, s = unbiased VARIANCE (the reference uses it as the kernel width; kept), k_nb = exp(-0.5 ((x_n - mu_b) / s)^2) /
 *   (s sqrt(2 pi)) / 15 with mu_b = (b + 0.5) / 15, h_b = sum_n k_nb, S = sum_b h_b, p_b = h_b / S + 1e-6, E = -sum_c sum_b p_b log p_b.
 *   value: one device float.  d_x (n x 3, may be NULL): dE/dx times *d_value_dev, including the path through s = var(x); d_value_dev
 *   may be NULL, which means 1.  The product with *d_value_dev is the last fp32 operation: scaling it by a power of two scales d_x bit
 *   for bit.  x is read and d_x written in fp32, the arithmetic between is double.
 *   Deviations from the reference, deliberate:
 *     - a channel with S <= 1e-6, with s == 0 or with a non-finite s contributes 0 to the value and EXACTLY 0 to d_x.  The reference
 *       takes its ones_like branch for the value there (also 0), but its autograd returns NaN gradients for a constant channel;
 *     - n < 2 is the error "bad sizes" (the reference's variance is NaN there).
 *   Any ctx will do (no weights are read); it provides the scratch.
 *
 * Both are asynchronous on stream and overwrite their outputs; a null required pointer is the error "null input";
 * ra_canonical_features returns 0 for n == 0 and gives the error "relight ctx" for a ctx that is not a relight ctx with weights.
 * Scratch is allocated on the first call of a size only.  No float atomics: partial sums go to one slab per workgroup and are added
 * in slab order, the grids depend on n alone, two identical calls are bit-identical. */
int ra_canonical_features(ra_ctx* ctx, const float* cpts_dev, int n, float* feat_dev, void* stream);
int ra_gaussian_entropy(ra_ctx* ctx, const float* x_dev, int n, const float* d_value_dev, float* value_dev, float* d_x_dev, void* stream);

/* novel_light_sphere_tracing.render_ground (:70-99): re-shade the ground layer of the main pass under n_probes probes from its
 * cached per-light visibility and cosine (ra_ground_out.lvis / .ldot of ALL frame pixels, P x 512 each): Lambert ground,
 * rgb = linear2srgb(albedo / pi * sum_l lvis ldot area L_probe(l)), shade = sum / pi, spec = shade / 20 (no shading_albedo, no
 * ground_shading_multiplier here).  albedo: attach_envmap != 0 -> the probe's image (images: n_probes x ih x iw x 3, or NULL ->
 * the probe itself) sampled along ray_d (:79-83), else albedo_map (P x 3).  Outputs n_probes x P x 3 each, any may be NULL. */
int ra_reshade_ground(ra_ctx* ctx, const float* ray_d, const float* albedo_map, const float* lvis, const float* ldot, int P,
                      const float* probes_dev, int n_probes, int probe_h, int probe_w, const float* images_dev, int image_h, int image_w,
                      int attach_envmap, float* rgb, float* albedo, float* shade, float* spec, void* stream);

/* ---- measurement ------------------------------------------------------------------------- */
typedef struct ra_counters {       /* cumulative since ra_reset_counters; read with a sync  */
    uint64_t n_coarse;             /* 3-NN queries (K1)                                       */
    uint64_t n_fine_sdf;           /* resd+SDF forward, sdf only  (F_sdf  = 1 901 568 FLOP)   */
    uint64_t n_fine_full;          /* resd+SDF forward+tangents+heads (geometry points)       */
    uint64_t n_shadow_rays;
    uint64_t n_hit_pixels;
    uint64_t n_shaded;             /* pixel x probe shading evaluations                       */
    uint64_t n_fine_sdf_wide;      /* the part of n_fine_sdf computed by the 8-wave distance kernel (launches that fill the chip) */
    uint64_t n_fine_sdf_comp;      /* the part of n_fine_sdf computed in compensated arithmetic (ra_config.trace_precision): 3 x F_sdf executed */
} ra_counters;
int ra_get_counters(ra_ctx* ctx, ra_counters* out, void* stream); /* synchronises stream */
int ra_reset_counters(ra_ctx* ctx, void* stream);

/* time (ms) spent in the fused MLP kernel launches since the last reset, measured with HIP
 * events on `stream`; n_launches receives the launch count.  Synchronises. */
int ra_get_mlp_time(ra_ctx* ctx, float* ms, int* n_launches, void* stream);
/* the same for one kernel family: kind 0 = fused distance query (K3, every width), 1 = full query with normals / material / colour (K4),
 * 2 = the 8-wave distance query only (the launches that fill the chip: the frame's dominant kernel), 3 = the 2- / 4-wave distance query,
 * 4 = the compensated distance query (K3C and its cooperative small-launch variant K3CC; not part of kind 0) */
int ra_get_kernel_time(ra_ctx* ctx, int kind, float* ms, int* n_launches, void* stream);
int ra_enable_timing(ra_ctx* ctx, int on);
/* ---- frames in flight --------------------------------------------------------------------------------------------
 * Throughput aid with no counterpart in the reference (its frame loop is sequential: lib/evaluators, run.py).  Several contexts on
 * several HIP streams render DIFFERENT frames at once; contexts that share a gate run their light-visibility stages (the frame's
 * large distance-query launches, sphere_tracing_renderer.py:265-344) one after the other in submission order, while everything
 * else of the next frame (pose, box structure, the 16 latency-bound surface-tracing iterations, normals, shading) runs beside the
 * previous frame's stage.  Frames are bit-identical with and without.  A gate is used from ONE host thread; it must outlive the
 * contexts attached to it (detach with gate = NULL). */
typedef struct ra_gate ra_gate;
int ra_gate_create(ra_gate** out, int device);
int ra_gate_destroy(ra_gate* gate);
int ra_set_gate(ra_ctx* ctx, ra_gate* gate);

/* ---- multi-GPU: the deal of a frame's in-box rays to the ranks of one node (no counterpart in the reference,
 * whose inference is single-process) ----------------------------------------------------------------------------------------------
 * HOST function, no device work, no ctx: relightableavatar_amd/shard.py make_plan's per-frame part in one pass over the mask.
 * mask: H x W bytes (batch.mask_at_box, row-major, non-zero = in box); P = number of in-box rays (= set bytes, checked); the in-box rays
 * are the mask's pixels in row-major order (lib/utils/data_utils.py:925-938).  Pixels are dealt in 8 x 8 tiles: ground = 0 -> the tiles
 * that hold in-box pixels round robin in raster order; ground != 0 -> fixed diagonal stripes (tile_y + tile_x) % world over the whole
 * frame (the sharded ground-plane pass needs a rank's in-box pixels to be a subset of its frame pixels).
 * Outputs (host, caller-allocated, e.g. inside one pinned staging block): owner[P] (nullable) rank of every ray; counts[world];
 * *n_max = max(counts); order[P] = rays grouped by owner, ascending inside (rank r's shard is order[offs[r] : offs[r + 1]]);
 * src[P]: item j of `order` is row src[j] = rank * n_max + position of the all_gather's (world * n_max)-row output, i.e.
 * full[order] = gathered[src]; inds[P] (nullable; needs ground_pos[H * W] = position of every frame pixel in its owner's full-frame
 * pixel list): ground_pos of the rays in `order` order.  edges[n_edges] (nullable): ascending ray indices (chunk boundaries of the
 * unsharded ray list, chunkify's rule net_utils.py:323); chunk_pos[r * n_edges + e] = how many of rank r's rays lie before ray
 * edges[e].  world <= 256. */
int ra_shard_plan(const unsigned char* mask, int H, int W, int world, int ground, long long P, const long long* ground_pos,
                  const long long* edges, int n_edges, unsigned char* owner, long long* order, long long* src, long long* inds,
                  long long* counts, long long* chunk_pos, long long* n_max);

/* 1 (default): exact 3-NN through the per-frame vertex BVH; 0: brute force over all vertices (validation path).
 * Takes effect at the next ra_set_frame. Both return identical neighbours. */
int ra_set_knn_mode(ra_ctx* ctx, int use_bvh);

/* ---- N1: ground-plane pass --------------------------------------------------------------------
 * replaces render_ground (lib/networks/renderer/sphere_tracing_renderer.py:463-548) for one chunk of full-frame rays:
 * ray/plane hit (moller_trumbore on one triangle of the plane, mesh_utils.py:710-738), DFSS shadows of the avatar onto
 * the plane (light_visibility :265-344 with cfg.env_lvis), Lambert ground lit by the probe, distance fade (:497-505). */
typedef struct ra_ground_params {
    float normal[3];            /* cfg.ground_normal (normalised inside) */
    float origin[3];            /* cfg.ground_origin */
    float albedo[3];            /* cfg.ground_albedo, used when attach_envmap == 0 */
    int attach_envmap;          /* cfg.ground_attach_envmap: albedo = probe sampled along the view ray */
    float env_r;                /* cfg.env_r */
    float shading_multiplier;   /* cfg.ground_shading_multiplier */
    ra_trace_params shadow;     /* cfg.env_lvis as a trace-parameter block */
    float shadow_near_offset;   /* cfg.env_lvis.near_offset */
    int no_visibility, local_visibility;
    /* Several of the reference's render chunks in ONE call (their launches merged; pixels identical): pixel r of the call belongs to chunk j
     * with box_start[j] <= r < box_start[j + 1] and its shadow rays are clipped against boxes[6 j .. 6 j + 5], the box the reference's
     * in-place growth (sphere_tracing_renderer.py:1054-1056) had reached at that chunk — computed by the caller, in the reference's float
     * arithmetic.  n_boxes = 0 or 1: the call is one chunk and uses the bbox argument.  At most 32 boxes per call. */
    int n_boxes;
    const float* boxes;         /* host, n_boxes x 6 */
    const int* box_start;       /* host, n_boxes + 1 ascending pixel indices, box_start[0] = 0, box_start[n_boxes] = P */
} ra_ground_params;

typedef struct ra_ground_out {  /* device buffers with P rows, any may be NULL */
    void* rgb;      /* (P,3) */
    void* surf;     /* (P,3) */
    void* albedo;   /* (P,3) */
    void* shade;    /* (P,3) shade_map (multiplier applied) */
    void* spec;     /* (P,3) spec_map = shade / 20 */
    void* depth;    /* (P)   t clipped to +-env_r */
    void* lvis;     /* (P,512) visibility after the distance fade (render_ground :505), cfg.vis_novel_light (:541-543) */
    void* ldot;     /* (P,512) ground normal . light direction, not clamped (:504) */
} ra_ground_out;

/* ray_o, ray_d: (P,3); acc: (P) = 1 - human acc (pixels with acc <= 0 are not traced and come back as zeros);
 * bbox: 6 host floats (the human box grown by the caller, get_ground_value :1054-1056); probe: (ph,pw,3) device. */
int ra_render_ground_chunk(ra_ctx* ctx, const float* ray_o, const float* ray_d, const float* acc, int P, const float* bbox,
                           const float* probe, int ph, int pw, const ra_ground_params* p, const ra_ground_out* out, void* stream);

/* blend_output_ / alpha_blend (sphere_tracing_renderer.py:396-451) for one map of C channels:
 *   dst[f] = ground[f] * acc[f]                      for all F full-frame pixels (ground == NULL: zeros, the acc_map case)
 *   dst[inds[j]] += human[j] * (1 - acc[inds[j]])    for the P in-box rays (human == NULL: skipped, the ground-only keys)
 * acc: (F) = 1 - human acc scattered to the frame; inds: (P) int64 frame index of every in-box ray. */
int ra_blend_ground(ra_ctx* ctx, const float* ground, const float* human, const long long* inds, const float* acc, int F, int P, int C,
                    float* dst, void* stream);

/* ---- N2: ray generation + bounding-box culling on the device ------------------------------------
 * replaces lib/utils/data_utils.py:827-845 (get_rays), :860-875 (get_full_near_far), :925-938 (get_rays_within_bounds),
 * called per frame by lib/datasets/pose_dataset.py:53-68 on the CPU.
 * K, R: 9 doubles row-major, T: 3 doubles (host); bounds: 6 floats (host: min xyz, max xyz = batch.wbounds).
 * Device outputs with capacity H*W rays: ray_o, ray_d (n,3) f32; near, far (n) f32 — the in-box rays in row-major
 * pixel order, exactly the reference's boolean-mask order; mask_at_box: H*W uint8.  *n_rays receives the count
 * (synchronises the stream); n_rays = NULL: no read-back, no synchronisation (the caller knows the count, e.g. H*W for an unbounded box).
 * bounds_dev (6 device floats, takes precedence over the host `bounds`, which may then be NULL): the box of a frame whose body state
 * is still being computed on the stream (ra_pose_frame's wbounds) — no host round trip between N3 and N2.  n_rays_dev (device int,
 * nullable) receives the count too: an animation loop copies it to pinned memory behind an event and reads it a pipeline turn later
 * (relightableavatar_amd/engine.py gen_rays_async), so generating the rays of frame f + 1 never waits for frame f.  Directions are computed in fp64 and rounded once (the reference computes them in the
 * camera's dtype and casts to float32); near/far follow the reference's float32 arithmetic operation by operation. */
int ra_gen_rays(ra_ctx* ctx, int H, int W, const double* K, const double* R, const double* T, const float* bounds, const float* bounds_dev,
                void* ray_o, void* ray_d, void* near, void* far, void* mask_at_box, int* n_rays, int* n_rays_dev, void* stream);

/* ---- N3: per-frame body state on the device -----------------------------------------------------
 * replaces lib/datasets/base_dataset.py:308-397 (get_lbs_params with cfg.use_geometry, get_blend), which runs on the CPU
 * per frame: bone transforms from the axis-angle poses (net_utils.py:1164-1183 / data_utils.py:1004-1069), template ->
 * T pose -> posed -> world vertices (blend_utils.py:212-218,264-313), vertex normals (pytorch3d Meshes.verts_normals),
 * bounds (data_utils.py:616-622).
 * Host inputs: poses, tjoints (J,3) f32, parents (J) int32 (topological order, parents[0] unused), big_A (J,16) f32,
 * Rh, Th (3) f32, faces (F,3) int32 (its vertex -> corner list is cached by content hash).
 * Device inputs: tverts (N,3), weights (N,J).  Device outputs (any may be NULL): A (J,16), joints (J,3), tpose (N,3),
 * pverts (N,3), wverts (N,3), pnorm (N,3), R (9), pbounds (6), wbounds (6).
 * ASYNCHRONOUS: the host inputs are copied into a pinned staging ring of the context before the call returns (the caller may reuse its
 * arrays at once), uploaded with one asynchronous copy, and the bone transforms (Rodrigues + the chain of 4 x 4 products, float64) run
 * on the device; nothing waits for the stream except the first call with a new `faces` array (its vertex -> corner list is built on the
 * host and uploaded synchronously, once per mesh). */
typedef struct ra_pose_in {
    const float *poses, *tjoints, *big_A, *Rh, *Th;
    const int* parents;
    const int* faces;
    int n_bones, n_faces, n_verts;
    const void *tverts, *weights;
    float bounds_padding;           /* get_bounds(padding=0.05) */
} ra_pose_in;
typedef struct ra_pose_out {
    void *A, *joints, *tpose, *pverts, *wverts, *pnorm, *R, *pbounds, *wbounds;
    void *poses, *Th;               /* device copies of the uploaded poses (J,3) and Th (3): the batch keys `poses` / `Th` without a second upload */
} ra_pose_out;
int ra_pose_frame(ra_ctx* ctx, const ra_pose_in* in, const ra_pose_out* out, void* stream);

/* The reference grows batch.wbounds IN PLACE by cfg.env_lvis.bbox_margin once per render chunk (sphere_tracing_renderer.py:1020-1022,
 * :1054-1056: bbox[:, 0] -= m; bbox[:, 1] += m).  wbounds: the batch's device tensor, 2 x 3 floats (min | max); one launch. */
int ra_grow_bounds(ra_ctx* ctx, float* wbounds_dev, float margin, void* stream);

/* ---- N4: environment-map rotation and the light-probe inset -------------------------------------
 * ra_shift_envmap: rotate_envmap's shift_image (lib/utils/relight_utils.py:69-85): out[y][x] = bilinear sample of img at
 * x + 0.5 + shift (wrapped modulo W; grid_sample align_corners=False, border padding), img/out: (H,W,C) device fp32.
 * ra_add_light_probe: add_light_probe (relight_utils.py:38-54 with gen_light_dir :9-35): overwrites the top-left uH x uW
 * pixels of rgb (H,W,3) with the probe seen along the camera's horizontal heading; cam_R: 9 host floats (world-to-camera). */
int ra_shift_envmap(ra_ctx* ctx, const float* img, int H, int W, int C, float shift, float* out, void* stream);
int ra_add_light_probe(ra_ctx* ctx, float* rgb, int H, int W, const float* probe, int ph, int pw, const float* cam_R, int uH, int uW,
                       void* stream);

/* ---- N4, third item: map -> image normalisations of the reference visualiser -------------------------------------
 * Visualizer.generate_image (lib/visualizers/base_visualizer.py:54-201) for one output type (lib/config/config.py:364-378): the
 * per-type normalisation of the rendered map, then the scatter of the P in-box rays into the H x W image over bg_brightness
 * (:188-195) and, if alpha != NULL, the alpha plane (:201-208; the caller concatenates it after the light-probe inset).
 *   SURFACE   a = cpts_map | surf_map (P,3): (a - tbounds[0]) / (tbounds[1] - tbounds[0]) * acc
 *   RESIDUAL  a = cpts_map, b = bpts_map:     acc * (a - b) / (the int(0.005 * 3P)-th largest value of a - b)
 *   DEPTH     a = depth_map (P):              clip((a - lo) / (hi - lo), 0, 1), lo / hi = the int(0.01 * P)-th smallest / largest
 *                                             depth among rays with acc != 0, lo clipped to min_clip (fewer such rays than the
 *                                             rank: the rank is clamped to their count, where the reference's topk raises)
 *   ALPHA     acc;   ROUGHNESS a (P);   RENDERING a (P,3);   ALBEDO a (P,3), linear2srgb if tonemap
 *   NORMAL    a = norm_map (P,3):             (normalize(a) @ cam_R^T, y and z flipped) * 0.5 + 0.5, times acc
 *   SHADING / SPECULAR a (P,3):               if normalize: a / (the int(0.005 * 3P)-th largest value)
 * pix: frame pixel of every ray (NULL: the maps are full-frame, P == H*W).  image: H*W x 3. */
enum { RA_IMG_SURFACE = 3, RA_IMG_RESIDUAL = 4, RA_IMG_DEPTH = 5, RA_IMG_ALPHA = 6, RA_IMG_NORMAL = 7, RA_IMG_SPECULAR = 8,
       RA_IMG_ALBEDO = 9, RA_IMG_ROUGHNESS = 10, RA_IMG_SHADING = 11, RA_IMG_RENDERING = 12 };      /* values of the Output enum */
typedef struct ra_image_params {
    int type, H, W;
    float bg_brightness;    /* cfg.bg_brightness */
    int normalize;          /* cfg.normalize_shading / cfg.normalize_specular */
    int tonemap;            /* cfg.tonemapping_albedo */
    float min_clip;         /* cfg.min_clip */
    float cam_R[9];         /* batch.cam_R (world -> camera), NORMAL */
    float tbounds[6];       /* batch.tbounds (big-pose box), SURFACE */
} ra_image_params;
int ra_map_to_image(ra_ctx* ctx, const ra_image_params* p, const float* a_dev, const float* b_dev, const float* acc_dev,
                    const long long* pix_dev, int P, float* image_dev, float* alpha_dev, void* stream);

/* ---- evaluation: the metrics of the reference's evaluator (lib/evaluators/base_evaluator.py) for one image pair --------------------
 * pred / gt: P x 3 fp32, either all H*W pixels of the image (pix NULL, P == H*W) or a ray list with pix[i] = the flat pixel index of
 * ray i (mask_at_box.nonzero()); a pixel no ray covers has bg_brightness in both images (:79-85).  The assembled images are never
 * built.  out (4 doubles on the device, 8-byte aligned; e.g. one row of an N x 4 table):
 *   out[0]  mse: the mean of (pred - gt)^2 over the H*W*3 values of the assembled images (cfg.eval_whole_img, the reference's default);
 *           with mse_over_rays over the P*3 ray values (eval_whole_img = False, :94; P == 0 gives NaN)
 *   out[1]  psnr = -10 log10(mse) (:26-29); +inf for mse == 0
 *   out[2]  ssim: skimage.metrics.structural_similarity(pred, gt, channel_axis=-1, data_range=data_range) at its defaults — 7 x 7
 *           uniform window, K1 = 0.01, K2 = 0.03, sample covariance, the mean over the windows that do not touch the border and
 *           over the 3 channels.  With crop_to_mask the images are first cropped to the bounding rectangle of the nonzero pixels of
 *           mask (H*W bytes; cv2.boundingRect, :32-39); crop_to_mask changes out[2] and out[3] only.  An image or rectangle narrower
 *           or lower than 7 (an empty mask too), where skimage raises: NaN
 *   out[3]  the number of windows averaged per channel (0 with the NaN)
 * Inputs are read as fp32, all arithmetic after them is double.  Asynchronous on stream, no read-back, no synchronisation; scratch is
 * allocated on the first call of a size only.  No float atomics: one partial per workgroup, added in index order, grids that depend
 * on H and W alone — two identical calls are bit-identical, a ray list gives the bits of its assembled image in any ray order, and
 * crop_to_mask gives the ssim bits of a call on the cropped arrays.
 * pix values are NOT validated: a value outside [0, H*W) drops that ray (its pixel keeps bg) without an error, and of two rays on one
 * pixel either may win.  Any ctx will do (no weights are read).
 * Errors: "null argument", "bad sizes" (H, W < 1, H*W >= 2^30, P < 0, P > H*W), "pixel indices" (P != H*W without pix), "mask"
 * (crop_to_mask without mask), "alignment" (out). */
typedef struct ra_metrics_params {
    int H, W;
    float bg_brightness;    /* cfg.bg_brightness */
    float data_range;       /* 1 in the reference */
    int mse_over_rays;
    int crop_to_mask;
} ra_metrics_params;
int ra_image_metrics(ra_ctx* ctx, const ra_metrics_params* p, const float* pred_dev, const float* gt_dev, const long long* pix_dev, int P,
                     const unsigned char* mask_dev, double* out_dev /* 4 */, void* stream);

/* ---- evaluation: LPIPS, the fourth metric of the reference's evaluator (lib/evaluators/base_evaluator.py:19-24, 50-69) ---------------
 * lpips.LPIPS() at its defaults — net 'alex', version '0.1', linear layers on, spatial = False, eval mode — on images in [0, 1] as the
 * evaluator passes them (no normalize=True: the network sees [0, 1], not [-1, 1]):
 *   x = (x - shift) / scale per channel; AlexNet's five convolutions (11/4/2 3->64, maxpool 3/2, 5/1/2 64->192, maxpool 3/2,
 *   3/1/1 192->384, 384->256, 256->256), a tap after every ReLU; per tap k, n = f / (sqrt(sum_c f^2) + 1e-10) for both images and
 *   r_k = mean over positions of sum_c lin_k[c] (n0 - n1)^2; lpips = r_0 + r_1 + r_2 + r_3 + r_4.
 * The pretrained weights are not part of this project: ra_lpips_load takes a user-supplied set (HOST pointers, fp32: conv_w[k] in
 * torch's (Cout, Cin, k, k) order, conv_b[k] (Cout), lin[k] (Cout, the bias-free 1 x 1 convolution), shift / scale), packs the
 * convolutions into the order the kernel reads and uploads them; a second call replaces the set behind the calls already queued.
 * ra_lpips_load synchronises the stream; ra_lpips_loaded returns 1 once a set is loaded (0 for a NULL ctx). */
typedef struct ra_lpips_weights {
    const float* conv_w[5];     /* (64,3,11,11) (192,64,5,5) (384,192,3,3) (256,384,3,3) (256,256,3,3) */
    const float* conv_b[5];
    const float* lin[5];        /* 64, 192, 384, 256, 256 */
    float shift[3], scale[3];   /* lpips: -0.030 -0.088 -0.188 / 0.458 0.448 0.450 */
} ra_lpips_weights;
int ra_lpips_load(ra_ctx* ctx, const ra_lpips_weights* w, void* stream);
int ra_lpips_loaded(ra_ctx* ctx);
/* pred / gt / pix / P / mask and p->H, W, bg_brightness, crop_to_mask as in ra_image_metrics (image assembly and the crop to
 * cv2.boundingRect(mask) are the ones of its SSIM); p->mse_over_rays and p->data_range are ignored.  out (6 doubles on the device,
 * 8-byte aligned): out[0] the value, out[1..5] the per-tap terms r_0..r_4.  An image or rectangle below 31 in either dimension (an empty
 * mask too), where torch raises in the second pool: six NaNs.
 * The convolutions run in fp32 (fp32-input MFMA: one k-ordered fmaf chain per output), everything after the fp32 features in double.
 * Asynchronous on stream, no read-back, no synchronisation, no float atomics; the host never learns the rectangle: every grid depends
 * on H and W alone, and scratch is allocated on the first call of a size only.  Two identical calls are bit-identical, (pred, gt) and
 * (gt, pred) agree bit for bit, identical images give six exact zeros, a ray list gives the bits of its assembled image in any ray
 * order, and crop_to_mask gives the bits of a call on the cropped arrays.
 * Errors: those of ra_image_metrics, and "lpips weights not loaded" (a NULL ctx holds none). */
int ra_lpips(ra_ctx* ctx, const ra_metrics_params* p, const float* pred_dev, const float* gt_dev, const long long* pix_dev, int P,
             const unsigned char* mask_dev, double* out_dev /* 6 */, void* stream);
/* stage hook for the parity tests: one image's (H*W x 3 fp32, H, W >= 31) post-ReLU activations of tap 0..4 in (C, h, w) order */
int ra_lpips_features(ra_ctx* ctx, const float* img_dev, int H, int W, int tap, float* out_dev, void* stream);
/* output pixels (of both images together) per workgroup tile of the convolutions: the tests take their edge sizes from it */
int ra_lpips_tile_m(void);

/* ---- evaluation: exact point-to-mesh distance, the primitive of the reference's mesh evaluator (lib/evaluators/mesh_evaluator.py) ----
 * and of its bvh_distance_queries / point_mesh_distance callers (base_network.py:417-427, sample_utils.py:681-724, mesh_utils.py:758-764).
 * ra_mesh_create builds a flat box structure over the triangles on the stream — box of the finite faces' centroids, 30-bit Morton
 * codes, one radix sort, leaves of ra_mesh_tile(0) face records that keep their original face id, leaf boxes, boxes of groups of
 * ra_mesh_tile(1) leaves — and reads nothing back.  verts: DEVICE, n_verts x 3 fp32.  faces: HOST, n_faces x 3 int32, checked against
 * [0, n_verts) before anything is launched; the mesh keeps its own copy of them and gathers the triangles into its own storage, so both
 * arrays are the caller's again once the stream has passed the call.  A face with a non-finite vertex is dropped on the device and is
 * never an answer.  The mesh belongs to the ctx: ra_mesh_destroy frees it (after a device synchronisation), ra_ctx_destroy frees those
 * still alive.  A mesh is immutable.  ra_mesh_create and ra_mesh_closest share scratch of the ctx (the sort's keys and the order of the
 * query points): the mesh calls of ONE ctx must be ordered with respect to each other — one stream, or streams the caller orders — as
 * the calls that share the ctx's other scratch must.
 * Errors: "null argument", "bad sizes" (n_verts < 1, n_faces < 1, n_faces > 2^24), "face index" (an index outside [0, n_verts)),
 * "not a mesh of this ctx". */
typedef struct ra_mesh ra_mesh;
enum { RA_MESH_BRUTE = 1,       /* scan every face, no pruning: the in-arithmetic reference of the sweep */
       RA_MESH_UNSORTED = 2 };  /* test and measurement hook: do not Morton-sort the query points internally (the same bits, slower) */
int ra_mesh_create(ra_ctx* ctx, const float* verts_dev, int n_verts, const int* faces_host, int n_faces, ra_mesh** out, void* stream);
int ra_mesh_destroy(ra_ctx* ctx, ra_mesh* mesh);
/* Per point (pts: DEVICE n x 3 fp32) the closest point of the mesh, in fp32: closest (n x 3), d2 (n) = the squared length of
 * p - closest as stored, face (n) = the ORIGINAL index of a face that attains d2, bary (n x 3) = the barycentrics of closest in that
 * face, in the face's vertex order.  Any output may be NULL, not all four; n == 0 launches nothing and reads no pointer.
 * Per triangle: Ericson's region method (Real-Time Collision Detection 5.1.5) with every product and sum a named fp32 operation and
 * every division guarded; a degenerate face acts as its segment or point.  Among faces of equal fp32 d2 the lowest original index wins.
 * The result is therefore a function of (point, mesh) alone: not of the leaf order, the pruning, the wave a point sits in, the order
 * of the points or the launch shape — the default call and RA_MESH_BRUTE agree bit for bit.  Pruning uses conservative box bounds only
 * and never discards a box whose bound equals a lane's best.
 * A point with a non-finite coordinate: d2 = closest = bary = NaN, face = -1.  A mesh whose every face was dropped: d2 = +inf,
 * face = -1, closest = bary = NaN for every finite point.
 * Asynchronous on stream, no read-back, no float atomics; scratch is allocated on the first call of a size only.
 * Errors: "null argument", "bad sizes" (n < 0, n >= 2^30), "unknown flag", "not a mesh of this ctx". */
int ra_mesh_closest(ra_ctx* ctx, const ra_mesh* mesh, const float* pts_dev, int n, int flags, float* d2_dev, float* closest_dev,
                    int* face_dev, float* bary_dev, void* stream);
/* test hook: 0 faces per leaf, 1 leaves per group, 2 points up to which a query is never sorted — the tests take their edge sizes from it */
int ra_mesh_tile(int which);
/* The backward of ra_mesh_closest in the points, the mesh's vertices and per-vertex attributes (the reference's grad_points / grad_tris
 * of point_face_dist_backward, lib/utils/sample_utils.py:198-307).  It needs no ra_mesh: it reads the forward's stored outputs and a
 * DEVICE copy of the faces (n_faces x 3 int32) of a mesh of n_verts vertices.
 * Per row i (ra_mesh_grad_rules.hpp, every operation a named fp32 operation): p = pts[i], q = closest[i], f = face[i], b = bary[i],
 * g = g_d2[i] the upstream gradient of d2 — the SQUARED distance —, ga = g_attr[i] (C values, 0 <= C <= 64) the upstream gradient of C
 * attribute channels interpolated at the closest point, sum_k b[k] attr[faces[f][k]].  With the face and the barycentrics held fixed
 * d(d2)/dp = 2 (p - q) and d(d2)/dv_k = -2 b[k] (p - q), in the face, edge and vertex regions alike.
 * A row is LIVE when 0 <= f < n_faces and the face's three indices lie in [0, n_verts), otherwise DEAD (a non-finite point of the
 * forward has face -1).
 *   live:  dpts[i][c] = (2 g) * (p[c] - q[c]), one subtraction and one product; slot (i, k), k = 0..2, belongs to vertex faces[f][k]
 *          and carries -(b[k] * dpts[i][c]) for dverts and b[k] * ga[ch] for dattr.
 *   dead:  dpts[i] = +0 and no slot.
 * Non-finite values of a live row are not filtered: they reach that row's dpts and its three vertices and nothing else.
 * dverts[v] and dattr[v] are the sums of v's slots in ascending 3 i + k, taken as the run sum of ra_texture_backward: lane l of a wave
 * adds terms l, l + 64, ... from +0 and the 64 lanes meet in the xor tree 32, 16, .., 1; a vertex without a slot gets +0.  The result
 * is a function of the inputs in their given order, bit for bit: not of the launch shape, and not of which outputs were asked for.
 * (The order of the rows IS the order of summation: permuting the rows keeps dpts' rows and may change dverts' last bits.)
 * Outputs: dpts (n x 3), dverts (n_verts x 3), dattr (n_verts x C); each may be NULL, not all three.  dpts and dverts need g_d2, dattr
 * needs g_attr.  n == 0 writes zeros to the vertex-sized outputs and reads no row pointer.
 * Asynchronous on stream, no read-back, no float atomics: one stable radix sort of the 3 n keys (vertex, 3 i + k), one wave per
 * vertex run.  Scratch (the keys) is allocated on the first call of a size only and belongs to the ctx: the ordering rule of the other
 * mesh calls holds.
 * Errors: "null argument" (no output asked for, or an output asked for without its upstream gradient), "bad sizes" (n < 0, n >= 2^30,
 * n_verts < 1, n_faces < 1, n_faces > 2^24, C outside [0, 64]). */
int ra_mesh_closest_backward(ra_ctx* ctx, const int* faces_dev, int n_faces, int n_verts, const float* pts_dev, const float* closest_dev,
                             const int* face_dev, const float* bary_dev, int n, const float* g_d2_dev, const float* g_attr_dev, int C,
                             float* dpts_dev, float* dverts_dev, float* dattr_dev, void* stream);
/* Per point (pts: DEVICE n x 3 fp32) the generalised winding number of the mesh (Jacobson et al. 2013; the reference's winding_number,
 * lib/utils/mesh_utils.py:614-680): winding (n) = sum over every face the mesh kept of sign * Omega / (4 pi), fp32.  About 1 inside a
 * closed mesh whose faces are wound outwards, 0 outside, and a smooth value in between near holes and open boundaries; a flipped face
 * counts negative.  A face with a non-finite vertex was dropped at ra_mesh_create and contributes nothing.  Dense: every point sees
 * every face (no tree, no approximation).
 * Per pair (ra_winding_tri.hpp, every operation a named fp32 operation): u_i = (v_i - p) / |v_i - p|, sign = sign(det[u0 u1 u2]),
 * Omega = 4 atan(sqrt(T + 1e-10)) with T = tan^2(Omega_0 / 4) — the reference's function, its eps included, evaluated through
 * tan(Omega_0 / 4) = |det| / (hypot(det, den) + den), den = 1 + u0.u1 + u1.u2 + u2.u0, instead of its ill-conditioned L'Huilier
 * product; det == 0 (a point in a face's plane, a face of no area) contributes exactly 0.
 * The sum is carried in float64: faces in the mesh's stored order, in chunks of ra_winding_tile(1) records whose sums start from 0
 * and are added in chunk order.  A point's result is therefore a function of (point, mesh) alone, bit for bit: not of n, of the order
 * or the subset of the points, or of the launch shape — below ra_winding_tile(2) point tiles the faces are split across workgroups
 * and a second pass adds the chunk sums in the same order (RA_WINDING_ONE_PASS / RA_WINDING_SPLIT force either shape: the same bits).
 * NaN, as the reference's arithmetic gives it: a point with a non-finite coordinate, and a point bit-equal to a vertex of a kept face
 * (0 / 0 in the normalisation).  No other point of the launch is affected.
 * Asynchronous on stream, no read-back, no float atomics; n == 0 launches nothing and reads no pointer; scratch (the split launch's
 * chunk sums) is allocated on the first call of a size only and belongs to the ctx: the ordering rule of the other mesh calls holds.
 * Errors: "null argument", "bad sizes" (n < 0, n >= 2^30), "unknown flag", "not a mesh of this ctx". */
enum { RA_WINDING_ONE_PASS = 1,   /* test and measurement hooks: every point sums all chunks itself ... */
       RA_WINDING_SPLIT = 2 };    /* ... or one workgroup per (point tile, chunk) and the combining pass, whatever n is (both: "unknown flag") */
int ra_mesh_winding(ra_ctx* ctx, const ra_mesh* mesh, const float* pts_dev, int n, int flags, float* winding_dev, void* stream);
/* test hook: 0 points per tile (workgroup), 1 face records per chunk, 2 point tiles below which the faces are split across workgroups */
int ra_winding_tile(int which);
/* Per point (pts: DEVICE n x 3 fp32) the winding number of ra_mesh_winding AND its gradient with respect to the point: winding (n, may
 * be NULL) and grad (n x 3), fp32.  What the reference gets from autograd through winding_number, in closed form: the gradient of the
 * function ra_mesh_winding computes, its eps under the root included, not of the ideal solid angle.
 * Per pair (ra_winding_grad_tri.hpp, every operation a named fp32 operation), with d_i = v_i - p:
 *   grad (sign Omega) = k(T) sum over the edges (x, y) = (d0, d1), (d1, d2), (d2, d0) of (x cross y) (|x| + |y|) / (|x| |y| (|x| |y| + x.y)),
 *   k(T) = (1 + T) sqrt(T) / ((1 + T + eps) sqrt(T + eps)),  T = tan^2(Omega_0 / 4),  eps = 1e-10
 * — the Biot-Savart form of the gradient of the signed solid angle, times the derivative of 4 atan(sqrt(T + eps)) over that of
 * 4 atan(sqrt(T)), which is far from 1 for a small or distant face.  The value is ra_mesh_winding's bit for bit: the pair's
 * normalisations are formed once and serve both.  det == 0 (a point in a face's plane, a face of no area): value 0 and gradient 0.  A
 * face dropped at ra_mesh_create contributes nothing.
 * Sums: four float64 sums per point (value, gx, gy, gz), faces in the mesh's stored order in chunks of ra_winding_tile(1) records whose
 * sums start from 0 and are added in chunk order; each is scaled by 1 / (4 pi) in float64 and rounded once to fp32.  A row is a
 * function of (point, mesh) alone, bit for bit: not of n, of the order or the subset of the points, or of the launch shape (flags:
 * RA_WINDING_ONE_PASS / RA_WINDING_SPLIT as for ra_mesh_winding; the default splits the faces across workgroups below
 * ra_winding_tile(2) point tiles).
 * Non-finite rows: a point with a non-finite coordinate and a point bit-equal to a vertex of a kept face (value and gradient NaN),
 * and a point on the segment of an edge of a kept face — where the computed |x| |y| + x.y of that edge is not positive: the gradient
 * is NaN (the solid angle jumps there), the value is ra_mesh_winding's.  No other row of the launch is affected.
 * Asynchronous on stream, no read-back, no float atomics; n == 0 launches nothing and reads no pointer; scratch (the split launch's
 * chunk sums, four float64 per point and chunk) is allocated on the first call of a size only and belongs to the ctx: the ordering
 * rule of the other mesh calls holds.
 * Errors: "null argument", "bad sizes" (n < 0, n >= 2^30), "unknown flag", "not a mesh of this ctx". */
int ra_mesh_winding_grad(ra_ctx* ctx, const ra_mesh* mesh, const float* pts_dev, int n, int flags, float* winding_dev, float* grad_dev,
                         void* stream);
/* Per ray (ray_o, ray_d: DEVICE n x 3 fp32; d is not normalised, t is in units of |d|) where it meets the mesh: the reference's
 * moller_trumbore and ray_stabbing (lib/utils/mesh_utils.py:686-738) over the faces the mesh kept.
 *   t (n)       the smallest t over the faces the hit predicate accepts; +inf without a hit
 *   face (n)    the ORIGINAL index of a face that attains it, the lowest among faces of equal fp32 t; -1 without a hit
 *   uv (n x 2)  that pair's u, v (hit point = (1 - u - v) a + u b + v c); NaN without a hit
 *   count (n)   the number of faces the predicate accepts: the reference's inside.count_nonzero, whose parity is ray_stabbing
 * Any output may be NULL, not all four; n == 0 launches nothing and reads no pointer.
 * Per pair (ra_raycast_tri.hpp, every product, fused multiply-add and division a named fp32 operation): the reference's u, v, t, its
 * eps included.  A pair is a hit when (1) the reference's two-sided test holds, t >= 0, u >= 0, v >= 0, u + v <= 1; (2) |det| is above
 * the fp32 rounding bound of its own computation, 2^-21 sum_k |d_k| (|E1 x E2|_k with absolute products) — the grazing guard, the one
 * departure from the reference, which below that bound "hits" faces the ray is nowhere near (a ray in a face's plane, a face of no area,
 * d = 0); (3) the computed t lies in the computed ray interval of the face's own box, widened by 2^-6 relative: an exact hit does, and
 * it is what makes the box sweep exact.  The test is not watertight on shared edges and vertices (u and v are rounded per face), and
 * neither is the reference's: count may be off by one for a ray through an edge.
 * The result is a function of (ray, mesh) alone, bit for bit: not of the leaf order, the pruning, the wave a ray sits in, the order or
 * subset of the rays or the launch shape.  Boxes are pruned by a conservative slab test only; with count_dev given nothing is pruned
 * by t.  The default call, RA_RAYCAST_BRUTE and RA_RAYCAST_UNSORTED agree bit for bit.
 * A ray with a non-finite component of o or d: t = uv = NaN, face = -1, count = -1; no other ray is affected.  A mesh whose every
 * face was dropped: t = +inf, face = -1, uv = NaN, count = 0.
 * Asynchronous on stream, no read-back, no float atomics; scratch (the internal order of the rays) is allocated on the first call of
 * a size only and belongs to the ctx: the ordering rule of the other mesh calls holds.
 * Errors: "null argument", "bad sizes" (n < 0, n >= 2^30), "unknown flag", "not a mesh of this ctx". */
enum { RA_RAYCAST_BRUTE = 1,      /* scan every face, no box test: the in-arithmetic reference of the sweep */
       RA_RAYCAST_UNSORTED = 2 }; /* do not re-order the rays internally (the same bits; test and measurement hook) */
int ra_mesh_raycast(ra_ctx* ctx, const ra_mesh* mesh, const float* ray_o_dev, const float* ray_d_dev, int n, int flags, float* t_dev,
                    int* face_dev, float* uv_dev, int* count_dev, void* stream);
/* test hook: 0 rays per workgroup, 1 pairs per workgroup of ra_ray_tri_pairs, 2 rays up to which a query is never re-ordered */
int ra_raycast_tile(int which);
/* The reference's dense moller_trumbore for tris of shape (f, 3, 3): u, v, t (each DEVICE n x f fp32, ray-major; any may be NULL, not
 * all three) of every (ray, triangle) pair, raycast_tri with NO guard.  o, d: DEVICE n x 3; tris: DEVICE f x 9.  Needs no mesh.
 * n == 0 or f == 0 launches nothing.  Errors: "null argument", "bad sizes" (n < 0, f < 0, n * f >= 2^31). */
int ra_ray_tri_pairs(ra_ctx* ctx, const float* o_dev, const float* d_dev, int n, const float* tris_dev, int f, float* u_dev, float* v_dev,
                     float* t_dev, void* stream);

/* ---- mesh connectivity and Taubin smoothing (lib/utils/mesh_utils.py: triangle_to_halfedge :540-611, get_edges :898-922,
 * get_face_connectivity :146-168, laplacian_smoothing :943-1015) ----
 * An ra_topo is the connectivity of n_faces triangles over n_verts vertices, built once on the device and immutable; it belongs to
 * its ctx like an ra_mesh (freed by ra_topo_destroy or with the ctx) and holds no vertex positions.
 * faces_dev: DEVICE n_faces x 3 int32 (what ra_marching_cubes writes), checked on the device against [0, n_verts).
 * Conventions, the reference's: half-edge 3 f + k leaves corner k of face f towards corner (k + 1) % 3; an edge is the unordered pair
 * of a half-edge's ends and its id is its rank in lexicographic (min, max) order; twin is the other half-edge of an edge that has
 * exactly two, else -(the edge's number of half-edges).  The pairing is symmetric.  Arrays (ra_topo_array; all int32, DEVICE):
 *   RA_TOPO_VERT, _TWIN, _EDGE   3 F each: start vertex, twin, edge id of every half-edge
 *   RA_TOPO_EDGES                E x 2: the true (min, max) of every edge — NOT the reference's get_edges decode, which turns an edge
 *                                (a, faces.max()) into (a + 1, 0)
 *   RA_TOPO_EDGE_COUNTS          E: half-edges per edge (2 = manifold, 1 = boundary)
 *   RA_TOPO_EDGE_HE_START, _HE   E + 1, 3 F: the half-edges of every edge, ascending (for a count of 2: the face connectivity)
 *   RA_TOPO_NBR_START, _NBR      V + 1, 2 E: the neighbours of every vertex through the unique edges, ascending; an edge (a, a), which
 *                                a face with a repeated index makes, lists a twice under a, as the reference's adjacency counts it
 *   RA_TOPO_OUT_START, _OUT_HE   V + 1, 3 F: the half-edges that leave every vertex, ascending
 * ra_topo_create queues everything and then reads back ONCE (the face-index verdict, E and the two largest valences together).
 * n_faces == 0 gives an empty, valid object.  ra_topo_sizes (HOST, no device work): sizes[7] = F, V, E, the longest neighbour list,
 * the most half-edges leaving one vertex, the blocking read-backs of the build, the most half-edges on one edge.  ra_topo_array copies one array to out_dev
 * (asynchronous; an empty array may have out_dev == NULL).
 * Errors: "null argument", "bad sizes", "face index" (outside [0, n_verts)), "not a topology of this ctx", "unknown array". */
typedef struct ra_topo ra_topo;
enum { RA_TOPO_VERT = 0, RA_TOPO_TWIN = 1, RA_TOPO_EDGE = 2, RA_TOPO_EDGES = 3, RA_TOPO_EDGE_COUNTS = 4, RA_TOPO_EDGE_HE_START = 5,
       RA_TOPO_EDGE_HE = 6, RA_TOPO_NBR_START = 7, RA_TOPO_NBR = 8, RA_TOPO_OUT_START = 9, RA_TOPO_OUT_HE = 10 };
int ra_topo_create(ra_ctx* ctx, const int* faces_dev, int n_faces, int n_verts, ra_topo** topo, void* stream);
int ra_topo_destroy(ra_ctx* ctx, ra_topo* topo);
int ra_topo_sizes(ra_ctx* ctx, const ra_topo* topo, int* sizes);
int ra_topo_array(ra_ctx* ctx, const ra_topo* topo, int which, int* out_dev, void* stream);
/* test hook: 0 half-edges / edges / vertices per workgroup of the build, 1 (vertex, channel) results per workgroup of a smoothing
 * pass, 2 the largest channel count of ra_mesh_smooth */
int ra_topo_tile(int which);
/* Taubin lambda | mu smoothing of n_verts x C fp32 rows (positions; albedo, blend weights ... ride along as further channels),
 * 1 <= C <= 64; the reference's laplacian_smoothing on the topology's true edges, float32.  An iteration is two passes; a pass is, per
 * (vertex, channel) and in fp32 operations of one rounding each, no contraction (csrc/ra_topo_rules.hpp):
 *     s = sum of the neighbour rows in ascending neighbour order, from 0;   l = s * inv - v   (inv = 1.0f / deg; 0 for deg = 0);
 *     v' = v + c * l,   c = alpha in the first pass, -(alpha + 0.01f) in the second.
 * Every pass reads the previous pass's buffer and writes another one (the reference's L @ v before +=): 2 x iters launches, no
 * atomics, no read-back; the result is a function of the inputs alone, bit for bit.  inds_dev: DEVICE n_inds int64 row indices —
 * only those rows move, every row is read (mesh_utils.py:1006, 1014); entries outside [0, n_verts) name no row; NULL: every row
 * moves.  values_dev is not modified; out_dev (n_verts x C) must be another array.  iters == 0 copies.  A vertex without
 * neighbours shrinks towards 0 like the reference's (l = -v).
 * Errors: "null argument", "bad sizes", "bad alpha" (NaN), "not a topology of this ctx". */
int ra_mesh_smooth(ra_ctx* ctx, const ra_topo* topo, const float* values_dev, int n_verts, int C, const long long* inds_dev, int n_inds,
                   float alpha, int iters, float* out_dev, void* stream);
/* One Loop subdivision step (halfedge_loop_subdivision, mesh_utils.py:382-514; export_mesh(..., subdivision=N) runs N of them):
 * n_verts x C fp32 rows in, (n_verts + E) x C rows out (row V + e is the new vertex of edge e), 1 <= C <= 64 — positions, and albedo,
 * roughness, blend weights ... carried along; the interior stencil sums to 1.  Every output row is the sum of its half-edges'
 * contributions in ASCENDING half-edge order, each contribution in named fp32 operations of one rounding (csrc/ra_topo_rules.hpp,
 * which states the four rules); the two coefficients per valence come from a table computed in double and rounded once to fp32
 * (ra_loop_weights exposes an entry), which covers the topology's largest valence: the result is a function of the inputs alone,
 * bit for bit.  The reference's quirks are kept: a boundary vertex of one face only gets half its stencil, an unreferenced vertex
 * moves to the origin, a face with a repeated index runs through the same arithmetic.
 * out_faces_dev (nullable): DEVICE 4 F x 3 int32 — face h < 3 F is (vert[h], V + edge[h], V + edge[prev h]), face 3 F + f holds the
 * three edge vertices of face f.  *child (nullable): a new ra_topo of the subdivided mesh, owned by the ctx, made by the reference's
 * index arithmetic on twin / vert / edge (:419-451): no sort, and no read-back, since E' = 2 E + 3 F is known.  Its edge ids are that
 * arithmetic's (edge e splits into 2 e and 2 e + 1, the middle edge opposite half-edge h is 2 E + h), NOT lexicographic ranks;
 * RA_TOPO_EDGES lists the ends of each id's lowest half-edge.  On an edge shared by three or more faces the two halves get their ids
 * the opposite way round from the two directions, as in the reference, so an id there names half-edges of both halves: chained
 * steps on such a mesh differ from a freshly built topology of the same faces; on closed and open manifold
 * meshes they agree in every corner position.  Of the child's ra_topo_sizes the longest neighbour list is an upper bound.
 * Without child the call synchronises the stream once when out_faces_dev is given (the faces are written through a temporary).
 * Errors: "null argument", "bad sizes" (n_verts, C; a step whose 12 F half-edges or (V + E) x C values would leave int32),
 * "not a topology of this ctx". */
int ra_mesh_subdivide(ra_ctx* ctx, const ra_topo* topo, const float* values_dev, int n_verts, int C, float* out_values_dev, int* out_faces_dev,
                      ra_topo** child, void* stream);
/* test hook: the Loop coefficients of a vertex with n >= 1 outgoing half-edges, w_self = 1 / n - beta and
 * beta = (1 / n)(5 / 8 - (3 / 8 + cos(2 pi / n) / 4)^2), as the library's table holds them (double, rounded once) */
int ra_loop_weights(int n, float* w_self, float* beta);
/* The vertex-mask dilation of segment_mesh (mesh_utils.py:226-236), (A^steps mask) != 0 as a neighbour-OR: after a step a vertex is
 * set when one of its neighbours was (NOT when only itself was: the adjacency has no diagonal).  mask_dev, out_dev: DEVICE n_verts
 * bytes, non-zero = set; out_dev holds 0 / 1 and must be another array; steps == 0 copies. */
int ra_topo_dilate(ra_ctx* ctx, const ra_topo* topo, const unsigned char* mask_dev, int n_verts, int steps, unsigned char* out_dev,
                   void* stream);

/* ---- mesh fitting: what bidirectional_icp_fitting (lib/utils/mesh_utils.py:265-379) takes from largesteps, pytorch3d and
 * bvh_distance_queries, on a topology's neighbour lists and a mesh's closest-point query ----
 * Common to all five calls: fp32 in and out, float64 inside; every operation a named one of one rounding, no contraction
 * (csrc/ra_fit_rules.hpp states each rule); one thread per (vertex, channel), neighbours added in ascending order; every sum across
 * workgroups is per-workgroup partial sums in a fixed tree order, added again by one workgroup in a fixed order; no float atomics, no read-back, and no
 * kernel waits for another workgroup.  Every result is a function of its inputs alone, bit for bit.  Asynchronous on stream; scratch
 * belongs to the ctx (the ordering rule of the other mesh calls).
 *
 * The operator is largesteps' compute_matrix, M = I + lambda L with L = D - A the combinatorial Laplacian of the topology's unique
 * edges (RA_TOPO_NBR_START / _NBR; positions are not used).  An entry of a neighbour list that names the vertex itself (an edge (a, a))
 * is skipped: it cancels between D and A.  A vertex without neighbours has the row x = b.  M is symmetric positive definite.
 * ra_topo_diffuse_apply (to_differential): out = fl32(x + lambda (deg x - s)), s the ascending neighbour sum, n_verts x C rows,
 * 1 <= C <= 64; out_dev must not be x_dev.
 * ra_topo_diffuse_solve (from_differential; its gradient is the same call, M being symmetric): Jacobi-preconditioned conjugate
 * gradients on M x = b from x0 (x0_dev == NULL: 0), the C channels C independent systems with their own scalars.  A channel stops when
 * |r|_2 <= tol |b|_2 (float64 norms, r the recurrence residual) and is frozen from then on, so its result depends on its own column of
 * b and x0, the topology, lambda, tol and max_iter alone: the same bits alone or beside other channels.  The host queues max_iter
 * iterations of four launches each; a launch of a stopped channel returns at once.  A channel with b = 0 gives x = 0 exactly; a channel
 * whose b or x0 holds a non-finite value gives NaN in that channel only; max_iter == 0 stores x0 (under those two rules).
 * info_dev (nullable): DEVICE, per channel 16 bytes { int32 iterations used; int32 stop reason (0 max_iter reached, 1 converged,
 * 2 b = 0, 3 non-finite, 4 p.Mp <= 0); float64 final |r| / |b| }.
 * Errors: "null argument", "bad sizes" (n_verts of the topology, C, 0 <= max_iter < 2^20), "bad lambda" (NaN, negative, infinite),
 * "bad tol" (outside [0, 1)), "not a topology of this ctx". */
int ra_topo_diffuse_apply(ra_ctx* ctx, const ra_topo* topo, const float* x_dev, int n_verts, int C, float lambda, float* out_dev, void* stream);
int ra_topo_diffuse_solve(ra_ctx* ctx, const ra_topo* topo, const float* b_dev, int n_verts, int C, float lambda, const float* x0_dev, double tol,
                          int max_iter, float* out_dev, void* info_dev, void* stream);
/* Normals and areas of the topology's faces at verts_dev (n_verts x 3); the corners of face f are RA_TOPO_VERT[3 f + k].  Any output may
 * be NULL, not all three.
 *   face_normal (F x 3)  the reference's face_normals (:130-143): n = (v1 - v0) x (v2 - v1), n / (|n| + 1e-8)
 *   face_area (F)        the reference's get_face_areas (:193-201): |(v2 - v0) x (v1 - v0)| / 2
 *   vert_normal (V x 3)  pytorch3d's verts_normals: the sum of the UNNORMALISED n (area-weighted) over the vertex's outgoing half-edges
 *                        in ascending order (RA_TOPO_OUT_*), divided by max(|.|, 1e-6); a vertex no face uses gets 0
 * Errors: "null argument", "bad sizes", "not a topology of this ctx". */
int ra_mesh_normals(ra_ctx* ctx, const ra_topo* topo, const float* verts_dev, int n_verts, float* face_normal_dev, float* face_area_dev,
                    float* vert_normal_dev, void* stream);
/* The residual of icp_loss (:265-291) for n points with normals against a mesh: closest point and face as ra_mesh_closest gives them
 * (without gradient: the closest points are constants, which is plain ICP), delta = p - closest; a row is kept when
 * d2 < fl32(dist_th^2) AND dot(face_normals[face], pt_normals[row]) > angle_th.  face_normals_dev: F x 3 in the ORIGINAL face order.
 *   sums_dev   DEVICE float64[2]: the sum of |delta|^2 over the kept rows, and their count; the loss is sums[0] / sums[1], NaN for
 *              count 0 as the reference's empty mean()
 *   grad_dev   (nullable) n x 3: d loss / d pts = (2 / count) delta on kept rows, 0 elsewhere (all 0 for count 0)
 *   keep_dev   (nullable) n bytes: 1 where the row is kept
 * A point with a non-finite coordinate is not kept and disturbs no other row.  n == 0 writes sums = (0, 0).
 * Errors: "null argument", "bad sizes", "bad threshold" (NaN), "not a mesh of this ctx". */
int ra_icp_residual(ra_ctx* ctx, const ra_mesh* mesh, const float* pts_dev, const float* pt_normals_dev, int n, const float* face_normals_dev,
                    float dist_th, float angle_th, double* sums_dev, float* grad_dev, unsigned char* keep_dev, void* stream);
/* One step t = step >= 1 of largesteps' AdamUniform on n parameters (param, grad, g1: DEVICE n fp32; g2: DEVICE ONE float per tensor):
 *   g1 = b1 g1 + (1 - b1) grad;   g2 = b2 g2 + (1 - b2) max(grad^2);   p -= lr (g1 / (1 - b1^t)) / (1e-8 + sqrt(g2 / (1 - b2^t)))
 * Two launches: the maximum (of bit patterns: order-free, hence exact; a NaN gradient makes it NaN), then the update.  b1^t and b2^t
 * are t - 1 float64 multiplications on the host.
 * Errors: "null argument", "bad sizes" (n outside [0, 2^31), step outside [1, 2^24)), "bad lr or betas". */
int ra_adam_uniform_step(ra_ctx* ctx, float* param_dev, const float* grad_dev, float* g1_dev, float* g2_dev, long long n, int step, float lr,
                         float b1, float b2, void* stream);
/* test hook: 0 vertices of one channel per workgroup of the solve's kernels, 1 rows per workgroup of the residual's */
int ra_fit_tile(int which);

/* ---- cloth energies: the garment model of lib/utils/physx_utils.py (StVKMaterial, Garment, stretch_energy :242-267, bending_energy
 * :270-311, gravity_energy, inertia_term / dynamic_term :322-351) with the gradient with respect to the vertex positions ----
 * An ra_cloth is an immutable garment on a topology: per face the rest area (get_face_areas) and Dm_inv — get_shape_matrix of the 2-D
 * material triangle vm[fm], inverted as torch_inverse_2x2 does, its det + 2^-23 included —, per vertex the mass
 * (the sum of density area / 3 over its faces in ascending outgoing-half-edge order; a vertex no face uses has mass 0 and
 * inv_mass = inf) and, per EDGE of the topology, a hinge where the edge has exactly two half-edges.  Hinges are addressed by edge id:
 * in edge order they are the reference's get_face_connectivity, the lower half-edge's face first.  It belongs to its ctx (freed by
 * ra_cloth_destroy or with the ctx) and reads its topology, which must outlive it (ra_topo_destroy refuses meanwhile).
 * rest_verts_dev: n_verts x 3 fp32; vm_dev: n_vm x 2 fp32; fm_dev: n_faces x 3 int32, checked on the device against [0, n_vm) before
 * anything dereferences it — the ONE blocking read-back of the build (4 bytes).  The material's derived coefficients (A,
 * stretch_coeff, bending_coeff, lame_mu, lame_lambda: ra_cloth_material_derive, HOST, float64, StVKMaterial.__init__) are computed in
 * float64 and rounded once.  Arrays (ra_cloth_array, DEVICE, asynchronous): F_AREA F fp32, DM and DM_INV F x 4 fp32 (row-major 2 x 2),
 * V_MASS and INV_MASS V fp32, HINGE_FACES and HINGE_VERTS E x 2 int32 with -1 where the edge is no hinge.
 * Errors: "null argument", "bad sizes" (n_verts of the topology, n_vm, 18 E < 2^31), "bad material" (a non-finite parameter),
 * "material index" (fm outside [0, n_vm)), "not a topology / cloth of this ctx", "unknown array". */
typedef struct ra_cloth ra_cloth;
typedef struct ra_cloth_material {
    double density, thickness, young_modulus, poisson_ratio, bending_multiplier, stretch_multiplier, material_multiplier;
} ra_cloth_material;
enum { RA_CLOTH_F_AREA = 0, RA_CLOTH_DM = 1, RA_CLOTH_DM_INV = 2, RA_CLOTH_V_MASS = 3, RA_CLOTH_INV_MASS = 4, RA_CLOTH_HINGE_FACES = 5,
       RA_CLOTH_HINGE_VERTS = 6 };
enum { RA_CLOTH_STRETCH = 1, RA_CLOTH_BENDING = 2, RA_CLOTH_GRAVITY = 4 };
int ra_cloth_material_derive(const ra_cloth_material* material, double* out5);
int ra_cloth_create(ra_ctx* ctx, const ra_topo* topo, const float* rest_verts_dev, int n_verts, const float* vm_dev, int n_vm, const int* fm_dev,
                    const ra_cloth_material* material, ra_cloth** cloth, void* stream);
int ra_cloth_destroy(ra_ctx* ctx, ra_cloth* cloth);
int ra_cloth_array(ra_ctx* ctx, const ra_cloth* cloth, int which, void* out_dev, void* stream);
/* The selected terms (a bit set of RA_CLOTH_STRETCH, _BENDING, _GRAVITY) at B rows of positions x_dev (B x n_verts x 3 fp32).
 *   energy_dev  DEVICE float64 B x 3: per row the sums of the per-face stretch, per-hinge bending and per-vertex gravity (g mass y)
 *               energies, 0 for a term that is not selected; NOT divided by B
 *   grad_dev    (nullable) B x n_verts x 3 fp32: the gradient of the row's selected terms' sum with respect to x
 * Element arithmetic is fp32, one named operation per rounding (csrc/ra_cloth_rules.hpp).  Element kernels write corner gradients to
 * scratch; a vertex kernel adds a vertex's face corners in ascending half-edge order, then its hinge slots in ascending (hinge, slot)
 * order, each term on its own, and then (stretch + bending) + gravity.  Energies are float64 sums in fixed chunks of one row.  No float
 * atomics: row b of every output is a function of x[b] and the cloth alone, bit for bit — not of B, the other rows, the other
 * selected terms or the launch geometry.  Asynchronous, no read-back.
 * Errors: "null argument", "bad sizes" (1 <= B <= 65535, B x elements < 2^31), "bad terms" (none, or an unknown bit), "bad gravity"
 * (NaN), "not a cloth of this ctx". */
int ra_cloth_energy(ra_ctx* ctx, const ra_cloth* cloth, const float* x_dev, int B, int terms, float gravity, double* energy_dev, float* grad_dev,
                    void* stream);
/* inertia_term, or dynamic_term when accel3 (HOST, 3 floats) is non-NULL, over rows x V vertices with mass_dev (V fp32):
 * d = x_next - (x_curr + dt v_curr (+ dt dt accel)), value_dev[row] (DEVICE float64) = the row's sum of (d . d) mass / (2 dt dt), NOT
 * divided by rows; g_next = d mass / (dt dt), g_curr = -g_next, g_vel = -dt g_next (each nullable, rows x V x 3 fp32).
 * Errors: "null argument", "bad sizes" (1 <= rows <= 65535, V >= 1, rows x V < 2^31), "bad delta_t" (NaN or 0). */
int ra_cloth_inertia(ra_ctx* ctx, const float* mass_dev, const float* x_next_dev, const float* x_curr_dev, const float* v_curr_dev, int rows, int V,
                     float delta_t, const float* accel3, double* value_dev, float* g_next_dev, float* g_curr_dev, float* g_vel_dev, void* stream);
/* test hook: elements per workgroup of 0 the face kernel, 1 the hinge kernel, 2 the vertex kernel; 3 elements per chunk of an energy sum */
int ra_cloth_tile(int which);

/* ---- mesh rasterisation: what the reference's lib/utils/raster_utils.py asks of nvdiffrast (rasterize, interpolate), with gradients ----
 * Homogeneous (clipless) rasterisation of B views of one face list.  pos_dev: B x n_verts x 4 fp32 clip-space (x, y, z, w);
 * faces_dev: n_faces x 3 int32, shared by the views.  Pixel (ix, iy) is sampled at NDC ((2 ix + 1) / W - 1, (2 iy + 1) / H - 1): row 0
 * is at y = -1.  The rule of a (pixel, face) pair — canonical per-edge edge functions, the tie rule on an edge, the face's pixel box,
 * perspective-correct barycentrics, w > 0 and -1 <= z/w <= 1 — is csrc/ra_raster_rules.hpp's, one named fp32 operation per rounding;
 * two faces that share an edge decide a sample on it from the same bits, so a consistently oriented mesh has neither cracks nor
 * doubly owned pixels along interior edges.  Per pixel the lexicographic minimum of (z/w, face index) wins: the maps are a function of
 * the pixel and the mesh alone, bit for bit, not of the launch or of the order in which faces are met.
 *   uv_dev B x H x W x 2 fp32 (the barycentrics of corners 0 and 1), zw_dev B x H x W fp32, face_dev B x H x W int32 (-1: empty;
 *   uv and zw hold 0 there).
 * Set-up per (view, face), deterministic binning into 8 x 8-pixel tiles (sum, keys, radix sort), one wave per tile.  ONE blocking
 * read-back per call, 8 bytes: the (tile, face) pair count, which sizes the key buffers, and the face-index verdict; everything else
 * is asynchronous on the stream.  RA_RASTER_BRUTE scans every face per pixel without binning: the same bits (it still reads the
 * verdict back).  n_faces == 0 launches nothing and returns empty maps.  Scratch belongs to the ctx.
 * Errors: "null argument", "bad sizes" (B, H, W >= 1, B x H x W < 2^31, n_faces < 2^24, B x n_faces < 2^31, fewer than 2^31 pairs),
 * "unknown flag", "face index" (an index outside [0, n_verts), found on the device). */
enum { RA_RASTER_BRUTE = 1 };
int ra_rasterize(ra_ctx* ctx, const float* pos_dev, int B, int n_verts, const int* faces_dev, int n_faces, int H, int W, int flags, float* uv_dev,
                 float* zw_dev, int* face_dev, void* stream);
/* out[b, y, x, :] = (u a_0 + v a_1) + ((1 - u) - v) a_2 over the A (1..64) channels of the pixel's face's corners, 0 where the pixel
 * is empty.  attr_dev: n_verts x A fp32 shared by the views (per_view == 0) or B x n_verts x A.  A face id outside [0, n_faces) or a
 * vertex index outside [0, n_verts) gives 0 at that pixel (ra_rasterize is the call that reports indices).  Asynchronous, no read-back.
 * Errors: "null argument", "bad sizes". */
int ra_interpolate(ra_ctx* ctx, const float* attr_dev, int per_view, int n_verts, int A, const int* faces_dev, int n_faces, const float* uv_dev,
                   const int* face_dev, int B, int H, int W, float* out_dev, void* stream);
/* The backward passes.  Both read the faces from a topology of the same face list (ra_topo_create, whose build checked them) and use
 * its vertex -> half-edge lists; the face map is held fixed and zw and face carry no gradient, as in nvdiffrast.
 * ra_interpolate_backward: dout_dev B x H x W x A -> dattr_dev (nullable; n_verts x A summed over the views when the attributes are
 * shared, else B x n_verts x A) and duv_dev (nullable; B x H x W x 2, 0 where empty).
 * ra_rasterize_backward: duv_dev B x H x W x 2 -> dpos_dev B x n_verts x 4, the gradient of the computed (u, v) in the clip-space
 * positions (the z component is 0).
 * Reduction order: no float atomics.  The pixels are grouped by (view, face) with one radix sort; one wave per (view, face) adds its
 * pixels in ascending order per lane and the lanes in a fixed tree, writes corner gradients to scratch, and a vertex pass adds a
 * vertex's corners in ascending half-edge order (shared attributes: each view's sum, the views ascending).  Every output row is a
 * function of its inputs alone, bit for bit; row b of dpos does not depend on the other views.  Asynchronous, no read-back.
 * Errors: "null argument", "bad sizes", "not a topology of this ctx". */
int ra_interpolate_backward(ra_ctx* ctx, const ra_topo* topo, const float* attr_dev, int per_view, int n_verts, int A, const float* uv_dev,
                            const int* face_dev, int B, int H, int W, const float* dout_dev, float* dattr_dev, float* duv_dev, void* stream);
int ra_rasterize_backward(ra_ctx* ctx, const ra_topo* topo, const float* pos_dev, int B, int n_verts, int H, int W, const float* uv_dev,
                          const int* face_dev, const float* duv_dev, float* dpos_dev, void* stream);
/* test hook: 0 pixels per tile edge (a tile is one wave), 1 elements per workgroup of the set-up, interpolation and vertex kernels,
 * 2 the largest channel count */
int ra_raster_tile(int which);

/* ---- silhouette antialiasing: what the reference's render_nvdiffrast asks of dr.antialias, with position gradients ----
 * color_dev B x H x W x C fp32 (C >= 1, no upper bound), zw_dev / face_dev: ra_rasterize's maps of the same views, pos_dev B x n_verts x 4
 * the clip-space positions they were rasterised from, topo: a topology of the same face list -> out_dev B x H x W x C.
 * The rule is csrc/ra_antialias_rules.hpp's, this project's statement of Laine et al. 2020 section 3.4, one named fp32 operation per
 * rounding.  A PAIR is two 4-adjacent pixels with different face ids.  Its OWN pixel is the covered one, or the winner of the depth
 * rule (z/w, face id).  Among the three edges of the own pixel's face, ascending, the first one counts whose ends have w > 0, that
 * straddles the line through the own centre along the pair's axis, whose crossing lies at d in [0, 1] pixels from the own centre
 * towards the other pixel, and that is a silhouette in this view (not exactly two half-edges, a dropped twin face, or both faces on the
 * same side of it); alpha = d - 0.5.  alpha >= 0: out[other] += alpha (in[own] - in[other]); else out[own] += -alpha (in[other] -
 * in[own]); always from the INPUT colours.  A pixel adds its pairs in the order left, right, up, down.  A face id outside [-1, F) makes
 * its pairs inert.  Deviations from nvdiffrast: no fixed-point snapping, and only the own pixel's face is searched (as in the paper).
 * ra_antialias: one thread per (pixel, four channels) gathers its four pairs — both pixels of a pair evaluate the same function of the
 * pair and get the same bits.  No atomics, asynchronous, NO read-back.  B x H x W == 0 writes nothing; an empty topology copies color.
 * ra_antialias_backward: dout_dev B x H x W x C -> dcolor_dev (nullable; the transposed gather) and dpos_dev (nullable; B x n_verts x 4,
 * the z component 0), the face map and the set of active pairs held fixed; pos_gradient_boost multiplies dpos only (the finished sum).
 * Reduction order of dpos: no float atomics.  Every pair slot (view, 2 pixel + axis) gets the key (view, half-edge of its edge, slot);
 * the active ones are compacted in ascending slot order and their number is read back — the ONE blocking read-back of the backward
 * (4 bytes, only with dpos; it sizes the sort and the launch); one radix sort of the active keys groups them by (view, half-edge); one
 * wave per run adds d L / d C of its pairs in ascending order per lane (pairs l, l + 64, ...) and the lanes in the fixed xor tree 32,
 * 16, .., 1, and writes the gradients of the half-edge's two ends to zeroed scratch; a vertex pass adds, over the vertex's outgoing
 * half-edges in ascending order, the tail term of each and then the head term of the half-edge before it in its face.  Row b of dpos
 * depends on view b alone; the same bits every time.  Otherwise asynchronous.  Scratch belongs to the ctx and only grows.  Outputs of
 * no elements may be null.
 * Errors: "null argument", "bad sizes" (C >= 1, B x H x W x C < 2^31, n_verts of the topology; with dpos B x H x W < 2^30), "not a
 * topology of this ctx". */
int ra_antialias(ra_ctx* ctx, const ra_topo* topo, const float* color_dev, int C, const float* pos_dev, int B, int n_verts, const float* zw_dev,
                 const int* face_dev, int H, int W, float* out_dev, void* stream);
int ra_antialias_backward(ra_ctx* ctx, const ra_topo* topo, const float* color_dev, int C, const float* pos_dev, int B, int n_verts, const float* zw_dev,
                          const int* face_dev, int H, int W, const float* dout_dev, float pos_gradient_boost, float* dcolor_dev, float* dpos_dev,
                          void* stream);

/* ---- the texture path: what the reference's render_nvdiffrast asks of dr.interpolate(rast_db=, diff_attrs=) and dr.texture ----
 * The rule is csrc/ra_texture_rules.hpp's, this project's statement of Laine et al. 2020 section 3.3, one named fp32 operation per
 * rounding: pixel differentials of the barycentrics, a 2 x 2-mean mip chain, a level of detail from the squared major axis of the
 * pixel's footprint (its log2 is a fixed polynomial: the same bits on the host and the device), bilinear / trilinear / nearest taps
 * with wrap or clamp.  A uv that is not finite (or beyond 2^30 texels) gives 0 and no gradient.  No entry point reads anything back.
 * ra_raster_db: pos_dev B x n_verts x 4, faces_dev n_faces x 3, face_dev B x H x W (ra_rasterize's) -> rast_db_dev B x H x W x 4 =
 *   (du/dX, du/dY, dv/dX, dv/dY), 0 where the pixel is empty.  One lane per pixel.
 * ra_interpolate_da: attr_dev (n_verts x A, or B x n_verts x A with per_view), channels: n HOST ints in [0, A), 1 <= n <= 64 ->
 *   out_da_dev B x H x W x 2n = (da_0/dX, da_0/dY, da_1/dX, ...).  Forward only.
 * ra_texture_mips: the chain of tex_dev Bt x TH x TW x C into mips_dev, Bt x offsets[*lmax + 1] x C floats, level l of texture t at
 *   (t offsets[*lmax + 1] + offsets[l]) C, level 0 included.  offsets: RA_TEX_MAX_LEVELS + 1 HOST entries; they and *lmax are host
 *   arithmetic from the sizes alone, and with mips_dev == NULL nothing else happens (ctx and tex_dev may be null).
 * ra_texture: tex_dev Bt x TH x TW x C (Bt = 1: shared by the views, or B), row 0 at v = 0; uv_dev B x H x W x 2; uv_da_dev B x H x W x 4
 *   (needed by RA_TEX_FILTER_TRILINEAR alone, else ignored) -> out_dev B x H x W x C.  A per-pixel gather.
 * ra_texture_backward: dout_dev B x H x W x C -> duv_dev B x H x W x 2 (nullable) and dtex_dev Bt x TH x TW x C (nullable), first
 *   order: the texel cells, the level pair and lod held fixed, no gradient to uv_da.  dtex uses no float atomics: the tap slots
 *   (view, pixel, tap) are sorted by (view, level, texel), one wave sums a run in a fixed lane and tree order, a last pass folds the
 *   chain into level 0 and adds the views of a shared texture in ascending order: the same bits every time, and row t of a per-view
 *   dtex depends on view t alone.  The tap count is not compacted.  Scratch belongs to the ctx and only grows.
 * Errors, all named before the ctx is touched: "bad sizes" (Bt = 1 or B, 1 <= TH, TW <= 32768, 1 <= C <= 64, max_mip_level >= 0,
 * Bt x TH x TW x C < 2^31, B x H x W x C < 2^31; with dtex the tap-count limit B x H x W x taps < 2^31 - 1, taps = 1 / 4 / 8 for
 * nearest / linear / trilinear), "unknown mode", "null argument". */
#define RA_TEX_FILTER_NEAREST 0
#define RA_TEX_FILTER_LINEAR 1
#define RA_TEX_FILTER_TRILINEAR 2       /* nvdiffrast's linear-mipmap-linear */
#define RA_TEX_BOUNDARY_WRAP 0
#define RA_TEX_BOUNDARY_CLAMP 1
#define RA_TEX_MAX_LEVELS 16
int ra_raster_db(ra_ctx* ctx, const float* pos_dev, int B, int n_verts, const int* faces_dev, int n_faces, const int* face_dev, int H, int W,
                 float* rast_db_dev, void* stream);
int ra_interpolate_da(ra_ctx* ctx, const float* attr_dev, int per_view, int n_verts, int A, const int* faces_dev, int n_faces, const int* face_dev,
                      const float* rast_db_dev, int B, int H, int W, const int* channels, int n, float* out_da_dev, void* stream);
int ra_texture_mips(ra_ctx* ctx, const float* tex_dev, int Bt, int TH, int TW, int C, int max_mip_level, float* mips_dev, int* lmax, long long* offsets,
                    void* stream);
int ra_texture(ra_ctx* ctx, const float* tex_dev, int Bt, int TH, int TW, int C, const float* uv_dev, const float* uv_da_dev, int B, int H, int W,
               int filter, int boundary, int max_mip_level, float* out_dev, void* stream);
int ra_texture_backward(ra_ctx* ctx, const float* tex_dev, int Bt, int TH, int TW, int C, const float* uv_dev, const float* uv_da_dev, int B, int H, int W,
                        int filter, int boundary, int max_mip_level, const float* dout_dev, float* duv_dev, float* dtex_dev, void* stream);
/* 0: the largest C, 1: RA_TEX_MAX_LEVELS, 2: the largest extent, 3: the channels a wave of the run pass sums per trip */
int ra_texture_tile(int which);

/* ---- mesh extraction: the two steps the reference's mesh renderer leaves to mcubes and trimesh (mesh_renderer.py:74-84) ----
 * ra_marching_cubes: classic marching cubes on a DEVICE volume of nx x ny x nz fp32 values, x slowest (what reshape gives), with the
 * classic corner and edge numbering, 256-entry tables derived by rule (relightableavatar_amd/mcubes_tables.py) and linear
 * interpolation.  A corner is below when v < iso, so a NaN counts as not below (and a vertex next to one is NaN); cells all of whose
 * corners are on one side give nothing.  Each grid edge whose ends straddle iso carries exactly ONE vertex, owned by the lower of its
 * two grid points; each cell is owned by its minimum corner.  A vertex is in index coordinates, fp32: the owning point's (x, y, z) with
 * t = (iso - a) / (b - a) added along the edge's axis, a the value at the owning point, b at the other end, every step one rounded
 * fp32 operation (sub, sub, div, add).  Vertices are ordered by (owning point's linear index, axis x < y < z), faces by (cell's
 * minimum corner's linear index, order in the table); no atomic decides an index, so the output is a function of the volume alone,
 * bit for bit.  Face normals (right-hand rule) point towards SMALLER volume values.
 * Two calls.  verts_dev == faces_dev == NULL: the size query — classifies, sums, writes the two counts to *n_verts / *n_faces (HOST)
 * and synchronises the stream once.  The next call with the same volume pointer, sizes and iso and arrays of n_verts x 3 fp32 /
 * n_faces x 3 int32 (DEVICE; NULL allowed where the count is 0) writes the mesh, asynchronously, and uses the query up.  The volume
 * must not change in between (if it does the mesh is wrong; nothing is written outside the arrays).
 * Errors: "null argument", "bad sizes" (an axis below 2, more than 2^27 points), "bad iso", "no size query". */
/* ra_sdf_volume: the scalar volume in front of marching cubes (mesh_renderer.py:42-72).  xs / ys / zs: DEVICE fp32 axis coordinates
 * (the caller's torch.arange(lo, hi + vs, vs): nothing here re-derives arange's rounding); the grid point (x, y, z) is
 * (xs[x], ys[y], zs[z]).  verts: DEVICE n_verts x 3 fp32, what the filter measures against (the template vertices for
 * RA_VOLUME_CANONICAL / _TPOSE, the world vertices for _POSED).  Per point: the exact K (1..4) nearest vertices by an exhaustive scan,
 * d2 = (dx^2 + dy^2) + dz^2; d_k = sqrt(d2_k), w_k = 1 / (d_k + 1e-8) normalised; t = sum w_k d_k; kept when t < dist_th
 * (sample_blend_K_closest_points without values, sample_utils.py:631-641, as mesh_renderer.py:44-46 calls it).
 * A kept cell gets -sdf of the mode's decoder on the compensated (fp32-grade) tier — canonical: sdf(x); tpose: sdf(x + resd(x)), as
 * ra_observed_sdf; posed: the hierarchical world query without the smooth transition, as ra_hdq_sdf(x, dist_th, 0) — every other
 * cell and the pad get `fill`.  volume: DEVICE (nx + 2 pad) x (ny + 2 pad) x (nz + 2 pad) fp32, x slowest.  Needs weights and a frame.
 * One blocking read-back (the kept count, also written to *n_kept when not NULL), then asynchronous.
 * Errors: "null argument", "unknown mode", "bad sizes", "bad K", "bad dist_th or fill". */
enum { RA_VOLUME_CANONICAL = 0, RA_VOLUME_TPOSE = 1, RA_VOLUME_POSED = 2 };
int ra_sdf_volume(ra_ctx* ctx, const float* xs_dev, int nx, const float* ys_dev, int ny, const float* zs_dev, int nz, int mode,
                  const float* verts_dev, int n_verts, int K, float dist_th, float fill, int pad, float* volume_dev, int* n_kept,
                  void* stream);
int ra_marching_cubes(ra_ctx* ctx, const float* volume_dev, int nx, int ny, int nz, float iso, float* verts_dev, int* faces_dev,
                      int* n_verts, int* n_faces, void* stream);
/* The backward of ra_marching_cubes and grid attributes carried to its vertices (csrc/ra_mcubes_grad_rules.hpp).
 * A crossed edge owned by grid point p along `axis`, q its other end, a = vol[p], b = vol[q], v its vertex index (the forward's):
 *   d = b - a, t = (iso - a) / d — the forward's own bits;
 *   attribute forward: attr[v][c] = (1 - t) A[p][c] + t A[q][c], two products and one add;
 *   gt = dverts[v][axis] (+0 without dverts), then gt += dattr[v][c] * (A[q][c] - A[p][c]) for c ascending; s = gt / d;
 *   dvolume[p] += (t - 1) s, dvolume[q] += -(t s); dA[p][c] += (1 - t) dattr[v][c], dA[q][c] += t dattr[v][c].
 * Every step is one rounded fp32 operation.  A grid point adds its terms from +0 in a fixed order — its own edges towards +x, +y, +z,
 * then the edges arriving from -x, -y, -z — as a gather: no float atomics, the same bits on every run.  The set of crossed edges is
 * held fixed (no d / d iso, no second order).  An edge with a non-finite end contributes nothing to either end.
 * attrs_dev: DEVICE n x C fp32 (n = nx ny nz grid points, x slowest), 0 <= C <= 64.
 * ra_marching_cubes_attrs writes out_dev (n_verts x C) in the forward's vertex order.
 * ra_marching_cubes_backward: dverts_dev n_verts x 3 or NULL, dattr_dev n_verts x C (C == 0: attrs / dattr are not read), dvolume_dev n or
 * NULL, dattrs_grid_dev n x C or NULL (one of the two at least); every output is written in full, zeros included.
 * Both are asynchronous and make NO read-back: they classify and sum the volume they are given again, in scratch of their own (a
 * pending size query of ra_marching_cubes stays valid), and bound every vertex access by n_verts — a volume that changed since the
 * forward gives a wrong result, never an access outside the arrays.  n_verts == 0: the outputs are zero-filled, nothing else runs.
 * Errors, before the ctx is touched: "null argument", "bad sizes" (an axis below 2, more than 2^27 points, C outside 0..64, n C,
 * 3 n_verts or n_verts C not below 2^31), "bad iso". */
int ra_marching_cubes_attrs(ra_ctx* ctx, const float* volume_dev, int nx, int ny, int nz, float iso, const float* attrs_dev, int C, int n_verts,
                            float* out_dev, void* stream);
int ra_marching_cubes_backward(ra_ctx* ctx, const float* volume_dev, int nx, int ny, int nz, float iso, const float* dverts_dev, int n_verts,
                               const float* attrs_dev, const float* dattr_dev, int C, float* dvolume_dev, float* dattrs_grid_dev, void* stream);
/* The largest component of a triangle mesh, components being sets of faces connected through SHARED EDGES (two faces that only share
 * a vertex are not connected) — trimesh's split(only_watertight=False) followed by "the one with the most vertices".  Size = the
 * number of distinct vertices the component's faces refer to; among equals the component that holds the lowest face index wins.  The
 * result keeps the referenced vertices in their original order and the component's faces in their original order, re-indexed.
 * Nothing else is done to the mesh: coincident vertices are not merged and degenerate faces are not dropped (trimesh.Trimesh's own
 * processing is not reproduced).
 * verts: DEVICE n_verts x 3 fp32, faces: DEVICE n_faces x 3 int32; both are checked on the device.  Two calls, as above: the size query
 * (out_verts_dev == out_faces_dev == NULL) sorts the edges, lowers face labels to the component's lowest face index — integer minima
 * only: the result does not depend on the order of execution — and reads the counts back ONCE: ra_mcubes_tile(1) label passes are
 * queued together and decide on the device whether they still have work (a mesh that needs more gets another batch and another
 * read-back; correct for any mesh); the second call gathers into out_verts_dev / out_faces_dev.  n_faces == 0: (0, 0).
 * Errors: "null argument", "bad sizes", "face index" (an index outside [0, n_verts), reported by the size query), "no size query". */
int ra_mesh_largest_component(ra_ctx* ctx, const float* verts_dev, int n_verts, const int* faces_dev, int n_faces, float* out_verts_dev,
                              int* out_faces_dev, int* n_out_verts, int* n_out_faces, void* stream);
/* test hook: 0 grid points / faces / edges per workgroup, 1 label passes queued per read-back of the component search, 2 vertices per
 * LDS tile of the volume filter (= its workgroup size), 3 the largest K of the volume filter */
int ra_mcubes_tile(int which);
/* measurement hook: the blocking read-backs (stream synchronisations behind a device-to-host copy) that this ctx's last
 * 0 ra_sdf_volume, 1 ra_marching_cubes size query, 2 ra_mesh_largest_component size query made, counted where they happen;
 * 3 the label passes of that last component query that lowered a label; -1 for a null ctx */
int ra_mesh_extract_stats(const ra_ctx* ctx, int which);

/* ---- test hooks: stage outputs for the parity tests (tests/test_gpu_*.py); not used by renderers ---- */
/* resd + sdf MLPs on given big-pose points: resd n x 3, sdf n, feat n x 256 (any may be NULL) */
/* the current frame's key lights (ra_config.key_light_share): n_lights flags and every light's largest share of a probe's power */
int ra_debug_key_lights(ra_ctx* ctx, unsigned char* key_dev, float* share_dev, void* stream);
int ra_debug_mlp(ra_ctx* ctx, const float* bpts_dev, int n, float* resd, float* sdf, float* feat, void* stream);
/* full kernel with identity warp: d sdf/d bpts n x 3, sdf n, feat n x 256, raw n x C */
int ra_debug_full(ra_ctx* ctx, const float* bpts_dev, int n, float* grad, float* sdf, float* feat, float* raw, void* stream);
/* the vertex ids of the current frame's box structure in leaf order (32 per leaf; the padding of the last leaf is 0x7fffffff) to a HOST array
 * of `capacity` ints; *n_out = 32 x leaves (0 without a structure: brute-force mode or a mesh beyond its limit).  Synchronises the stream. */
int ra_debug_bvh_ids(ra_ctx* ctx, int* ids_host, int capacity, int* n_out, void* stream);
/* coarse level: per-point coarse sdf n, sdf_batch n x 3, nn_batch n x 3 (int32), filtered d2 n x 3, and for fine points
 * bpts/tpts n x 3, blended (A|big_A) rows n x 24 (zeros elsewhere); fine_count_host receives the count (synchronises) */
int ra_debug_hdq(ra_ctx* ctx, const float* x_dev, int n, float dist_th, float* sdf_coarse, float* sdf_batch, int* nn_batch,
                 float* d2, float* bpts, float* tpts, float* mats, int* fine_count_host, void* stream);

/* get_near_far_aabb (net_utils.py:1683-1712, return_raw) on n rays: the slab test the shadow-ray generator runs inline */
int ra_debug_aabb(ra_ctx* ctx, const float* o_dev, const float* d_dev, int n, const float* bbox_host6, float* near_dev, float* far_dev, void* stream);
/* light_visibility (sphere_tracing_renderer.py:265-344) for n surface points: surf, norm n x 3, acc n -> lvis, ldot n x 512 */
int ra_debug_lvis(ra_ctx* ctx, const float* surf_dev, const float* norm_dev, const float* acc_dev, int n, const float* bbox_host6,
                  const ra_trace_params* shadow, float near_offset, float* lvis_dev, float* ldot_dev, void* stream);
/* Microfacet.__call__ (relight_utils.py:484-577): pts2l L x N x 3, pts2c / normal / albedo N x 3, rough N -> brdf L x N x 3 */
int ra_debug_brdf(ra_ctx* ctx, const float* p2l_dev, const float* p2c_dev, const float* normal_dev, const float* albedo_dev,
                  const float* rough_dev, int L, int N, float* brdf_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELIGHTABLEAVATAR_H */

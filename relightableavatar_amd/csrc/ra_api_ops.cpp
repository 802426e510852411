// C ABI: the stateless and thin entry points (include/relightableavatar.h) — re-shading, the material heads and regularisers, the
// per-frame body state, ray generation, images, metrics, LPIPS and the row gathers.  Each checks its arguments and enqueues a kernel
// or two; the render hot path is ra_api.cpp.
#include "ra_api_impl.hpp"
#include "ra_mcubes.hpp"
#include "ra_mcubes_grad_rules.hpp"
#include "ra_topo_rules.hpp"
#include "ra_fit_rules.hpp"
#include "ra_cloth_rules.hpp"
#include "ra_raster_rules.hpp"
#include "ra_antialias.hpp"
#include "ra_texture.hpp"
#include "ra_mesh_grad.hpp"
#include <cmath>
#include <cstring>

// the weights of a relight context, its device current (no frame needed); who: the entry point, for the message
static int relight_ready(ra_ctx* c, const char* who) {
    if (!(c && c->have_weights && c->cfg.relight)) { ra_set_error(std::string(who) + ": needs a relight ctx with weights"); return 1; }
    if (hipSetDevice(c->device) != hipSuccess) { ra_set_error(std::string(who) + ": hipSetDevice failed"); return 1; }
    return 0;
}

// ra_reshade's configuration (the forward and its backward)
static ra_config reshade_config(const ra_ctx* c) {
    ra_config cfg = c->cfg;
    cfg.tonemapping = 1;      // novel_light_sphere_tracing.py:47 applies linear2srgb unconditionally
    cfg.only_visibility = 0;  // ... and knows none of render_human's debugging switches (:21-66): it shades with the cosines and probes it is given
    cfg.vis_shade_map = 0;
    return cfg;
}

// the image pair of ra_image_metrics / ra_lpips; w: the entry point, for the message
static int check_image_pair(const std::string& w, const ra_metrics_params* p, const float* pred, const float* gt, const long long* pix, int P,
                            const unsigned char* mask, const double* out) {
    RA_CHECK(p->H >= 1 && p->W >= 1 && (long long)p->H * p->W < (1ll << 30) && P >= 0 && P <= (long long)p->H * p->W, w + ": bad sizes");
    RA_CHECK(P == 0 || (pred && gt), w + ": null argument (pred, gt)");
    RA_CHECK(pix || P == p->H * p->W, w + ": without pixel indices the maps must hold all H*W pixels");
    RA_CHECK(!p->crop_to_mask || mask, w + ": crop_to_mask needs the mask");
    RA_CHECK(((uintptr_t)out & 7) == 0, w + ": bad alignment of out (doubles)");
    return 0;
}

extern "C" {

int ra_gather_rays(int device, const long long* idx, int n, const float* ray_o, const float* ray_d, const float* near_, const float* far_,
                   float* out_o, float* out_d, float* out_near, float* out_far, void* stream) {
    RA_CHECK(n >= 0 && (n == 0 || (idx && ray_o && ray_d && near_ && far_ && out_o && out_d && out_near && out_far)), "ra_gather_rays: bad arguments");
    RA_HIP(hipSetDevice(device));
    launch_gather_shard_rays(idx, n, ray_o, ray_d, near_, far_, out_o, out_d, out_near, out_far, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_scatter_rows(int device, const float* src, const long long* src_idx, const long long* dst_idx, long long n, int C, float* dst, void* stream) {
    RA_CHECK(n >= 0 && C > 0 && (n == 0 || (src && src_idx && dst_idx && dst)) && n * C < (1ll << 40), "ra_scatter_rows: bad arguments");
    RA_HIP(hipSetDevice(device));
    launch_scatter_rows(src, src_idx, dst_idx, n, C, dst, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_blend_ground(ra_ctx* c, const float* ground, const float* human, const long long* inds, const float* acc, int F, int P, int C,
                    float* dst, void* stream) {
    RA_CHECK(c, "ra_blend_ground: null ctx");
    RA_CHECK(acc && dst && F >= 0 && P >= 0 && C > 0 && (!human || inds), "ra_blend_ground: bad arguments");
    RA_HIP(hipSetDevice(c->device));
    launch_blend_ground(ground, human, inds, acc, F, P, C, dst, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}
int ra_reshade(ra_ctx* c, const float* ray_o, const float* surf, const float* norm, const float* albedo, const float* roughness,
               const float* lvis, const float* ldot, int P, const float* probes, int n_probes, int ph, int pw, float* rgb,
               float* shade, float* spec, void* stream) {
    if (relight_ready(c, "ra_reshade")) return 1;
    RA_CHECK(P >= 0 && n_probes >= 0, "ra_reshade: bad sizes");
    if (P == 0 || n_probes == 0) return 0;
    RA_CHECK(ray_o && surf && norm && albedo && roughness && lvis && ldot && probes, "ra_reshade: null input");
    hipStream_t s = (hipStream_t)stream;
    const ra_config cfg = reshade_config(c);
    for (int q0 = 0; q0 < n_probes; q0 += 8) {
        const int nq = n_probes - q0 < 8 ? n_probes - q0 : 8;
        ShadeIn in{};
        in.ray_o = ray_o; in.surf = surf; in.idx = nullptr; in.count = nullptr; in.n = P;
        in.norm = norm; in.albedo = albedo; in.rough = roughness; in.lvis = lvis; in.ldot = ldot;
        in.light_xyz = c->light_xyz.as<float>(); in.light_area = c->light_area.as<float>(); in.L = c->n_lights;
        in.probes = probes + (size_t)q0 * ph * pw * 3; in.n_probes = nq; in.ph = ph; in.pw = pw; in.want_spec = spec != nullptr;
        in.rgb = rgb ? rgb + (size_t)q0 * P * 3 : nullptr;
        in.shade = shade ? shade + (size_t)q0 * P * 3 : nullptr;
        in.spec = spec ? spec + (size_t)q0 * P * 3 : nullptr;
        launch_shade(in, cfg, s);
    }
    c->n_shaded += (uint64_t)P * n_probes;
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_reshade_backward(ra_ctx* c, const float* ray_o, const float* surf, const float* norm, const float* albedo, const float* roughness,
                        const float* lvis, const float* ldot, int P, const float* probes, int n_probes, int ph, int pw,
                        const float* d_rgb, float* d_albedo, float* d_roughness, float* d_probes, void* stream) {
    if (relight_ready(c, "ra_reshade_backward")) return 1;
    RA_CHECK(P >= 0 && n_probes >= 0, "ra_reshade_backward: bad sizes");
    if (P == 0 || n_probes == 0) return 0;
    RA_CHECK(ray_o && surf && norm && albedo && roughness && lvis && ldot && probes && d_rgb, "ra_reshade_backward: null input");
    RA_CHECK(ph > 0 && pw > 0 && shade_bwd_probes_per_launch(ph, pw) >= 1, "ra_reshade_backward: the probe does not fit the kernel's LDS tile (h * w <= 5461)");
    hipStream_t s = (hipStream_t)stream;
    ShadeBwd a{};
    a.ray_o = ray_o; a.surf = surf; a.norm = norm; a.albedo = albedo; a.rough = roughness; a.lvis = lvis;      // ldot: cancel_cosine, rgb does not read it
    a.light_xyz = c->light_xyz.as<float>(); a.light_area = c->light_area.as<float>(); a.L = c->n_lights;
    a.probes = probes; a.n_probes = n_probes; a.ph = ph; a.pw = pw; a.d_rgb = d_rgb; a.P = P;
    a.d_albedo = d_albedo; a.d_rough = d_roughness; a.d_probes = d_probes;
    if (d_probes) {      // one partial slab per workgroup: grown on the first call of a size, reused afterwards
        int err = 0;
        const int per = shade_bwd_probes_per_launch(ph, pw);
        a.slabs = c->buf<float>("rsb_slabs", (size_t)shade_bwd_grid(P) * (per < n_probes ? per : n_probes) * ph * pw * 3, &err);
        if (err) return 1;
    }
    launch_shade_bwd(a, reshade_config(c), s);
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- the material heads on cached features (ra_heads.hip) ----------------------------------------
size_t ra_heads_param_count(const ra_ctx*) { return HEADS_PARAMS; }

int ra_heads_get_params(ra_ctx* c, float* theta, void* stream) {
    if (relight_ready(c, "ra_heads_get_params")) return 1;
    RA_CHECK(theta, "ra_heads_get_params: null input");
    std::vector<float>& t = c->heads_theta;
    t.clear();
    for (const char* net : {"albedo_network", "roughness_network"})
        for (int l = 0; l < 3; ++l)
            for (const char* kind : {"weight", "bias"}) {
                const std::string key = std::string(net) + ".linears." + std::to_string(l) + "." + kind;
                auto it = c->state_dict.find(key);
                RA_CHECK(it != c->state_dict.end(), "ra_heads_get_params: missing " + key);
                t.insert(t.end(), it->second.begin(), it->second.end());
            }
    RA_CHECK(t.size() == (size_t)HEADS_PARAMS, "ra_heads_get_params: the loaded heads are not 256 -> 128 -> 128 -> {3, 1}");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipMemcpyAsync(theta, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, s));
    RA_HIP(hipStreamSynchronize(s));      // the staging vector may be rebuilt by the next call
    return 0;
}

int ra_heads_forward(ra_ctx* c, const float* theta, const float* feat, int n, float* albedo, float* rough, void* stream) {
    if (relight_ready(c, "ra_heads_forward")) return 1;
    RA_CHECK(n >= 0, "ra_heads_forward: bad sizes");
    if (n == 0) return 0;
    RA_CHECK(theta && feat, "ra_heads_forward: null input");
    int err = 0;
    HeadsIO io{};
    io.theta = theta; io.feat = feat; io.n = n; io.albedo = albedo; io.rough = rough;
    io.w16 = c->buf<char>("heads_w16", HEADS_W16_BYTES, &err);
    if (err) return 1;
    launch_heads_forward(io, c->cfg, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_heads_backward(ra_ctx* c, const float* theta, const float* feat, int n, const float* d_albedo, const float* d_rough, float* d_theta,
                      void* stream) {
    if (relight_ready(c, "ra_heads_backward")) return 1;
    RA_CHECK(n >= 0, "ra_heads_backward: bad sizes");
    if (n == 0) return 0;
    RA_CHECK(theta && feat && d_theta, "ra_heads_backward: null input");
    int err = 0;
    HeadsIO io{};
    io.theta = theta; io.feat = feat; io.n = n; io.d_albedo = d_albedo; io.d_rough = d_rough; io.d_theta = d_theta;
    const int held = n < HEADS_CHUNK ? n : HEADS_CHUNK;
    io.w16 = c->buf<char>("heads_w16", HEADS_W16_BYTES, &err);
    io.amax = c->buf<unsigned>("heads_amax", 2, &err);
    io.tape = c->buf<char>("heads_tape", (size_t)((held + 63) / 64) * HEADS_TAPE_BYTES_PER_TILE, &err);
    io.slabs = c->buf<float>("heads_slabs", (size_t)heads_grid(n) * HEADS_PARAMS, &err);
    if (err) return 1;
    launch_heads_backward(io, c->cfg, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_bigpose_features(ra_ctx* c, const float* bpts, int n, float* feat, void* stream) {
    if (check_ready(c, "ra_bigpose_features")) return 1;
    RA_CHECK(c->cfg.relight, "ra_bigpose_features: needs a relight ctx with weights");
    RA_CHECK(n >= 0, "ra_bigpose_features: bad sizes");
    if (n == 0) return 0;
    RA_CHECK(bpts && feat, "ra_bigpose_features: null input");
    return ra_debug_mlp(c, bpts, n, nullptr, nullptr, feat, stream);
}

// ---- the regularisers of the relighting stage (ra_k4_canon.hpp, ra_entropy.hip) -------------------
int ra_canonical_features(ra_ctx* c, const float* cpts, int n, float* feat, void* stream) {
    if (relight_ready(c, "ra_canonical_features")) return 1;      // weights of a relight ctx; no frame: the SDF net has no pose condition
    RA_CHECK(n >= 0, "ra_canonical_features: bad sizes");
    if (n == 0) return 0;
    RA_CHECK(cpts && feat, "ra_canonical_features: null input");
    RA_CHECK(c->host.fwd_arena.size() == (size_t)2080 * 512, "ra_canonical_features: the forward stream is not the 2080 fragments the kernel walks");
    hipStream_t s = (hipStream_t)stream;
    if (c->cfg.mlp_f16) launch_canonical_features_f16(c->host.geo, c->fwd_arena.p, c->barena.as<float>(), cpts, n, feat, s);
    else launch_canonical_features_bf16(c->host.geo, c->fwd_arena.p, c->barena.as<float>(), cpts, n, feat, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_gaussian_entropy(ra_ctx* c, const float* x, int n, const float* d_value, float* value, float* d_x, void* stream) {
    RA_CHECK(c, "ra_gaussian_entropy: null ctx");
    RA_CHECK(x && value, "ra_gaussian_entropy: null input");
    RA_CHECK(n >= 2, "ra_gaussian_entropy: bad sizes (the variance needs two rows)");
    RA_HIP(hipSetDevice(c->device));
    int err = 0;
    double* scratch = c->buf<double>("entropy", entropy_scratch_doubles(n), &err);
    if (err) return 1;
    launch_gaussian_entropy(x, n, d_value, value, d_x, scratch, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_reshade_ground(ra_ctx* c, const float* ray_d, const float* albedo_map, const float* lvis, const float* ldot, int P,
                      const float* probes, int n_probes, int ph, int pw, const float* images, int ih, int iw, int attach_envmap,
                      float* rgb, float* albedo, float* shade, float* spec, void* stream) {
    if (relight_ready(c, "ra_reshade_ground")) return 1;
    RA_CHECK(P >= 0 && n_probes >= 0, "ra_reshade_ground: bad sizes");
    if (P == 0 || n_probes == 0) return 0;
    RA_CHECK(ray_d && lvis && ldot && probes && ph > 0 && pw > 0, "ra_reshade_ground: null input");
    RA_CHECK(attach_envmap || albedo_map, "ra_reshade_ground: albedo_map is needed when the probe is not attached to the ground");
    RA_CHECK(!images || (ih > 0 && iw > 0), "ra_reshade_ground: bad image size");
    GroundReshade in{};
    in.ray_d = ray_d; in.albedo_map = albedo_map; in.lvis = lvis; in.ldot = ldot;
    in.ldir = c->light_dir.as<float>(); in.light_area = c->light_area.as<float>(); in.L = c->n_lights;
    in.probes = probes; in.n_probes = n_probes; in.ph = ph; in.pw = pw; in.images = images; in.ih = ih; in.iw = iw;
    in.attach_envmap = attach_envmap; in.P = P;
    in.rgb = rgb; in.albedo = albedo; in.shade = shade; in.spec = spec;
    launch_ground_reshade(in, (hipStream_t)stream);
    c->n_shaded += (uint64_t)P * n_probes;
    RA_HIP(hipGetLastError());
    return 0;
}
// pinned staging ring of the context (ra_ctx.hpp PinRing)
static char* pin_acquire(ra_ctx* c, size_t bytes, int* slot) {
    PinRing& r = c->pin;
    if (bytes > r.slot_bytes) {
        if (r.base) {
            for (int k = 0; k < PinRing::n; ++k) if (r.used[k]) { hipEventSynchronize(r.ev[k]); r.used[k] = false; }
            hipHostFree(r.base);
            r.base = nullptr;
        }
        const size_t sb = (bytes + 4095) & ~(size_t)4095;
        if (hipHostMalloc((void**)&r.base, sb * PinRing::n, hipHostMallocDefault) != hipSuccess) { r.base = nullptr; r.slot_bytes = 0; return nullptr; }
        r.slot_bytes = sb;
        for (int k = 0; k < PinRing::n; ++k) if (!r.ev[k]) hipEventCreateWithFlags(&r.ev[k], hipEventDisableTiming);
    }
    const int k = r.next;
    r.next = (k + 1) % PinRing::n;
    if (r.used[k]) hipEventSynchronize(r.ev[k]);        // only when the host is PinRing::n frames ahead of this stream
    *slot = k;
    return r.base + (size_t)k * r.slot_bytes;
}
static void pin_release(ra_ctx* c, int slot, hipStream_t s) {
    hipEventRecord(c->pin.ev[slot], s);
    c->pin.used[slot] = true;
}

int ra_pose_frame(ra_ctx* c, const ra_pose_in* in, const ra_pose_out* out, void* stream) {
    RA_CHECK(c && in && out, "ra_pose_frame: null argument");
    const int J = in->n_bones, N = in->n_verts, F = in->n_faces;
    RA_CHECK(J > 0 && J <= 256 && N > 0 && F >= 0, "ra_pose_frame: bad sizes");
    RA_CHECK(in->poses && in->tjoints && in->parents && in->big_A && in->Rh && in->Th && in->tverts && in->weights, "ra_pose_frame: null input");
    RA_CHECK(!out->pnorm || (in->faces && F > 0), "ra_pose_frame: vertex normals need faces");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    for (int j = 1; j < J; ++j) RA_CHECK(in->parents[j] >= 0 && in->parents[j] < j, "ra_pose_frame: parents must be in topological order");
    // ---- the frame's small host inputs: ONE pinned block, ONE asynchronous upload; the bone transforms themselves (52 Rodrigues
    // rotations + the chain of 4 x 4 products, float64) run on the device behind it.  Nothing here waits for the stream: with frames
    // in flight an animated sequence poses frame f + 1 while frame f renders (round 3 computed the chain on the host and ended in a
    // hipStreamSynchronize: a full host stall per animated frame).
    const size_t n_in = (size_t)J * (3 + 3 + 16 + 1) + 6;
    int err = 0;
    float* dIn = c->buf<float>("pf_in", n_in, &err);
    float* dA = c->buf<float>("pf_A", (size_t)J * 16, &err);
    float* dJ = c->buf<float>("pf_J", (size_t)J * 3, &err);
    float* dR = c->buf<float>("pf_R", 12, &err);
    float* dP = c->buf<float>("pf_p", (size_t)N * 3, &err);
    float* dW = c->buf<float>("pf_w", (size_t)N * 3, &err);
    RA_CHECK(!err, "ra_pose_frame: out of device memory");
    {
        int slot = 0;
        float* st = reinterpret_cast<float*>(pin_acquire(c, n_in * sizeof(float), &slot));
        RA_CHECK(st, "ra_pose_frame: no pinned host memory for the staging ring");
        std::memcpy(st, in->poses, (size_t)J * 12);
        std::memcpy(st + 3 * J, in->tjoints, (size_t)J * 12);
        std::memcpy(st + 6 * J, in->big_A, (size_t)J * 64);
        std::memcpy(st + 22 * J, in->Rh, 12);
        std::memcpy(st + 22 * J + 3, in->Th, 12);
        std::memcpy(st + 22 * J + 6, in->parents, (size_t)J * 4);
        RA_HIP(hipMemcpyAsync(dIn, st, n_in * sizeof(float), hipMemcpyHostToDevice, s));
        pin_release(c, slot, s);
    }
    launch_bone_transforms(dIn, J, dA, dJ, dR, s);
    const float* dB = dIn + 6 * J;             // big_A as uploaded
    float* pv = out->pverts ? (float*)out->pverts : dP;
    float* wv = out->wverts ? (float*)out->wverts : dW;
    launch_lbs_verts((const float*)in->tverts, (const float*)in->weights, dA, dB, dR, dR + 9, N, J, (float*)out->tpose, pv, wv, s);
    if (out->pnorm) {
        // incident corners per vertex in index_add order, cached per (faces pointer, count)
        // the cache key is the CONTENT of the face array (a multiply-xorshift mix over 8-byte words, four independent lanes: ~10 us for
        // SMPL's 13 776 faces; FNV-1a byte by byte took 40 us of host time per frame)
        unsigned long long fh = 1469598103934665603ull ^ (unsigned long long)F;
        {
            const size_t nw = (size_t)F * 3 / 2;
            unsigned long long lane[4] = {0x9e3779b97f4a7c15ull, 0xc2b2ae3d27d4eb4full, 0x165667b19e3779f9ull, 0x27d4eb2f165667c5ull};
            size_t k = 0;
            for (; k + 4 <= nw; k += 4)
                for (int l = 0; l < 4; ++l) {
                    unsigned long long w;
                    std::memcpy(&w, reinterpret_cast<const char*>(in->faces) + (k + l) * 8, 8);
                    lane[l] = (lane[l] ^ w) * 0x100000001b3ull;
                    lane[l] ^= lane[l] >> 29;
                }
            for (; k < nw; ++k) {
                unsigned long long w;
                std::memcpy(&w, reinterpret_cast<const char*>(in->faces) + k * 8, 8);
                lane[0] = (lane[0] ^ w) * 0x100000001b3ull;
                lane[0] ^= lane[0] >> 29;
            }
            if ((size_t)F * 3 % 2) lane[1] = (lane[1] ^ (unsigned)in->faces[3 * F - 1]) * 0x100000001b3ull;
            for (int l = 0; l < 4; ++l) { fh = (fh ^ lane[l]) * 1099511628211ull; fh ^= fh >> 31; }
        }
        if (c->adj_hash != fh || c->adj_n_faces != F || c->adj_n_verts != N) {
            std::vector<int> start(N + 1, 0), adj((size_t)F * 3);
            const int order[3] = {1, 2, 0};
            for (int f = 0; f < F; ++f)
                for (int k = 0; k < 3; ++k) {
                    const int v = in->faces[3 * f + k];
                    RA_CHECK(v >= 0 && v < N, "ra_pose_frame: face index out of range");
                    ++start[v + 1];
                }
            for (int v = 0; v < N; ++v) start[v + 1] += start[v];
            std::vector<int> fill(start.begin(), start.end() - 1);
            for (int pass = 0; pass < 3; ++pass)
                for (int f = 0; f < F; ++f) { const int corner = order[pass]; adj[fill[in->faces[3 * f + corner]]++] = (f << 2) | corner; }
            // a new mesh (rare): a vert_normals launch of an earlier frame may still be queued on s (frames-in-flight streams are
            // non-blocking: not ordered against the null stream the copies below run on) and would read a half-overwritten list
            RA_HIP(hipStreamSynchronize(s));
            if (c->adj_start.ensure((size_t)(N + 1) * 4) || c->adj_list.ensure((size_t)F * 12 + 4) || c->adj_dfaces.ensure((size_t)F * 12 + 4)) return 1;
            RA_HIP(hipMemcpy(c->adj_start.p, start.data(), (size_t)(N + 1) * 4, hipMemcpyHostToDevice));
            RA_HIP(hipMemcpy(c->adj_list.p, adj.data(), (size_t)F * 12, hipMemcpyHostToDevice));
            RA_HIP(hipMemcpy(c->adj_dfaces.p, in->faces, (size_t)F * 12, hipMemcpyHostToDevice));
            c->adj_hash = fh; c->adj_n_faces = F; c->adj_n_verts = N;
        }
        launch_vert_normals(pv, c->adj_dfaces.as<int>(), c->adj_start.as<int>(), c->adj_list.as<int>(), N, (float*)out->pnorm, s);
    }
    if (out->pbounds) launch_bounds(pv, N, in->bounds_padding, (float*)out->pbounds, s);
    if (out->wbounds) launch_bounds(wv, N, in->bounds_padding, (float*)out->wbounds, s);
    if (out->A) RA_HIP(hipMemcpyAsync(out->A, dA, (size_t)J * 64, hipMemcpyDeviceToDevice, s));
    if (out->R) RA_HIP(hipMemcpyAsync(out->R, dR, 36, hipMemcpyDeviceToDevice, s));
    if (out->joints) RA_HIP(hipMemcpyAsync(out->joints, dJ, (size_t)J * 12, hipMemcpyDeviceToDevice, s));
    if (out->poses) RA_HIP(hipMemcpyAsync(out->poses, dIn, (size_t)J * 12, hipMemcpyDeviceToDevice, s));
    if (out->Th) RA_HIP(hipMemcpyAsync(out->Th, dIn + 22 * J + 3, 12, hipMemcpyDeviceToDevice, s));
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_grow_bounds(ra_ctx* c, float* wbounds, float margin, void* stream) {
    RA_CHECK(c && wbounds, "ra_grow_bounds: null argument");
    RA_HIP(hipSetDevice(c->device));
    launch_grow_bounds(wbounds, margin, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_shift_envmap(ra_ctx* c, const float* img, int H, int W, int C, float shift, float* out, void* stream) {
    RA_CHECK(c, "ra_shift_envmap: null ctx");
    RA_CHECK(img && out && H > 0 && W > 0 && C > 0 && img != out, "ra_shift_envmap: bad arguments");
    RA_HIP(hipSetDevice(c->device));
    launch_shift_envmap(img, H, W, C, shift, out, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_add_light_probe(ra_ctx* c, float* rgb, int H, int W, const float* probe, int ph, int pw, const float* cam_R, int uH, int uW,
                       void* stream) {
    RA_CHECK(c, "ra_add_light_probe: null ctx");
    RA_CHECK(rgb && probe && cam_R && H > 0 && W > 0 && ph > 0 && pw > 0, "ra_add_light_probe: bad arguments");
    RA_CHECK(uH >= 0 && uW >= 0 && uH <= H && uW <= W, "ra_add_light_probe: the inset does not fit the image");
    RA_HIP(hipSetDevice(c->device));
    // gen_light_dir (relight_utils.py:9-30): camera axes (columns of R^T) with only the horizontal heading kept
    const double front0[3] = {cam_R[6], cam_R[7], cam_R[8]};             // third row of the w2c rotation = camera z in the world
    const double downz = cam_R[5] > 0 ? 1.0 : (cam_R[5] < 0 ? -1.0 : 0.0);   // sign of (camera y).z
    const double down[3] = {0.0, 0.0, downz};
    auto cross = [](const double* a, const double* b, double* o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; };
    auto norml = [](double* v) { const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + 1e-8; v[0] /= n; v[1] /= n; v[2] /= n; };
    double right[3], front[3];
    cross(down, front0, right); norml(right);
    cross(right, down, front); norml(front);
    ProbeInset p{};
    for (int r = 0; r < 3; ++r) { p.axes[3 * r] = (float)right[r]; p.axes[3 * r + 1] = (float)-front[r]; p.axes[3 * r + 2] = (float)-down[r]; }
    p.H = H; p.W = W; p.uH = uH; p.uW = uW; p.ph = ph; p.pw = pw;
    launch_light_probe(p, probe, rgb, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_map_to_image(ra_ctx* c, const ra_image_params* p, const float* a, const float* b, const float* acc, const long long* pix, int P,
                    float* image, float* alpha, void* stream) {
    RA_CHECK(c && p && image, "ra_map_to_image: null argument");
    RA_CHECK(p->H > 0 && p->W > 0 && P >= 0 && (long long)p->H * p->W < (1ll << 30), "ra_map_to_image: bad sizes");
    RA_CHECK(p->type >= RA_IMG_SURFACE && p->type <= RA_IMG_RENDERING, "ra_map_to_image: unknown output type");
    RA_CHECK(P == 0 || a || p->type == RA_IMG_ALPHA, "ra_map_to_image: the map is missing");
    RA_CHECK(pix || P == p->H * p->W || P == 0, "ra_map_to_image: without pixel indices the maps must be full-frame");
    RA_CHECK(p->type != RA_IMG_RESIDUAL || b, "ra_map_to_image: Residual needs cpts_map and bpts_map");
    RA_CHECK((p->type != RA_IMG_SURFACE && p->type != RA_IMG_NORMAL && p->type != RA_IMG_ALPHA && p->type != RA_IMG_DEPTH) || acc || P == 0,
             "ra_map_to_image: this type needs acc_map");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    int err = 0;
    float* stats = c->buf<float>("im_stats", 4, &err);
    const bool pct_all = p->type == RA_IMG_RESIDUAL || ((p->type == RA_IMG_SHADING || p->type == RA_IMG_SPECULAR) && p->normalize);
    if (P > 0 && (pct_all || p->type == RA_IMG_DEPTH)) {
        const long long n = pct_all ? 3ll * P : P;
        const int k = (int)((pct_all ? 0.005 : 0.01) * (double)n);                    // int(percentile * depth_map.numel())
        RA_CHECK(k >= 1, "ra_map_to_image: too few rays for the percentile (the reference's topk(0).max() fails too)");
        const size_t tb = image_sort_temp_bytes(n);
        float* sa = c->buf<float>("im_sa", n, &err);
        float* sb = c->buf<float>("im_sb", n, &err);
        unsigned char* flag = c->buf<unsigned char>("im_flag", n, &err);
        char* tmp = c->buf<char>("im_tmp", tb + 16, &err);
        RA_CHECK(!err, "ra_map_to_image: out of device memory");
        const float* vals = a;
        if (p->type == RA_IMG_RESIDUAL) { launch_diff(a, b, n, sa, s); vals = sa; sa = c->buf<float>("im_sc", n, &err); RA_CHECK(!err, "ra_map_to_image: out of device memory"); }
        RA_CHECK(launch_percentiles(vals, n, p->type == RA_IMG_DEPTH ? acc : nullptr, k, sa, sb, flag, icnt(c, CNT_SAMP), tmp, tb, stats, s) == 0,
                 "ra_map_to_image: device sort failed");
    }
    RA_CHECK(!err, "ra_map_to_image: out of device memory");
    ImageJob j{};
    j.type = p->type; j.P = P; j.a = a; j.b = b; j.acc = acc; j.pix = pix; j.stats = stats;
    for (int k = 0; k < 9; ++k) j.cam_R[k] = p->cam_R[k];
    for (int k = 0; k < 6; ++k) j.tbounds[k] = p->tbounds[k];
    j.min_clip = p->min_clip; j.bg = p->bg_brightness; j.normalize = p->normalize; j.tonemap = p->tonemap;
    j.image = image; j.alpha = alpha;
    launch_compose_image(j, (long long)p->H * p->W, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_image_metrics(ra_ctx* c, const ra_metrics_params* p, const float* pred, const float* gt, const long long* pix, int P,
                     const unsigned char* mask, double* out, void* stream) {
    RA_CHECK(c && p && out, "ra_image_metrics: null argument");
    if (check_image_pair("ra_image_metrics", p, pred, gt, pix, P, mask, out)) return 1;
    RA_HIP(hipSetDevice(c->device));
    int err = 0;
    char* scratch = c->buf<char>("metrics", metrics_scratch_bytes(p->H, p->W, pix != nullptr), &err);
    RA_CHECK(!err, "ra_image_metrics: out of device memory");
    MetricsIO io{};
    io.pred = pred; io.gt = gt; io.pix = pix; io.P = P; io.mask = mask; io.H = p->H; io.W = p->W;
    io.bg = p->bg_brightness; io.data_range = p->data_range; io.mse_over_rays = p->mse_over_rays; io.crop_to_mask = p->crop_to_mask;
    io.out = out; io.scratch = scratch;
    launch_image_metrics(io, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_lpips_tile_m(void) { return LPIPS_BM; }

int ra_lpips_loaded(ra_ctx* c) { return c && c->lpips_loaded ? 1 : 0; }

int ra_lpips_load(ra_ctx* c, const ra_lpips_weights* w, void* stream) {
    RA_CHECK(c && w, "ra_lpips_load: null argument");
    for (int k = 0; k < LPIPS_TAPS; ++k) RA_CHECK(w->conv_w[k] && w->conv_b[k] && w->lin[k], "ra_lpips_load: null argument (a weight pointer)");
    for (int ch = 0; ch < 3; ++ch) RA_CHECK(w->scale[ch] != 0.f, "ra_lpips_load: a zero scale");
    const LpipsArena a = lpips_arena();
    std::vector<float>& h = c->lpips_host;
    h.assign(a.total, 0.f);
    for (int k = 0; k < LPIPS_TAPS; ++k) {
        lpips_pack_conv(LPIPS_LAYERS[k], w->conv_w[k], h.data() + a.conv[k]);
        std::copy(w->conv_b[k], w->conv_b[k] + LPIPS_LAYERS[k].cout, h.data() + a.bias[k]);
        std::copy(w->lin[k], w->lin[k] + LPIPS_LAYERS[k].cout, h.data() + a.lin[k]);
    }
    std::copy(w->shift, w->shift + 3, h.data() + a.shift);
    std::copy(w->scale, w->scale + 3, h.data() + a.scale);
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    RA_CHECK(!c->lpips_arena.ensure(a.total * sizeof(float)), "ra_lpips_load: out of device memory");
    RA_HIP(hipMemcpyAsync(c->lpips_arena.p, h.data(), a.total * sizeof(float), hipMemcpyHostToDevice, s));     // behind the calls that read the old set
    RA_HIP(hipStreamSynchronize(s));      // the staging vector may be rebuilt by the next call
    c->lpips_loaded = true;
    return 0;
}

int ra_lpips(ra_ctx* c, const ra_metrics_params* p, const float* pred, const float* gt, const long long* pix, int P, const unsigned char* mask,
             double* out, void* stream) {
    RA_CHECK(p && out, "ra_lpips: null argument");
    RA_CHECK(ra_lpips_loaded(c), "ra_lpips: lpips weights not loaded");      // a null ctx holds none
    if (check_image_pair("ra_lpips", p, pred, gt, pix, P, mask, out)) return 1;
    RA_HIP(hipSetDevice(c->device));
    int err = 0;
    char* scratch = c->buf<char>("lpips", lpips_scratch_bytes(p->H, p->W, pix != nullptr), &err);
    RA_CHECK(!err, "ra_lpips: out of device memory");
    LpipsIO io{};
    io.pred = pred; io.gt = gt; io.pix = pix; io.P = P; io.mask = mask; io.H = p->H; io.W = p->W;
    io.bg = p->bg_brightness; io.crop_to_mask = p->crop_to_mask; io.out = out; io.scratch = scratch;
    io.arena = c->lpips_arena.as<float>(); io.off = lpips_arena();
    launch_lpips(io, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_lpips_features(ra_ctx* c, const float* img, int H, int W, int tap, float* out, void* stream) {
    RA_CHECK(img && out, "ra_lpips_features: null argument");
    RA_CHECK(ra_lpips_loaded(c), "ra_lpips_features: lpips weights not loaded");
    RA_CHECK(H >= LPIPS_MIN_SIDE && W >= LPIPS_MIN_SIDE && (long long)H * W < (1ll << 30) && tap >= 0 && tap < LPIPS_TAPS,
             "ra_lpips_features: bad sizes (an image below 31 x 31 has no features; tap 0..4)");
    RA_HIP(hipSetDevice(c->device));
    int err = 0;
    char* scratch = c->buf<char>("lpips", lpips_scratch_bytes(H, W, false), &err);
    RA_CHECK(!err, "ra_lpips_features: out of device memory");
    LpipsIO io{};
    io.pred = img; io.gt = img; io.P = H * W; io.H = H; io.W = W; io.scratch = scratch;
    io.arena = c->lpips_arena.as<float>(); io.off = lpips_arena();
    launch_lpips_features(io, tap, out, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- exact point-to-mesh distance (ra_mesh.hip) -------------------------------------------------
int ra_mesh_tile(int which) { return which == 0 ? MESH_LEAF : which == 1 ? MESH_FAN : which == 2 ? MESH_SORT_MIN : 0; }

// the scratch of a Morton sort of n items (a mesh build, the points of a query); grown on the first call of a size only
static int mesh_sort_scratch(ra_ctx* c, int n, MeshBuild* b) {
    int err = 0;
    b->temp_bytes = mesh_sort_temp_bytes(n);
    b->bb = c->buf<unsigned>("mesh_bb", 8, &err);
    b->keys = c->buf<unsigned>("mesh_keys", n, &err);
    b->keys_sorted = c->buf<unsigned>("mesh_keys_sorted", n, &err);
    b->vals = c->buf<int>("mesh_vals", n, &err);
    b->vals_sorted = c->buf<int>("mesh_vals_sorted", n, &err);
    b->temp = c->buf<char>("mesh_tmp", b->temp_bytes + 16, &err);
    return err;
}

static ra_mesh* find_mesh(ra_ctx* c, const ra_mesh* m) {
    for (auto& p : c->meshes) if (p.get() == m) return p.get();
    return nullptr;
}

int ra_mesh_create(ra_ctx* c, const float* verts, int n_verts, const int* faces, int n_faces, ra_mesh** out, void* stream) {
    RA_CHECK(c && out, "ra_mesh_create: null argument");
    RA_CHECK(n_verts >= 1 && n_faces >= 1 && n_faces <= MESH_MAX_FACES, "ra_mesh_create: bad sizes (n_verts >= 1, 1 <= n_faces <= 2^24)");
    RA_CHECK(verts && faces, "ra_mesh_create: null argument (verts, faces)");
    for (size_t k = 0; k < (size_t)n_faces * 3; ++k)
        RA_CHECK(faces[k] >= 0 && faces[k] < n_verts, "ra_mesh_create: face index outside [0, n_verts)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    std::unique_ptr<ra_mesh> m(new ra_mesh());
    m->faces.assign(faces, faces + (size_t)n_faces * 3);
    MeshView& v = m->view;
    v.n_faces = n_faces; v.n_leaves = mesh_leaf_count(n_faces); v.n_groups = mesh_group_count(v.n_leaves);
    MeshBuild b{};
    int err = mesh_sort_scratch(c, n_faces, &b);
    b.faces = c->buf<int>("mesh_faces", (size_t)n_faces * 3, &err);
    RA_CHECK(!err && !m->recs.ensure((size_t)v.n_leaves * MESH_LEAF * MESH_REC * 4) && !m->lbox.ensure((size_t)v.n_leaves * 24) && !m->gbox.ensure((size_t)v.n_groups * 24),
             "ra_mesh_create: out of device memory");
    v.recs = m->recs.as<float>(); v.lbox = m->lbox.as<float>(); v.gbox = m->gbox.as<float>();
    RA_HIP(hipMemcpyAsync(b.faces, m->faces.data(), (size_t)n_faces * 12, hipMemcpyHostToDevice, s));      // from the mesh's own copy
    RA_CHECK(launch_mesh_build(verts, b, v, m->recs.as<float>(), m->lbox.as<float>(), m->gbox.as<float>(), s) == 0, "ra_mesh_create: device sort failed");
    RA_HIP(hipGetLastError());
    *out = m.get();
    c->meshes.push_back(std::move(m));
    return 0;
}

int ra_mesh_destroy(ra_ctx* c, ra_mesh* mesh) {
    RA_CHECK(c, "ra_mesh_destroy: null argument");
    if (!mesh) return 0;
    RA_CHECK(find_mesh(c, mesh), "ra_mesh_destroy: not a mesh of this ctx");
    hipSetDevice(c->device);
    hipDeviceSynchronize();      // queries and the upload of its faces may still be queued
    for (auto it = c->meshes.begin(); it != c->meshes.end(); ++it)
        if (it->get() == mesh) { c->meshes.erase(it); break; }
    return 0;
}

int ra_mesh_closest(ra_ctx* c, const ra_mesh* mesh, const float* pts, int n, int flags, float* d2, float* closest, int* face, float* bary,
                    void* stream) {
    RA_CHECK(c && mesh, "ra_mesh_closest: null argument");
    RA_CHECK(find_mesh(c, mesh), "ra_mesh_closest: not a mesh of this ctx");
    RA_CHECK(n >= 0 && n < (1 << 30), "ra_mesh_closest: bad sizes");
    RA_CHECK((flags & ~(RA_MESH_BRUTE | RA_MESH_UNSORTED)) == 0, "ra_mesh_closest: unknown flag");
    if (n == 0) return 0;       // nothing to read or write: empty arrays have no address
    RA_CHECK(pts && (d2 || closest || face || bary), "ra_mesh_closest: null argument (pts, or all four outputs)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    MeshQuery q{};
    q.pts = pts; q.n = n; q.brute = (flags & RA_MESH_BRUTE) != 0; q.d2 = d2; q.closest = closest; q.face = face; q.bary = bary;
    // neighbours in space share a wave, so a wave opens little more than one lane would; the answers do not depend on it.  The
    // exhaustive scan opens everything anyway
    if (!q.brute && !(flags & RA_MESH_UNSORTED) && n > MESH_SORT_MIN) {
        MeshBuild b{};
        RA_CHECK(!mesh_sort_scratch(c, n, &b), "ra_mesh_closest: out of device memory");
        RA_CHECK(launch_mesh_sort_points(pts, n, b, s) == 0, "ra_mesh_closest: device sort failed");
        q.perm = b.vals_sorted;
    }
    launch_mesh_closest(mesh->view, q, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_mesh_closest_backward(ra_ctx* c, const int* faces, int n_faces, int n_verts, const float* pts, const float* closest, const int* face,
                             const float* bary, int n, const float* g_d2, const float* g_attr, int C, float* dpts, float* dverts, float* dattr,
                             void* stream) {
    RA_CHECK(n >= 0 && n < (1 << 30) && n_verts >= 1 && n_faces >= 1 && n_faces <= MESH_MAX_FACES && C >= 0 && C <= MESHG_MAX_C,
             "ra_mesh_closest_backward: bad sizes (0 <= n < 2^30, n_verts >= 1, 1 <= n_faces <= 2^24, 0 <= C <= 64)");
    RA_CHECK(c && (dpts || dverts || dattr), "ra_mesh_closest_backward: null argument (ctx, or all three outputs)");
    // n == 0: empty arrays have no address, so no row pointer is asked for or read
    RA_CHECK(n == 0 || ((g_d2 || !(dpts || dverts)) && (g_attr || !dattr || C == 0)),
             "ra_mesh_closest_backward: null argument (an output without its upstream gradient)");
    RA_CHECK(n == 0 || (faces && pts && closest && face && bary), "ra_mesh_closest_backward: null argument (faces, pts, closest, face, bary)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    MeshGradJob j{};
    j.faces = faces; j.pts = pts; j.closest = closest; j.face = face; j.bary = bary; j.g_d2 = g_d2; j.g_attr = g_attr;
    j.F = n_faces; j.V = n_verts; j.n = n; j.C = C; j.dpts = dpts; j.dverts = dverts; j.dattr = dattr;
    MeshGradScratch t{};
    if (n > 0 && (dverts || (dattr && C > 0))) {
        int err = 0;
        const size_t n_keys = 3 * (size_t)n;
        t.sort_bytes = mesh_grad_sort_bytes((long long)n_keys);
        t.select_bytes = mesh_grad_select_bytes((long long)n_keys);
        t.keys = c->buf<unsigned long long>("mesh_grad_keys", n_keys, &err);
        t.sorted = c->buf<unsigned long long>("mesh_grad_keys_sorted", n_keys, &err);
        t.flags = c->buf<unsigned char>("mesh_grad_flags", n_keys, &err);
        t.heads = c->buf<unsigned>("mesh_grad_heads", n_keys, &err);
        t.count = c->buf<unsigned>("mesh_grad_count", 4, &err);
        t.sort_temp = c->buf<char>("mesh_grad_sort_tmp", t.sort_bytes + 16, &err);
        t.select_temp = c->buf<char>("mesh_grad_select_tmp", t.select_bytes + 16, &err);
        RA_CHECK(!err, "ra_mesh_closest_backward: out of device memory");
    }
    RA_CHECK(launch_mesh_closest_backward(j, t, s) == 0, "ra_mesh_closest_backward: device sort failed");
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- generalised winding number (ra_winding.hip) --------------------------------------------------
int ra_winding_tile(int which) { return which == 0 ? WIND_BLOCK : which == 1 ? WIND_CHUNK : which == 2 ? WIND_SPLIT_TILES : 0; }

int ra_mesh_winding(ra_ctx* c, const ra_mesh* mesh, const float* pts, int n, int flags, float* winding, void* stream) {
    RA_CHECK(c && mesh, "ra_mesh_winding: null argument");
    RA_CHECK(find_mesh(c, mesh), "ra_mesh_winding: not a mesh of this ctx");
    RA_CHECK(n >= 0 && n < (1 << 30), "ra_mesh_winding: bad sizes");
    RA_CHECK((flags & ~(RA_WINDING_ONE_PASS | RA_WINDING_SPLIT)) == 0 && flags != (RA_WINDING_ONE_PASS | RA_WINDING_SPLIT), "ra_mesh_winding: unknown flag");
    if (n == 0) return 0;       // nothing to read or write: empty arrays have no address
    RA_CHECK(pts && winding, "ra_mesh_winding: null argument (pts, winding)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    // few points: the faces are split across workgroups to fill the chip, and a second pass adds the chunk sums in chunk order (the same bits)
    const long long n_chunks = wind_chunk_count(mesh->view.n_leaves), tiles = ((long long)n + WIND_BLOCK - 1) / WIND_BLOCK;
    const bool split = (flags & RA_WINDING_SPLIT) || (!(flags & RA_WINDING_ONE_PASS) && n_chunks > 1 && tiles < WIND_SPLIT_TILES && n * n_chunks <= WIND_SPLIT_MAX);
    double* partial = nullptr;
    if (split) {
        int err = 0;
        partial = c->buf<double>("winding_partial", (size_t)(n * n_chunks), &err);
        RA_CHECK(!err, "ra_mesh_winding: out of device memory");
    }
    launch_mesh_winding(mesh->view, pts, n, partial, winding, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_mesh_winding_grad(ra_ctx* c, const ra_mesh* mesh, const float* pts, int n, int flags, float* winding, float* grad, void* stream) {
    RA_CHECK(c && mesh, "ra_mesh_winding_grad: null argument");
    RA_CHECK(find_mesh(c, mesh), "ra_mesh_winding_grad: not a mesh of this ctx");
    RA_CHECK(n >= 0 && n < (1 << 30), "ra_mesh_winding_grad: bad sizes");
    RA_CHECK((flags & ~(RA_WINDING_ONE_PASS | RA_WINDING_SPLIT)) == 0 && flags != (RA_WINDING_ONE_PASS | RA_WINDING_SPLIT), "ra_mesh_winding_grad: unknown flag");
    if (n == 0) return 0;       // nothing to read or write: empty arrays have no address
    RA_CHECK(pts && grad, "ra_mesh_winding_grad: null argument (pts, grad)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    // ra_mesh_winding's rule, with four float64 sums per (point, chunk) in the same budget of bytes
    const long long n_chunks = wind_chunk_count(mesh->view.n_leaves), tiles = ((long long)n + WIND_BLOCK - 1) / WIND_BLOCK;
    const bool split = (flags & RA_WINDING_SPLIT) || (!(flags & RA_WINDING_ONE_PASS) && n_chunks > 1 && tiles < WIND_SPLIT_TILES && n * n_chunks * 4 <= WIND_SPLIT_MAX);
    double* partial = nullptr;
    if (split) {
        int err = 0;
        partial = c->buf<double>("winding_grad_partial", (size_t)(n * n_chunks * 4), &err);
        RA_CHECK(!err, "ra_mesh_winding_grad: out of device memory");
    }
    launch_mesh_winding_grad(mesh->view, pts, n, partial, winding, grad, s);
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- ray-mesh intersection (ra_raycast.hip) -------------------------------------------------------
int ra_raycast_tile(int which) { return which == 0 ? RAY_BLOCK : which == 1 ? RAY_PAIR_BLOCK : which == 2 ? MESH_SORT_MIN : 0; }

int ra_mesh_raycast(ra_ctx* c, const ra_mesh* mesh, const float* ray_o, const float* ray_d, int n, int flags, float* t, int* face, float* uv,
                    int* count, void* stream) {
    RA_CHECK(c && mesh, "ra_mesh_raycast: null argument");
    RA_CHECK(find_mesh(c, mesh), "ra_mesh_raycast: not a mesh of this ctx");
    RA_CHECK(n >= 0 && n < (1 << 30), "ra_mesh_raycast: bad sizes");
    RA_CHECK((flags & ~(RA_RAYCAST_BRUTE | RA_RAYCAST_UNSORTED)) == 0, "ra_mesh_raycast: unknown flag");
    if (n == 0) return 0;       // nothing to read or write: empty arrays have no address
    RA_CHECK(ray_o && ray_d && (t || face || uv || count), "ra_mesh_raycast: null argument (ray_o, ray_d, or all four outputs)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    RayQuery q{};
    q.o = ray_o; q.d = ray_d; q.n = n; q.brute = (flags & RA_RAYCAST_BRUTE) != 0; q.t = t; q.face = face; q.uv = uv; q.count = count;
    // rays whose origins are neighbours share a wave (the Morton order of ra_mesh_closest's points; equal origins keep their order:
    // the radix sort is stable).  The answers do not depend on it
    if (!q.brute && !(flags & RA_RAYCAST_UNSORTED) && n > MESH_SORT_MIN) {
        MeshBuild b{};
        RA_CHECK(!mesh_sort_scratch(c, n, &b), "ra_mesh_raycast: out of device memory");
        RA_CHECK(launch_mesh_sort_points(ray_o, n, b, s) == 0, "ra_mesh_raycast: device sort failed");
        q.perm = b.vals_sorted;
    }
    launch_mesh_raycast(mesh->view, q, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_ray_tri_pairs(ra_ctx* c, const float* o, const float* d, int n, const float* tris, int f, float* u, float* v, float* t, void* stream) {
    RA_CHECK(c, "ra_ray_tri_pairs: null argument");
    RA_CHECK(n >= 0 && f >= 0 && (long long)n * f < RAY_MAX_PAIRS, "ra_ray_tri_pairs: bad sizes (n >= 0, f >= 0, n * f < 2^31)");
    if (n == 0 || f == 0) return 0;
    RA_CHECK(o && d && tris && (u || v || t), "ra_ray_tri_pairs: null argument (o, d, tris, or all three outputs)");
    RA_HIP(hipSetDevice(c->device));
    launch_ray_tri_pairs(o, d, n, tris, f, u, v, t, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- mesh connectivity and Taubin smoothing (ra_topo.hip) -----------------------------------------
int ra_topo_tile(int which) { return which == 0 ? TOPO_BLOCK : which == 1 ? TOPO_SMOOTH_BLOCK : which == 2 ? TOPO_MAX_CHANNELS : 0; }

static ra_topo* find_topo(ra_ctx* c, const ra_topo* t) {
    for (auto& p : c->topos) if (p.get() == t) return p.get();
    return nullptr;
}

static void topo_bind(ra_topo* t) {
    TopoView& v = t->view;
    v.vert = t->vert.as<int>(); v.twin = t->twin.as<int>(); v.edge = t->edge.as<int>(); v.edges = t->edges.as<int>(); v.counts = t->counts.as<int>();
    v.ehe_start = t->ehe_start.as<int>(); v.ehe = t->ehe.as<int>(); v.nbr_start = t->nbr_start.as<int>(); v.nbr = t->nbr.as<int>();
    v.out_start = t->out_start.as<int>(); v.out_he = t->out_he.as<int>();
}

// the Loop coefficients of every outgoing count up to the topology's largest: the table a subdivision step reads
static int topo_upload_weights(ra_topo* t, hipStream_t s) {
    std::vector<float>& w = t->loop_w_host;
    w.assign((size_t)2 * (t->max_out + 1), 0.f);
    for (int n = 1; n <= t->max_out; ++n) loop_weights(n, &w[2 * n], &w[2 * n + 1]);
    if (t->loop_w.ensure(w.size() * sizeof(float))) return 1;
    return hipMemcpyAsync(t->loop_w.p, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, s) == hipSuccess ? 0 : 1;
}

int ra_topo_create(ra_ctx* c, const int* faces, int n_faces, int n_verts, ra_topo** out, void* stream) {
    RA_CHECK(c && out, "ra_topo_create: null argument");
    RA_CHECK(n_faces >= 0 && n_faces <= TOPO_MAX_FACES && n_verts >= 0 && n_verts < (1 << 30) && (n_verts > 0 || n_faces == 0),
             "ra_topo_create: bad sizes (n_faces <= 2^29 / 3, n_verts < 2^30; faces need vertices)");
    RA_CHECK(n_faces == 0 || faces, "ra_topo_create: null argument (faces)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    std::unique_ptr<ra_topo> t(new ra_topo());
    const size_t n = (size_t)3 * n_faces, V = (size_t)n_verts;
    // the edge-sized arrays at their upper bound (E <= 3 F), so that E is needed on the host only once everything is queued
    RA_CHECK(!t->vert.ensure(n * 4 + 4) && !t->twin.ensure(n * 4 + 4) && !t->edge.ensure(n * 4 + 4) && !t->edges.ensure(n * 8 + 4) && !t->counts.ensure(n * 4 + 4) &&
             !t->ehe_start.ensure(n * 4 + 4) && !t->ehe.ensure(n * 4 + 4) && !t->nbr_start.ensure(V * 4 + 4) && !t->nbr.ensure(n * 8 + 4) &&
             !t->out_start.ensure(V * 4 + 4) && !t->out_he.ensure(n * 4 + 4), "ra_topo_create: out of device memory");
    TopoView& v = t->view;
    v.n_faces = n_faces; v.n_verts = n_verts; v.n_edges = 0;
    topo_bind(t.get());
    if (n_faces == 0) {         // no edge: every list is empty
        RA_HIP(hipMemsetAsync(t->ehe_start.p, 0, 4, s));
        RA_HIP(hipMemsetAsync(t->nbr_start.p, 0, V * 4 + 4, s));
        RA_HIP(hipMemsetAsync(t->out_start.p, 0, V * 4 + 4, s));
    } else {
        TopoBuild b{};
        int err = 0;
        b.faces = faces; b.n_faces = n_faces; b.n_verts = n_verts;
        b.vert = t->vert.as<int>(); b.twin = t->twin.as<int>(); b.edge = t->edge.as<int>(); b.edges = t->edges.as<int>(); b.counts = t->counts.as<int>();
        b.ehe_start = t->ehe_start.as<int>(); b.ehe = t->ehe.as<int>(); b.nbr_start = t->nbr_start.as<int>(); b.nbr = t->nbr.as<int>();
        b.out_start = t->out_start.as<int>(); b.out_he = t->out_he.as<int>();
        b.temp_bytes = topo_temp_bytes(n_faces, n_verts);
        b.keys = c->buf<unsigned long long>("topo_keys", n, &err);
        b.keys_sorted = c->buf<unsigned long long>("topo_keys_sorted", n, &err);
        b.slots = c->buf<int>("topo_slots", n, &err);
        b.head = c->buf<int>("topo_head", n + 1, &err);
        b.off = c->buf<int>("topo_off", n + 1, &err);
        b.deg = c->buf<int>("topo_deg", V + 1, &err);
        b.odeg = c->buf<int>("topo_odeg", V + 1, &err);
        b.fill = c->buf<int>("topo_fill", V, &err);
        b.stat = c->buf<int>("topo_stat", TOPO_STAT_INTS, &err);
        b.temp = c->buf<char>("topo_tmp", b.temp_bytes + 16, &err);
        RA_CHECK(!err, "ra_topo_create: out of device memory");
        RA_HIP(hipMemsetAsync(b.deg, 0, (V + 1) * 4, s));
        RA_HIP(hipMemsetAsync(b.odeg, 0, (V + 1) * 4, s));
        RA_HIP(hipMemsetAsync(b.fill, 0, V * 4, s));
        RA_HIP(hipMemsetAsync(b.stat, 0, TOPO_STAT_INTS * sizeof(int), s));
        RA_CHECK(launch_topo_build(b, s) == 0, "ra_topo_create: device sort failed");
        RA_HIP(hipGetLastError());
        int stat[TOPO_STAT_INTS] = {};      // the one read-back: the face-index verdict, E and the two largest valences together
        RA_HIP(hipMemcpyAsync(stat, b.stat, sizeof(stat), hipMemcpyDeviceToHost, s));
        RA_HIP(hipStreamSynchronize(s));
        ++t->readbacks;
        RA_CHECK(stat[TOPO_BAD] == 0, "ra_topo_create: face index outside [0, n_verts)");
        v.n_edges = stat[TOPO_E]; t->max_nbr = stat[TOPO_MAX_NBR]; t->max_out = stat[TOPO_MAX_OUT]; t->max_count = stat[TOPO_MAX_COUNT];
    }
    RA_CHECK(!topo_upload_weights(t.get(), s), "ra_topo_create: out of device memory");
    *out = t.get();
    c->topos.push_back(std::move(t));
    return 0;
}

int ra_topo_destroy(ra_ctx* c, ra_topo* topo) {
    RA_CHECK(c, "ra_topo_destroy: null argument");
    if (!topo) return 0;
    RA_CHECK(find_topo(c, topo), "ra_topo_destroy: not a topology of this ctx");
    for (auto& g : c->cloths) RA_CHECK(g->topo != topo, "ra_topo_destroy: a cloth of this ctx still reads this topology (ra_cloth_destroy first)");
    hipSetDevice(c->device);
    hipDeviceSynchronize();      // smoothing passes that read it may still be queued
    for (auto it = c->topos.begin(); it != c->topos.end(); ++it)
        if (it->get() == topo) { c->topos.erase(it); break; }
    return 0;
}

int ra_topo_sizes(ra_ctx* c, const ra_topo* topo, int* sizes) {
    RA_CHECK(c && topo && sizes, "ra_topo_sizes: null argument");
    RA_CHECK(find_topo(c, topo), "ra_topo_sizes: not a topology of this ctx");
    sizes[0] = topo->view.n_faces; sizes[1] = topo->view.n_verts; sizes[2] = topo->view.n_edges;
    sizes[3] = topo->max_nbr; sizes[4] = topo->max_out; sizes[5] = topo->readbacks; sizes[6] = topo->max_count;
    return 0;
}

int ra_topo_array(ra_ctx* c, const ra_topo* topo, int which, int* out, void* stream) {
    RA_CHECK(c && topo, "ra_topo_array: null argument");
    RA_CHECK(find_topo(c, topo), "ra_topo_array: not a topology of this ctx");
    const TopoView& v = topo->view;
    const size_t HE = (size_t)3 * v.n_faces, E = (size_t)v.n_edges, V = (size_t)v.n_verts;
    const int* src = nullptr;
    size_t n = 0;
    switch (which) {
        case RA_TOPO_VERT: src = v.vert; n = HE; break;
        case RA_TOPO_TWIN: src = v.twin; n = HE; break;
        case RA_TOPO_EDGE: src = v.edge; n = HE; break;
        case RA_TOPO_EDGES: src = v.edges; n = 2 * E; break;
        case RA_TOPO_EDGE_COUNTS: src = v.counts; n = E; break;
        case RA_TOPO_EDGE_HE_START: src = v.ehe_start; n = E + 1; break;
        case RA_TOPO_EDGE_HE: src = v.ehe; n = HE; break;
        case RA_TOPO_NBR_START: src = v.nbr_start; n = V + 1; break;
        case RA_TOPO_NBR: src = v.nbr; n = 2 * E; break;
        case RA_TOPO_OUT_START: src = v.out_start; n = V + 1; break;
        case RA_TOPO_OUT_HE: src = v.out_he; n = HE; break;
        default: RA_CHECK(false, "ra_topo_array: unknown array");
    }
    if (n == 0) return 0;
    RA_CHECK(out, "ra_topo_array: null argument (out)");
    RA_HIP(hipSetDevice(c->device));
    RA_HIP(hipMemcpyAsync(out, src, n * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int ra_mesh_smooth(ra_ctx* c, const ra_topo* topo, const float* values, int n_verts, int C, const long long* inds, int n_inds, float alpha, int iters,
                   float* out, void* stream) {
    RA_CHECK(c && topo, "ra_mesh_smooth: null argument");
    RA_CHECK(find_topo(c, topo), "ra_mesh_smooth: not a topology of this ctx");
    RA_CHECK(n_verts == topo->view.n_verts && C >= 1 && C <= TOPO_MAX_CHANNELS && iters >= 0 && iters < (1 << 20) && n_inds >= 0 && (inds || n_inds == 0),
             "ra_mesh_smooth: bad sizes (n_verts of the topology, 1 <= C <= 64, iters >= 0, n_inds >= 0 with inds)");
    RA_CHECK(alpha == alpha, "ra_mesh_smooth: bad alpha (NaN)");
    if (n_verts == 0) return 0;     // nothing to read or write: empty arrays have no address
    RA_CHECK(values && out && values != out, "ra_mesh_smooth: null argument (values, out; out must not be values)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    const size_t total = (size_t)n_verts * C;
    if (iters == 0) {
        RA_HIP(hipMemcpyAsync(out, values, total * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    int err = 0;
    float* tmp = c->buf<float>("topo_smooth", total, &err);
    unsigned char* move = inds ? c->buf<unsigned char>("topo_move", n_verts, &err) : nullptr;
    RA_CHECK(!err, "ra_mesh_smooth: out of device memory");
    if (move) {
        RA_HIP(hipMemsetAsync(move, 0, n_verts, s));
        launch_topo_mark_rows(inds, n_inds, n_verts, move, s);
    }
    // pass k of 2 iters reads what pass k - 1 wrote; the last one writes out, so the buffers alternate backwards from there
    const int passes = 2 * iters;
    const float* src = values;
    for (int k = 0; k < passes; ++k) {
        float* dst = (passes - 1 - k) % 2 == 0 ? out : tmp;
        launch_topo_smooth_pass(topo->view, src, C, move, taubin_coeff(alpha, k & 1), dst, s);
        src = dst;
    }
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_loop_weights(int n, float* w_self, float* beta) {
    RA_CHECK(w_self && beta, "ra_loop_weights: null argument");
    RA_CHECK(n >= 1, "ra_loop_weights: bad sizes (n >= 1)");
    loop_weights(n, w_self, beta);
    return 0;
}

int ra_mesh_subdivide(ra_ctx* c, const ra_topo* topo, const float* values, int n_verts, int C, float* out_values, int* out_faces, ra_topo** child,
                      void* stream) {
    RA_CHECK(c && topo, "ra_mesh_subdivide: null argument");
    ra_topo* parent = find_topo(c, topo);
    RA_CHECK(parent, "ra_mesh_subdivide: not a topology of this ctx");
    const TopoView& pv = parent->view;
    const long long HE = 3ll * pv.n_faces, V2 = (long long)pv.n_verts + pv.n_edges, E2 = 2ll * pv.n_edges + HE;
    RA_CHECK(n_verts == pv.n_verts && C >= 1 && C <= TOPO_MAX_CHANNELS, "ra_mesh_subdivide: bad sizes (n_verts of the topology, 1 <= C <= 64)");
    RA_CHECK(4 * HE <= 3ll * TOPO_MAX_FACES && V2 < (1 << 30) && V2 * C < (1ll << 31),
             "ra_mesh_subdivide: bad sizes (the step's 12 F half-edges, V + E vertices or (V + E) x C values leave int32)");
    RA_CHECK((values && out_values && values != out_values) || V2 == 0, "ra_mesh_subdivide: null argument (values, out_values; out_values must not be values)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    if (V2 > 0) launch_loop_positions(pv, values, C, parent->loop_w.as<float>(), out_values, s);
    RA_HIP(hipGetLastError());
    if (!child && (!out_faces || pv.n_faces == 0)) return 0;
    // the child's connectivity: index arithmetic on the parent's; E' = 2 E + 3 F is known, so no sort and no read-back
    std::unique_ptr<ra_topo> t(new ra_topo());
    const size_t n = (size_t)4 * HE, V = (size_t)V2, E = (size_t)E2;
    RA_CHECK(!t->vert.ensure(n * 4 + 4) && !t->twin.ensure(n * 4 + 4) && !t->edge.ensure(n * 4 + 4) && !t->edges.ensure(E * 8 + 4) && !t->counts.ensure(E * 4 + 4) &&
             !t->ehe_start.ensure(E * 4 + 4) && !t->ehe.ensure(n * 4 + 4) && !t->nbr_start.ensure(V * 4 + 4) && !t->nbr.ensure(E * 8 + 4) &&
             !t->out_start.ensure(V * 4 + 4) && !t->out_he.ensure(n * 4 + 4), "ra_mesh_subdivide: out of device memory");
    t->view.n_faces = 4 * pv.n_faces; t->view.n_verts = (int)V2; t->view.n_edges = (int)E2;
    topo_bind(t.get());
    // what a read-back would have told: old vertices keep their outgoing count, an edge vertex has three per half-edge of its edge
    // (exact); the longest neighbour list is an upper bound (old: as before; an edge vertex: two ends and two per half-edge)
    t->max_count = pv.n_faces ? (parent->max_count > 2 ? parent->max_count : 2) : 0;
    t->max_out = parent->max_out > 3 * parent->max_count ? parent->max_out : 3 * parent->max_count;
    t->max_nbr = parent->max_nbr > 2 + 2 * parent->max_count ? parent->max_nbr : (pv.n_faces ? 2 + 2 * parent->max_count : 0);
    if (pv.n_faces == 0) {
        RA_HIP(hipMemsetAsync(t->ehe_start.p, 0, 4, s));
        RA_HIP(hipMemsetAsync(t->nbr_start.p, 0, V * 4 + 4, s));
        RA_HIP(hipMemsetAsync(t->out_start.p, 0, V * 4 + 4, s));
    } else {
        TopoChild k{};
        int err = 0;
        k.vert = t->vert.as<int>(); k.twin = t->twin.as<int>(); k.edge = t->edge.as<int>(); k.edges = t->edges.as<int>(); k.counts = t->counts.as<int>();
        k.ehe_start = t->ehe_start.as<int>(); k.ehe = t->ehe.as<int>(); k.nbr_start = t->nbr_start.as<int>(); k.nbr = t->nbr.as<int>();
        k.out_start = t->out_start.as<int>(); k.out_he = t->out_he.as<int>();
        k.temp_bytes = topo_temp_bytes(0, (int)V2);
        k.deg = c->buf<int>("topo_deg", V + 1, &err);
        k.fill = c->buf<int>("topo_fill", V, &err);
        k.scratch_stat = c->buf<int>("topo_stat", TOPO_STAT_INTS, &err);
        k.temp = c->buf<char>("topo_tmp", k.temp_bytes + 16, &err);
        RA_CHECK(!err, "ra_mesh_subdivide: out of device memory");
        RA_HIP(hipMemsetAsync(k.deg, 0, (V + 1) * 4, s));
        RA_HIP(hipMemsetAsync(k.fill, 0, V * 4, s));
        RA_CHECK(launch_topo_child(pv, k, out_faces, s) == 0, "ra_mesh_subdivide: device scan failed");
        RA_HIP(hipGetLastError());
    }
    RA_CHECK(!topo_upload_weights(t.get(), s), "ra_mesh_subdivide: out of device memory");
    if (child) {
        *child = t.get();
        c->topos.push_back(std::move(t));
    } else {
        RA_HIP(hipStreamSynchronize(s));      // the faces were written through the child's arrays, which go with it
    }
    return 0;
}

int ra_topo_dilate(ra_ctx* c, const ra_topo* topo, const unsigned char* mask, int n_verts, int steps, unsigned char* out, void* stream) {
    RA_CHECK(c && topo, "ra_topo_dilate: null argument");
    RA_CHECK(find_topo(c, topo), "ra_topo_dilate: not a topology of this ctx");
    RA_CHECK(n_verts == topo->view.n_verts && steps >= 0 && steps < (1 << 20), "ra_topo_dilate: bad sizes (n_verts of the topology, steps >= 0)");
    if (n_verts == 0) return 0;
    RA_CHECK(mask && out && mask != out, "ra_topo_dilate: null argument (mask, out; out must not be mask)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    if (steps == 0) {
        RA_HIP(hipMemcpyAsync(out, mask, n_verts, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    int err = 0;
    unsigned char* tmp = c->buf<unsigned char>("topo_dilate", n_verts, &err);
    RA_CHECK(!err, "ra_topo_dilate: out of device memory");
    const unsigned char* src = mask;
    for (int k = 0; k < steps; ++k) {
        unsigned char* dst = (steps - 1 - k) % 2 == 0 ? out : tmp;
        launch_topo_dilate_pass(topo->view, src, dst, s);
        src = dst;
    }
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- mesh fitting: the large-steps operator and solve, normals, ICP residual, AdamUniform (ra_fit.hip) ----------------------------
int ra_fit_tile(int which) { return which == 0 ? FIT_BLOCK : which == 1 ? FIT_BLOCK : 0; }

int ra_topo_diffuse_apply(ra_ctx* c, const ra_topo* topo, const float* x, int n_verts, int C, float lambda, float* out, void* stream) {
    RA_CHECK(c && topo, "ra_topo_diffuse_apply: null argument");
    RA_CHECK(find_topo(c, topo), "ra_topo_diffuse_apply: not a topology of this ctx");
    RA_CHECK(n_verts == topo->view.n_verts && C >= 1 && C <= FIT_MAX_CHANNELS, "ra_topo_diffuse_apply: bad sizes (n_verts of the topology, 1 <= C <= 64)");
    RA_CHECK(lambda >= 0.0f && lambda <= 3.0e38f, "ra_topo_diffuse_apply: bad lambda (NaN, negative or infinite)");
    if (n_verts == 0) return 0;
    RA_CHECK(x && out && x != out, "ra_topo_diffuse_apply: null argument (x, out; out must not be x)");
    RA_HIP(hipSetDevice(c->device));
    launch_fit_apply(topo->view, x, C, (double)lambda, out, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_topo_diffuse_solve(ra_ctx* c, const ra_topo* topo, const float* b, int n_verts, int C, float lambda, const float* x0, double tol, int max_iter,
                          float* out, void* info, void* stream) {
    RA_CHECK(c && topo, "ra_topo_diffuse_solve: null argument");
    RA_CHECK(find_topo(c, topo), "ra_topo_diffuse_solve: not a topology of this ctx");
    RA_CHECK(n_verts == topo->view.n_verts && C >= 1 && C <= FIT_MAX_CHANNELS && max_iter >= 0 && max_iter < (1 << 20),
             "ra_topo_diffuse_solve: bad sizes (n_verts of the topology, 1 <= C <= 64, 0 <= max_iter < 2^20)");
    RA_CHECK(lambda >= 0.0f && lambda <= 3.0e38f, "ra_topo_diffuse_solve: bad lambda (NaN, negative or infinite)");
    RA_CHECK(tol >= 0.0 && tol < 1.0, "ra_topo_diffuse_solve: bad tol (0 <= tol < 1)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    if (n_verts == 0) {
        if (info) RA_HIP(hipMemsetAsync(info, 0, (size_t)C * sizeof(FitInfo), s));
        return 0;
    }
    RA_CHECK(b && out, "ra_topo_diffuse_solve: null argument (b, out)");
    FitSolve f{};
    f.nbr_start = topo->view.nbr_start; f.nbr = topo->view.nbr;
    f.n_verts = n_verts; f.C = C; f.n_tiles = (n_verts + FIT_BLOCK - 1) / FIT_BLOCK;
    f.b = b; f.x0 = x0; f.lambda = (double)lambda; f.tol = tol;
    const size_t total = (size_t)n_verts * C;
    int err = 0;
    double* state = c->buf<double>("fit_state", 6 * total + n_verts, &err);
    f.part = c->buf<double>("fit_part", (size_t)3 * C * f.n_tiles, &err);
    f.st = c->buf<FitState>("fit_scalars", FIT_MAX_CHANNELS, &err);
    RA_CHECK(!err, "ra_topo_diffuse_solve: out of device memory");
    f.x = state; f.r = state + total; f.z = state + 2 * total; f.p0 = state + 3 * total; f.p1 = state + 4 * total; f.q = state + 5 * total; f.diag = state + 6 * total;
    launch_fit_solve(f, max_iter, out, (FitInfo*)info, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_mesh_normals(ra_ctx* c, const ra_topo* topo, const float* verts, int n_verts, float* face_normal, float* face_area, float* vert_normal,
                    void* stream) {
    RA_CHECK(c && topo, "ra_mesh_normals: null argument");
    RA_CHECK(find_topo(c, topo), "ra_mesh_normals: not a topology of this ctx");
    RA_CHECK(n_verts == topo->view.n_verts, "ra_mesh_normals: bad sizes (n_verts of the topology)");
    RA_CHECK(face_normal || face_area || vert_normal, "ra_mesh_normals: null argument (all three outputs)");
    if (n_verts == 0) return 0;
    RA_CHECK(verts, "ra_mesh_normals: null argument (verts)");
    RA_HIP(hipSetDevice(c->device));
    launch_mesh_normals(topo->view, verts, face_normal, face_area, vert_normal, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_icp_residual(ra_ctx* c, const ra_mesh* mesh, const float* pts, const float* pt_normals, int n, const float* face_normals, float dist_th,
                    float angle_th, double* sums, float* grad, unsigned char* keep, void* stream) {
    RA_CHECK(c && mesh && sums, "ra_icp_residual: null argument");
    RA_CHECK(find_mesh(c, mesh), "ra_icp_residual: not a mesh of this ctx");
    RA_CHECK(n >= 0 && n < (1 << 29), "ra_icp_residual: bad sizes");
    RA_CHECK(dist_th == dist_th && angle_th == angle_th, "ra_icp_residual: bad threshold (NaN)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    if (n == 0) {       // an empty mean: sum 0 over count 0
        RA_HIP(hipMemsetAsync(sums, 0, 2 * sizeof(double), s));
        return 0;
    }
    RA_CHECK(pts && pt_normals && face_normals, "ra_icp_residual: null argument (pts, pt_normals, face_normals)");
    IcpJob j{};
    j.n = n; j.n_faces = mesh->view.n_faces; j.n_tiles = (n + FIT_BLOCK - 1) / FIT_BLOCK;
    j.pts = pts; j.pt_normals = pt_normals; j.face_normals = face_normals; j.dist_th = dist_th; j.angle_th = angle_th;
    int err = 0;
    float* d2 = c->buf<float>("icp_d2", n, &err);
    float* closest = c->buf<float>("icp_closest", (size_t)n * 3, &err);
    int* face = c->buf<int>("icp_face", n, &err);
    j.part = c->buf<double>("icp_part", (size_t)2 * j.n_tiles, &err);
    j.keep = keep ? keep : c->buf<unsigned char>("icp_keep", n, &err);
    RA_CHECK(!err, "ra_icp_residual: out of device memory");
    if (ra_mesh_closest(c, mesh, pts, n, 0, d2, closest, face, nullptr, stream)) return 1;
    j.d2 = d2; j.closest = closest; j.face = face;
    launch_icp_residual(j, sums, grad, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_adam_uniform_step(ra_ctx* c, float* param, const float* grad, float* g1, float* g2, long long n, int step, float lr, float b1, float b2,
                         void* stream) {
    RA_CHECK(c, "ra_adam_uniform_step: null argument");
    RA_CHECK(n >= 0 && n < (1ll << 31) && step >= 1 && step < (1 << 24), "ra_adam_uniform_step: bad sizes (0 <= n < 2^31, 1 <= step < 2^24)");
    RA_CHECK(lr == lr && b1 >= 0.0f && b1 < 1.0f && b2 >= 0.0f && b2 < 1.0f, "ra_adam_uniform_step: bad lr or betas (0 <= beta < 1)");
    if (n == 0) return 0;
    RA_CHECK(param && grad && g1 && g2, "ra_adam_uniform_step: null argument (param, grad, g1, g2)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    int err = 0;
    unsigned* scratch = c->buf<unsigned>("adam_scratch", 2, &err);
    RA_CHECK(!err, "ra_adam_uniform_step: out of device memory");
    RA_HIP(hipMemsetAsync(scratch, 0, 2 * sizeof(unsigned), s));
    launch_adam_uniform(param, grad, g1, g2, n, scratch, (double)lr, (double)b1, (double)b2, 1.0 - fit_pow((double)b1, step), 1.0 - fit_pow((double)b2, step), s);
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- cloth energies: StVK stretch, dihedral bending, gravity, inertia (ra_cloth.hip) --------------------------------------------
int ra_cloth_tile(int which) { return which >= 0 && which <= 2 ? CLOTH_BLOCK : which == 3 ? CLOTH_CHUNK : 0; }

static ra_cloth* find_cloth(ra_ctx* c, const ra_cloth* g) {
    for (auto& p : c->cloths) if (p.get() == g) return p.get();
    return nullptr;
}

static bool cloth_finite(double x) { return x - x == 0.0; }

int ra_cloth_material_derive(const ra_cloth_material* m, double* out) {
    RA_CHECK(m && out, "ra_cloth_material_derive: null argument");
    cloth_material(m->thickness, m->young_modulus, m->poisson_ratio, m->bending_multiplier, m->stretch_multiplier, m->material_multiplier, out);
    return 0;
}

int ra_cloth_create(ra_ctx* c, const ra_topo* topo, const float* rest, int n_verts, const float* vm, int n_vm, const int* fm, const ra_cloth_material* m,
                    ra_cloth** out, void* stream) {
    RA_CHECK(c && topo && m && out, "ra_cloth_create: null argument");
    RA_CHECK(find_topo(c, topo), "ra_cloth_create: not a topology of this ctx");
    const TopoView& t = topo->view;
    RA_CHECK(n_verts == t.n_verts && n_vm >= 0 && n_vm < (1 << 30) && (long long)t.n_edges * 18 < (1ll << 31) && (long long)t.n_faces * 9 < (1ll << 31),
             "ra_cloth_create: bad sizes (n_verts of the topology, 0 <= n_vm < 2^30, 18 E and 9 F below 2^31)");
    RA_CHECK(cloth_finite(m->density) && cloth_finite(m->thickness) && cloth_finite(m->young_modulus) && cloth_finite(m->poisson_ratio) &&
             cloth_finite(m->bending_multiplier) && cloth_finite(m->stretch_multiplier) && cloth_finite(m->material_multiplier),
             "ra_cloth_create: bad material (a parameter is not finite)");
    RA_CHECK(t.n_faces == 0 || (rest && vm && fm && n_vm > 0), "ra_cloth_create: null argument (rest_verts, vm, fm)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    std::unique_ptr<ra_cloth> g(new ra_cloth());
    g->topo = topo;
    cloth_material(m->thickness, m->young_modulus, m->poisson_ratio, m->bending_multiplier, m->stretch_multiplier, m->material_multiplier, g->coeffs);
    g->thickness = (float)m->thickness; g->mu = (float)g->coeffs[3]; g->lambda = (float)g->coeffs[4]; g->bending = (float)g->coeffs[2];
    const size_t F = (size_t)t.n_faces, E = (size_t)t.n_edges, V = (size_t)t.n_verts;
    RA_CHECK(!g->frec.ensure(F * 32 + 32) && !g->f_area.ensure(F * 4 + 4) && !g->dm.ensure(F * 16 + 16) && !g->dm_inv.ensure(F * 16 + 16) &&
             !g->hrec.ensure(E * 32 + 32) && !g->h_faces.ensure(E * 8 + 8) && !g->h_verts.ensure(E * 8 + 8) && !g->mass.ensure(V * 4 + 4) &&
             !g->inv_mass.ensure(V * 4 + 4) && !g->vh.ensure(F * 36 + 4) && !g->vh_count.ensure(V * 4 + 4), "ra_cloth_create: out of device memory");
    if (t.n_faces > 0) {
        int err = 0;
        int* bad = c->buf<int>("cloth_bad", 1, &err);
        RA_CHECK(!err, "ra_cloth_create: out of device memory");
        RA_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
        launch_cloth_check_fm(fm, t.n_faces, n_vm, bad, s);
        RA_HIP(hipGetLastError());
        int verdict = 0;        // the one read-back: nothing dereferences vm[fm] before it
        RA_HIP(hipMemcpyAsync(&verdict, bad, sizeof(int), hipMemcpyDeviceToHost, s));
        RA_HIP(hipStreamSynchronize(s));
        RA_CHECK(verdict == 0, "ra_cloth_create: material index (fm) outside [0, n_vm)");
    }
    ClothBuild b{};
    b.rest = rest; b.vm = vm; b.fm = fm; b.density = (float)m->density;
    b.frec = g->frec.as<float>(); b.f_area = g->f_area.as<float>(); b.dm = g->dm.as<float>(); b.dm_inv = g->dm_inv.as<float>();
    b.hrec = g->hrec.as<int>(); b.h_faces = g->h_faces.as<int>(); b.h_verts = g->h_verts.as<int>();
    b.mass = g->mass.as<float>(); b.inv_mass = g->inv_mass.as<float>(); b.vh = g->vh.as<int>(); b.vh_count = g->vh_count.as<int>();
    if (V > 0) {
        launch_cloth_build(t, b, s);
        RA_HIP(hipGetLastError());
    }
    *out = g.get();
    c->cloths.push_back(std::move(g));
    return 0;
}

int ra_cloth_destroy(ra_ctx* c, ra_cloth* cloth) {
    RA_CHECK(c, "ra_cloth_destroy: null argument");
    if (!cloth) return 0;
    RA_CHECK(find_cloth(c, cloth), "ra_cloth_destroy: not a cloth of this ctx");
    hipSetDevice(c->device);
    hipDeviceSynchronize();      // launches that read it may still be queued
    for (auto it = c->cloths.begin(); it != c->cloths.end(); ++it)
        if (it->get() == cloth) { c->cloths.erase(it); break; }
    return 0;
}

int ra_cloth_array(ra_ctx* c, const ra_cloth* cloth, int which, void* out, void* stream) {
    RA_CHECK(c && cloth, "ra_cloth_array: null argument");
    RA_CHECK(find_cloth(c, cloth), "ra_cloth_array: not a cloth of this ctx");
    const TopoView& t = cloth->topo->view;
    const size_t F = (size_t)t.n_faces, E = (size_t)t.n_edges, V = (size_t)t.n_verts;
    const void* src = nullptr;
    size_t n = 0;
    switch (which) {
        case RA_CLOTH_F_AREA: src = cloth->f_area.p; n = F; break;
        case RA_CLOTH_DM: src = cloth->dm.p; n = 4 * F; break;
        case RA_CLOTH_DM_INV: src = cloth->dm_inv.p; n = 4 * F; break;
        case RA_CLOTH_V_MASS: src = cloth->mass.p; n = V; break;
        case RA_CLOTH_INV_MASS: src = cloth->inv_mass.p; n = V; break;
        case RA_CLOTH_HINGE_FACES: src = cloth->h_faces.p; n = 2 * E; break;
        case RA_CLOTH_HINGE_VERTS: src = cloth->h_verts.p; n = 2 * E; break;
        default: RA_CHECK(false, "ra_cloth_array: unknown array");
    }
    if (n == 0) return 0;
    RA_CHECK(out, "ra_cloth_array: null argument (out)");
    RA_HIP(hipSetDevice(c->device));
    RA_HIP(hipMemcpyAsync(out, src, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int ra_cloth_energy(ra_ctx* c, const ra_cloth* cloth, const float* x, int B, int terms, float gravity, double* energy, float* grad, void* stream) {
    RA_CHECK(c && cloth && energy, "ra_cloth_energy: null argument");
    RA_CHECK(find_cloth(c, cloth), "ra_cloth_energy: not a cloth of this ctx");
    const int all = RA_CLOTH_STRETCH | RA_CLOTH_BENDING | RA_CLOTH_GRAVITY;
    RA_CHECK(terms > 0 && (terms & ~all) == 0, "ra_cloth_energy: bad terms (a non-empty set of RA_CLOTH_STRETCH, _BENDING, _GRAVITY)");
    RA_CHECK(gravity == gravity, "ra_cloth_energy: bad gravity (NaN)");
    const TopoView& t = cloth->topo->view;
    const long long most = std::max((long long)t.n_faces, std::max((long long)t.n_edges, (long long)t.n_verts));
    RA_CHECK(B >= 1 && B <= 65535 && (long long)B * most < (1ll << 31), "ra_cloth_energy: bad sizes (1 <= B <= 65535, B x elements < 2^31)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    RA_HIP(hipMemsetAsync(energy, 0, (size_t)B * 3 * sizeof(double), s));
    if (t.n_verts == 0) return 0;
    RA_CHECK(x, "ra_cloth_energy: null argument (x)");
    ClothJob j{};
    j.x = x; j.B = B; j.n_faces = t.n_faces; j.n_edges = t.n_edges; j.n_verts = t.n_verts; j.terms = terms;
    j.thickness = cloth->thickness; j.mu = cloth->mu; j.lambda = cloth->lambda; j.bending = cloth->bending; j.gravity = gravity;
    j.frec = cloth->frec.as<float>(); j.hrec = cloth->hrec.as<int>(); j.mass = cloth->mass.as<float>();
    j.vh = cloth->vh.as<int>(); j.vh_count = cloth->vh_count.as<int>();
    j.grad = grad;
    const size_t nb = (size_t)B, F = (size_t)t.n_faces, E = (size_t)t.n_edges, V = (size_t)t.n_verts;
    int err = 0;
    j.e_face = c->buf<float>("cloth_e_face", nb * F + 1, &err);
    j.e_hinge = c->buf<float>("cloth_e_hinge", nb * E + 1, &err);
    j.e_vert = c->buf<float>("cloth_e_vert", nb * V + 1, &err);
    j.part = c->buf<double>("cloth_part", nb * (((size_t)most + CLOTH_CHUNK - 1) / CLOTH_CHUNK) + 1, &err);
    if (grad) {
        j.g_face = c->buf<float>("cloth_g_face", (terms & RA_CLOTH_STRETCH) ? nb * F * 9 + 1 : 1, &err);
        j.g_hinge = c->buf<float>("cloth_g_hinge", (terms & RA_CLOTH_BENDING) ? nb * E * 18 + 1 : 1, &err);
    }
    RA_CHECK(!err, "ra_cloth_energy: out of device memory");
    launch_cloth_energy(t, j, energy, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_cloth_inertia(ra_ctx* c, const float* mass, const float* x_next, const float* x_curr, const float* v_curr, int rows, int V, float dt,
                     const float* accel3, double* value, float* g_next, float* g_curr, float* g_vel, void* stream) {
    RA_CHECK(c && mass && x_next && x_curr && v_curr && value, "ra_cloth_inertia: null argument");
    RA_CHECK(rows >= 1 && rows <= 65535 && V >= 1 && (long long)rows * V < (1ll << 31), "ra_cloth_inertia: bad sizes (1 <= rows <= 65535, V >= 1, rows x V < 2^31)");
    RA_CHECK(dt == dt && dt != 0.0f, "ra_cloth_inertia: bad delta_t (NaN or 0)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    InertiaJob j{};
    j.mass = mass; j.x_next = x_next; j.x_curr = x_curr; j.v_curr = v_curr; j.rows = rows; j.V = V; j.dt = dt;
    j.has_accel = accel3 != nullptr;
    for (int k = 0; k < 3; ++k) j.accel[k] = accel3 ? accel3[k] : 0.0f;
    j.g_next = g_next; j.g_curr = g_curr; j.g_vel = g_vel;
    int err = 0;
    j.el = c->buf<float>("cloth_e_vert", (size_t)rows * V + 1, &err);
    j.part = c->buf<double>("cloth_part", (size_t)rows * (((size_t)V + CLOTH_CHUNK - 1) / CLOTH_CHUNK) + 1, &err);
    RA_CHECK(!err, "ra_cloth_inertia: out of device memory");
    launch_cloth_inertia(j, value, s);
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- mesh rasterisation (ra_raster.hip) -----------------------------------------------------------
int ra_raster_tile(int which) { return which == 0 ? RASTER_TILE : which == 1 ? RASTER_BLOCK : which == 2 ? RASTER_MAX_CHANNELS : 0; }

static bool raster_sizes_ok(int B, int H, int W) { return B >= 1 && H >= 1 && W >= 1 && (long long)B * H * W < (1ll << 31); }

int ra_rasterize(ra_ctx* c, const float* pos, int B, int V, const int* faces, int F, int H, int W, int flags, float* uv, float* zw, int* face,
                 void* stream) {
    // sizes and flags first: they need no ctx, so a caller's mistake is named before anything is dereferenced or launched
    RA_CHECK(raster_sizes_ok(B, H, W) && V >= 0 && V < (1 << 29) && F >= 0 && F < RASTER_MAX_FACES && (long long)B * F < (1ll << 31) - 1 && (V > 0 || F == 0),
             "ra_rasterize: bad sizes (B, H, W >= 1, B x H x W < 2^31, F < 2^24, B x F < 2^31; faces need vertices)");
    RA_CHECK((flags & ~RA_RASTER_BRUTE) == 0, "ra_rasterize: unknown flag");
    RA_CHECK(c && uv && zw && face, "ra_rasterize: null argument");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    const size_t n_pix = (size_t)B * H * W;
    if (F == 0) {               // empty maps: nothing is launched
        RA_HIP(hipMemsetAsync(uv, 0, n_pix * 2 * sizeof(float), s));
        RA_HIP(hipMemsetAsync(zw, 0, n_pix * sizeof(float), s));
        RA_HIP(hipMemsetAsync(face, 0xff, n_pix * sizeof(int), s));
        return 0;
    }
    RA_CHECK(pos && faces, "ra_rasterize: null argument (pos, faces)");
    const bool brute = (flags & RA_RASTER_BRUTE) != 0;
    const size_t n = (size_t)B * F;
    RasterJob j{};
    j.pos = pos; j.faces = faces; j.B = B; j.V = V; j.F = F; j.H = H; j.W = W; j.uv = uv; j.zw = zw; j.face = face;
    int err = 0;
    j.recs = c->buf<float4>("raster_recs", n * 5, &err);
    j.stat = c->buf<int>("raster_stat", 2, &err);
    if (!brute) {
        j.temp_bytes = raster_temp_bytes((long long)n + 1, 0);
        j.counts = c->buf<unsigned long long>("raster_counts", n + 1, &err);
        j.off = c->buf<unsigned long long>("raster_off", n + 1, &err);
        j.temp = c->buf<char>("raster_tmp", j.temp_bytes + 16, &err);
    }
    RA_CHECK(!err, "ra_rasterize: out of device memory");
    RA_HIP(hipMemsetAsync(j.stat, 0, 2 * sizeof(int), s));
    RA_CHECK(launch_raster_setup(j, s) == 0, "ra_rasterize: device scan failed");
    RA_HIP(hipGetLastError());
    int stat[2] = {};           // the one read-back: the (tile, face) pair count, which sizes the keys, and the face-index verdict
    RA_HIP(hipMemcpyAsync(stat, j.stat, sizeof(stat), hipMemcpyDeviceToHost, s));
    RA_HIP(hipStreamSynchronize(s));
    RA_CHECK(stat[1] == 0, "ra_rasterize: face index outside [0, n_verts)");
    long long n_pairs = -1;
    if (!brute) {
        n_pairs = stat[0];
        RA_CHECK(n_pairs < 0x7fffffff, "ra_rasterize: bad sizes (2^31 or more (tile, face) pairs)");
        j.temp_bytes = raster_temp_bytes(0, n_pairs);
        j.keys = c->buf<unsigned long long>("raster_keys", (size_t)n_pairs + 1, &err);
        j.keys_sorted = c->buf<unsigned long long>("raster_keys_sorted", (size_t)n_pairs + 1, &err);
        j.temp = c->buf<char>("raster_sort_tmp", j.temp_bytes + 16, &err);
        RA_CHECK(!err, "ra_rasterize: out of device memory");
    }
    RA_CHECK(launch_raster_tiles(j, n_pairs, s) == 0, "ra_rasterize: device sort failed");
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_interpolate(ra_ctx* c, const float* attr, int per_view, int V, int A, const int* faces, int F, const float* uv, const int* face, int B, int H, int W,
                   float* out, void* stream) {
    RA_CHECK(raster_sizes_ok(B, H, W) && V >= 0 && V < (1 << 29) && F >= 0 && F < RASTER_MAX_FACES && A >= 1 && A <= RASTER_MAX_CHANNELS &&
             (long long)B * V * A < (1ll << 40), "ra_interpolate: bad sizes (B, H, W >= 1, B x H x W < 2^31, F < 2^24, 1 <= A <= 64)");
    RA_CHECK(c && out, "ra_interpolate: null argument");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    if (F == 0 || V == 0) {
        RA_HIP(hipMemsetAsync(out, 0, (size_t)B * H * W * A * sizeof(float), s));
        return 0;
    }
    RA_CHECK(attr && faces && uv && face, "ra_interpolate: null argument (attr, faces, uv, face)");
    InterpJob j{};
    j.attr = attr; j.faces = faces; j.uv = uv; j.face = face; j.B = B; j.V = V; j.F = F; j.H = H; j.W = W; j.A = A; j.per_view = per_view != 0; j.out = out;
    launch_interpolate(j, s);
    RA_HIP(hipGetLastError());
    return 0;
}

// the pixels of every (view, face) in ascending order, for the two backward passes
static int raster_pixel_runs(ra_ctx* c, const int* face, int B, int F, int H, int W, unsigned long long** sorted, hipStream_t s) {
    const size_t n = (size_t)B * H * W;
    int err = 0;
    const size_t tb = raster_temp_bytes(0, (long long)n);
    unsigned long long* keys = c->buf<unsigned long long>("raster_pix_keys", n, &err);
    *sorted = c->buf<unsigned long long>("raster_pix_sorted", n, &err);
    void* temp = c->buf<char>("raster_sort_tmp", tb + 16, &err);
    if (err) return 1;
    return launch_raster_pixel_sort(face, B, F, H, W, keys, *sorted, temp, tb, s) ? 2 : 0;
}

int ra_interpolate_backward(ra_ctx* c, const ra_topo* topo, const float* attr, int per_view, int V, int A, const float* uv, const int* face, int B, int H,
                            int W, const float* dout, float* dattr, float* duv, void* stream) {
    RA_CHECK(raster_sizes_ok(B, H, W) && V >= 0 && A >= 1 && A <= RASTER_MAX_CHANNELS,
             "ra_interpolate_backward: bad sizes (B, H, W >= 1, B x H x W < 2^31, 1 <= A <= 64)");
    RA_CHECK(c && topo && (dattr || duv), "ra_interpolate_backward: null argument");
    RA_CHECK(find_topo(c, topo), "ra_interpolate_backward: not a topology of this ctx");
    const TopoView& t = topo->view;
    RA_CHECK(raster_sizes_ok(B, H, W) && V == t.n_verts && t.n_faces < RASTER_MAX_FACES && A >= 1 && A <= RASTER_MAX_CHANNELS &&
             (long long)B * t.n_faces < (1ll << 31) - 1 && (long long)B * t.n_faces * 3 * A < (1ll << 40),
             "ra_interpolate_backward: bad sizes (B, H, W >= 1, B x H x W < 2^31, n_verts of the topology, F < 2^24, B x F < 2^31, 1 <= A <= 64)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    const size_t n_pix = (size_t)B * H * W;
    if (t.n_faces == 0 || V == 0) {
        if (dattr && V > 0) RA_HIP(hipMemsetAsync(dattr, 0, (size_t)(per_view ? B : 1) * V * A * sizeof(float), s));
        if (duv) RA_HIP(hipMemsetAsync(duv, 0, n_pix * 2 * sizeof(float), s));
        return 0;
    }
    RA_CHECK(attr && uv && face && dout, "ra_interpolate_backward: null argument (attr, uv, face, dout)");
    InterpJob j{};
    j.attr = attr; j.faces = t.vert; j.uv = uv; j.face = face; j.B = B; j.V = V; j.F = t.n_faces; j.H = H; j.W = W; j.A = A; j.per_view = per_view != 0;
    unsigned long long* sorted = nullptr;
    float* g_face = nullptr;
    if (dattr) {
        int err = 0;
        g_face = c->buf<float>("raster_g_face", (size_t)B * t.n_faces * 3 * A, &err);
        RA_CHECK(!err, "ra_interpolate_backward: out of device memory");
        const int rc = raster_pixel_runs(c, face, B, t.n_faces, H, W, &sorted, s);
        RA_CHECK(rc != 1, "ra_interpolate_backward: out of device memory");
        RA_CHECK(rc == 0, "ra_interpolate_backward: device sort failed");
    }
    launch_interpolate_backward(j, t, sorted, dout, g_face, dattr, duv, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_rasterize_backward(ra_ctx* c, const ra_topo* topo, const float* pos, int B, int V, int H, int W, const float* uv, const int* face, const float* duv,
                          float* dpos, void* stream) {
    RA_CHECK(raster_sizes_ok(B, H, W) && V >= 0, "ra_rasterize_backward: bad sizes (B, H, W >= 1, B x H x W < 2^31)");
    RA_CHECK(c && topo && dpos, "ra_rasterize_backward: null argument");
    RA_CHECK(find_topo(c, topo), "ra_rasterize_backward: not a topology of this ctx");
    const TopoView& t = topo->view;
    RA_CHECK(raster_sizes_ok(B, H, W) && V == t.n_verts && V < (1 << 29) && t.n_faces < RASTER_MAX_FACES && (long long)B * t.n_faces < (1ll << 31) - 1,
             "ra_rasterize_backward: bad sizes (B, H, W >= 1, B x H x W < 2^31, n_verts of the topology, F < 2^24, B x F < 2^31)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    if (V == 0) return 0;
    if (t.n_faces == 0) {
        RA_HIP(hipMemsetAsync(dpos, 0, (size_t)B * V * 4 * sizeof(float), s));
        return 0;
    }
    RA_CHECK(pos && uv && face && duv, "ra_rasterize_backward: null argument (pos, uv, face, duv)");
    int err = 0;
    float* g_face = c->buf<float>("raster_g_face", (size_t)B * t.n_faces * 9, &err);
    RA_CHECK(!err, "ra_rasterize_backward: out of device memory");
    unsigned long long* sorted = nullptr;
    const int rc = raster_pixel_runs(c, face, B, t.n_faces, H, W, &sorted, s);
    RA_CHECK(rc != 1, "ra_rasterize_backward: out of device memory");
    RA_CHECK(rc == 0, "ra_rasterize_backward: device sort failed");
    RasterBwdJob j{};
    j.pos = pos; j.uv = uv; j.duv = duv; j.B = B; j.H = H; j.W = W; j.dpos = dpos;
    launch_rasterize_backward(j, t, sorted, g_face, s);
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- silhouette antialiasing (ra_antialias.hip) ----------------------------------------------------
static bool antialias_sizes_ok(int C, int B, int V, int H, int W) {
    return C >= 1 && B >= 0 && V >= 0 && H >= 0 && W >= 0 && (long long)B * H < (1ll << 31) && (long long)B * H * W < (1ll << 31) &&
           (long long)B * H * W * C < (1ll << 31);
}

int ra_antialias(ra_ctx* c, const ra_topo* topo, const float* color, int C, const float* pos, int B, int V, const float* zw, const int* face, int H, int W,
                 float* out, void* stream) {
    RA_CHECK(antialias_sizes_ok(C, B, V, H, W), "ra_antialias: bad sizes (C >= 1, B, H, W >= 0, B x H x W x C < 2^31)");
    RA_CHECK(c && topo, "ra_antialias: null argument");
    RA_CHECK(find_topo(c, topo), "ra_antialias: not a topology of this ctx");
    const TopoView& t = topo->view;
    RA_CHECK(V == t.n_verts, "ra_antialias: bad sizes (n_verts of the topology)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)B * H * W * C;
    if (n == 0) return 0;
    RA_CHECK(color && out, "ra_antialias: null argument (color, out)");
    if (t.n_faces == 0) {
        RA_HIP(hipMemcpyAsync(out, color, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    RA_CHECK(pos && zw && face, "ra_antialias: null argument (pos, zw, face)");
    AaJob j{};
    j.color = color; j.pos = pos; j.zw = zw; j.face = face; j.B = B; j.H = H; j.W = W; j.C = C;
    launch_antialias_gather(j, t, nullptr, out, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_antialias_backward(ra_ctx* c, const ra_topo* topo, const float* color, int C, const float* pos, int B, int V, const float* zw, const int* face, int H,
                          int W, const float* dout, float pos_gradient_boost, float* dcolor, float* dpos, void* stream) {
    RA_CHECK(antialias_sizes_ok(C, B, V, H, W), "ra_antialias_backward: bad sizes (C >= 1, B, H, W >= 0, B x H x W x C < 2^31)");
    RA_CHECK(c && topo, "ra_antialias_backward: null argument");
    RA_CHECK(find_topo(c, topo), "ra_antialias_backward: not a topology of this ctx");
    const TopoView& t = topo->view;
    const long long n_pix = (long long)B * H * W;
    RA_CHECK(V == t.n_verts && (!dpos || (n_pix < (1ll << 30) && (long long)B * t.n_faces < (1ll << 29) &&
                                          (double)B * 3.0 * t.n_faces * 2.0 * H * W < 9.0e18)),
             "ra_antialias_backward: bad sizes (n_verts of the topology; with dpos B x H x W < 2^30, B x F < 2^29, 6 B F H W < 2^63)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)n_pix * C;
    if (n == 0 || t.n_faces == 0) {             // no pixel or no face: no pair.  An output of no elements may be null
        if (dcolor && n > 0) {
            RA_CHECK(dout, "ra_antialias_backward: null argument (dout)");
            RA_HIP(hipMemcpyAsync(dcolor, dout, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        if (dpos && (size_t)B * V > 0) RA_HIP(hipMemsetAsync(dpos, 0, (size_t)B * V * 4 * sizeof(float), s));
        return 0;
    }
    RA_CHECK(dcolor || dpos, "ra_antialias_backward: null argument");
    RA_CHECK(color && pos && zw && face && dout, "ra_antialias_backward: null argument (color, pos, zw, face, dout)");
    AaJob j{};
    j.color = color; j.pos = pos; j.zw = zw; j.face = face; j.B = B; j.H = H; j.W = W; j.C = C;
    if (dcolor) launch_antialias_gather(j, t, dout, dcolor, s);
    if (dpos) {
        int err = 0;
        size_t tb = antialias_temp_bytes(2 * n_pix, 0);
        unsigned long long* keys = c->buf<unsigned long long>("antialias_keys", 2 * (size_t)n_pix, &err);
        unsigned long long* compact = c->buf<unsigned long long>("antialias_keys_active", 2 * (size_t)n_pix, &err);
        int* count = c->buf<int>("antialias_count", 1, &err);
        void* temp = c->buf<char>("antialias_tmp", tb + 16, &err);
        float* g_he = c->buf<float>("antialias_g_he", (size_t)B * t.n_faces * 18, &err);
        RA_CHECK(!err, "ra_antialias_backward: out of device memory");
        RA_CHECK(launch_antialias_keys(j, t, keys, compact, count, temp, tb, s) == 0, "ra_antialias_backward: device compaction failed");
        RA_HIP(hipGetLastError());
        int n_active = 0;           // the one read-back: the number of active pairs, which sizes the sort and the run pass
        RA_HIP(hipMemcpyAsync(&n_active, count, sizeof(int), hipMemcpyDeviceToHost, s));
        RA_HIP(hipStreamSynchronize(s));
        RA_CHECK(n_active >= 0 && n_active <= 2 * n_pix, "ra_antialias_backward: device compaction failed");
        tb = antialias_temp_bytes(0, n_active);
        unsigned long long* sorted = c->buf<unsigned long long>("antialias_keys_sorted", (size_t)n_active + 1, &err);
        temp = c->buf<char>("antialias_sort_tmp", tb + 16, &err);
        RA_CHECK(!err, "ra_antialias_backward: out of device memory");
        RA_CHECK(launch_antialias_dpos(j, t, dout, pos_gradient_boost, compact, sorted, n_active, temp, tb, g_he, dpos, s) == 0,
                 "ra_antialias_backward: device sort failed");
    }
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- the texture path (ra_texture.hip) ------------------------------------------------------------
int ra_texture_tile(int which) { return which == 0 ? TEX_MAX_CHANNELS : which == 1 ? TEX_MAX_LEVELS : which == 2 ? TEX_MAX_EXTENT : which == 3 ? TEX_GROUP : 0; }

int ra_raster_db(ra_ctx* c, const float* pos, int B, int V, const int* faces, int F, const int* face, int H, int W, float* rast_db, void* stream) {
    RA_CHECK(raster_sizes_ok(B, H, W) && (long long)B * H * W < (1ll << 29) && V >= 0 && V < (1 << 29) && F >= 0 && F < RASTER_MAX_FACES,
             "ra_raster_db: bad sizes (B, H, W >= 1, B x H x W < 2^29, F < 2^24)");
    RA_CHECK(c && face && rast_db, "ra_raster_db: null argument");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    if (F == 0 || V == 0) {
        RA_HIP(hipMemsetAsync(rast_db, 0, (size_t)B * H * W * 4 * sizeof(float), s));
        return 0;
    }
    RA_CHECK(pos && faces, "ra_raster_db: null argument (pos, faces)");
    launch_raster_db(pos, B, V, faces, F, face, H, W, rast_db, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_interpolate_da(ra_ctx* c, const float* attr, int per_view, int V, int A, const int* faces, int F, const int* face, const float* rast_db, int B, int H,
                      int W, const int* channels, int n, float* out_da, void* stream) {
    RA_CHECK(raster_sizes_ok(B, H, W) && V >= 0 && V < (1 << 29) && F >= 0 && F < RASTER_MAX_FACES && A >= 1 && (long long)B * V * A < (1ll << 40) && n >= 1 &&
             n <= TEX_MAX_CHANNELS && (long long)B * H * W * 2 * n < (1ll << 31),
             "ra_interpolate_da: bad sizes (B, H, W >= 1, F < 2^24, A >= 1, 1 <= n <= 64, B x H x W x 2 n < 2^31)");
    RA_CHECK(channels && out_da, "ra_interpolate_da: null argument");
    for (int k = 0; k < n; ++k) RA_CHECK(channels[k] >= 0 && channels[k] < A, "ra_interpolate_da: bad sizes (a selected channel outside [0, A))");
    RA_CHECK(c, "ra_interpolate_da: null argument");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    if (F == 0 || V == 0) {
        RA_HIP(hipMemsetAsync(out_da, 0, (size_t)B * H * W * 2 * n * sizeof(float), s));
        return 0;
    }
    RA_CHECK(attr && faces && face && rast_db, "ra_interpolate_da: null argument (attr, faces, face, rast_db)");
    TexDaJob j{};
    j.attr = attr; j.faces = faces; j.face = face; j.rast_db = rast_db; j.per_view = per_view != 0; j.V = V; j.A = A; j.F = F; j.B = B; j.H = H; j.W = W; j.n = n;
    for (int k = 0; k < n; ++k) j.ch[k] = channels[k];
    launch_interpolate_da(j, out_da, s);
    RA_HIP(hipGetLastError());
    return 0;
}

static bool texture_tex_ok(int Bt, int TH, int TW, int C, int max_mip_level) {
    return Bt >= 1 && TH >= 1 && TW >= 1 && TH <= TEX_MAX_EXTENT && TW <= TEX_MAX_EXTENT && C >= 1 && C <= TEX_MAX_CHANNELS && max_mip_level >= 0 &&
           (long long)Bt * TH * TW * C < (1ll << 31);
}

int ra_texture_mips(ra_ctx* c, const float* tex, int Bt, int TH, int TW, int C, int max_mip_level, float* mips, int* lmax, long long* offsets, void* stream) {
    RA_CHECK(texture_tex_ok(Bt, TH, TW, C, max_mip_level),
             "ra_texture_mips: bad sizes (Bt >= 1, 1 <= TH, TW <= 32768, 1 <= C <= 64, max_mip_level >= 0, Bt x TH x TW x C < 2^31)");
    RA_CHECK(lmax && offsets, "ra_texture_mips: null argument");
    TexLevels L;
    texture_levels(TH, TW, max_mip_level, L);
    *lmax = L.n - 1;
    for (int l = 0; l <= L.n; ++l) offsets[l] = L.off[l];
    if (!mips) return 0;                // the sizes alone
    RA_CHECK(c && tex, "ra_texture_mips: null argument (ctx, tex)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    const long long total = L.off[L.n] * C, level0 = L.off[1] * C;
    for (int bt = 0; bt < Bt; ++bt)
        RA_HIP(hipMemcpyAsync(mips + (long long)bt * total, tex + (long long)bt * level0, (size_t)level0 * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int l = 1; l < L.n; ++l) launch_texture_mip(mips + L.off[l - 1] * C, total, mips + L.off[l] * C, total, Bt, L.h[l], L.w[l], C, s);
    RA_HIP(hipGetLastError());
    return 0;
}

// the job of ra_texture and ra_texture_backward: the chain of a trilinear call goes to the ctx's scratch
static int texture_job(ra_ctx* c, const char* who, const float* tex, int Bt, int TH, int TW, int C, const float* uv, const float* uv_da, int B, int H, int W,
                       int filter, int boundary, int max_mip_level, TexJob* j, hipStream_t s) {
    j->tex = tex; j->uv = uv; j->uv_da = uv_da; j->Bt = Bt; j->B = B; j->H = H; j->W = W; j->C = C; j->filter = filter; j->boundary = boundary;
    texture_levels(TH, TW, filter == TEX_TRILINEAR ? max_mip_level : 0, j->L);
    if (j->L.n > 1) {
        int err = 0;
        const long long stride = (j->L.off[j->L.n] - j->L.off[1]) * C;
        float* mips = c->buf<float>("texture_mips", (size_t)Bt * stride, &err);
        if (err) { ra_set_error(std::string(who) + ": out of device memory"); return 1; }
        launch_texture_mip(tex, j->L.off[1] * C, mips, stride, Bt, j->L.h[1], j->L.w[1], C, s);
        for (int l = 2; l < j->L.n; ++l)
            launch_texture_mip(mips + (j->L.off[l - 1] - j->L.off[1]) * C, stride, mips + (j->L.off[l] - j->L.off[1]) * C, stride, Bt, j->L.h[l], j->L.w[l], C, s);
        j->mips = mips;
    }
    return 0;
}

static bool texture_sizes_ok(int Bt, int TH, int TW, int C, int B, int H, int W, int max_mip_level) {
    return texture_tex_ok(Bt, TH, TW, C, max_mip_level) && raster_sizes_ok(B, H, W) && (Bt == 1 || Bt == B) && (long long)B * H * W * C < (1ll << 31);
}
#define RA_TEXTURE_SIZES "bad sizes (Bt = 1 or B, 1 <= TH, TW <= 32768, 1 <= C <= 64, max_mip_level >= 0, Bt x TH x TW x C < 2^31, B, H, W >= 1, B x H x W x C < 2^31"

int ra_texture(ra_ctx* c, const float* tex, int Bt, int TH, int TW, int C, const float* uv, const float* uv_da, int B, int H, int W, int filter, int boundary,
               int max_mip_level, float* out, void* stream) {
    RA_CHECK(texture_sizes_ok(Bt, TH, TW, C, B, H, W, max_mip_level), "ra_texture: " RA_TEXTURE_SIZES ")");
    RA_CHECK(filter >= TEX_NEAREST && filter <= TEX_TRILINEAR && boundary >= TEX_WRAP && boundary <= TEX_CLAMP, "ra_texture: unknown mode");
    RA_CHECK(c && tex && uv && out && (uv_da || filter != TEX_TRILINEAR), "ra_texture: null argument");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    TexJob j{};
    if (texture_job(c, "ra_texture", tex, Bt, TH, TW, C, uv, uv_da, B, H, W, filter, boundary, max_mip_level, &j, s)) return 1;
    launch_texture(j, out, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_texture_backward(ra_ctx* c, const float* tex, int Bt, int TH, int TW, int C, const float* uv, const float* uv_da, int B, int H, int W, int filter,
                        int boundary, int max_mip_level, const float* dout, float* duv, float* dtex, void* stream) {
    // the tap-count limit: the B H W T tap slots (T = 1, 4, 8 by filter) are sorted as ONE array of 64-bit keys indexed by an int
    const long long taps = (long long)B * H * W * texture_taps_per_pixel(filter);
    TexLevels L;
    if (TH >= 1 && TW >= 1 && max_mip_level >= 0) texture_levels(TH, TW, filter == TEX_TRILINEAR ? max_mip_level : 0, L); else { L.n = 1; L.off[1] = 1; }
    RA_CHECK(texture_sizes_ok(Bt, TH, TW, C, B, H, W, max_mip_level) &&
             (!dtex || (taps < (1ll << 31) - 1 && (double)B * (double)L.off[L.n] * (double)taps < 9.0e18 && (long long)B * L.off[L.n] * C < (1ll << 40))),
             "ra_texture_backward: " RA_TEXTURE_SIZES "; with dtex B x H x W x taps < 2^31 - 1 (taps 1, 4, 8 by filter) and B x texels x B x H x W x taps < 2^63)");
    RA_CHECK(filter >= TEX_NEAREST && filter <= TEX_TRILINEAR && boundary >= TEX_WRAP && boundary <= TEX_CLAMP, "ra_texture_backward: unknown mode");
    RA_CHECK(c && tex && uv && dout && (duv || dtex) && (uv_da || filter != TEX_TRILINEAR), "ra_texture_backward: null argument");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    TexJob j{};
    if (texture_job(c, "ra_texture_backward", tex, Bt, TH, TW, C, uv, uv_da, B, H, W, filter, boundary, max_mip_level, &j, s)) return 1;
    if (duv) launch_texture_duv(j, dout, duv, s);
    if (dtex) {
        int err = 0;
        const size_t tb = texture_temp_bytes(taps);
        unsigned long long* keys = c->buf<unsigned long long>("texture_keys", (size_t)taps, &err);
        unsigned long long* sorted = c->buf<unsigned long long>("texture_keys_sorted", (size_t)taps, &err);
        void* temp = c->buf<char>("texture_sort_tmp", tb + 16, &err);
        float* g = c->buf<float>("texture_g", (size_t)B * j.L.off[j.L.n] * C, &err);
        RA_CHECK(!err, "ra_texture_backward: out of device memory");
        RA_CHECK(launch_texture_dtex(j, dout, keys, sorted, temp, tb, g, dtex, s) == 0, "ra_texture_backward: device sort failed");
    }
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- mesh extraction: marching cubes and the largest component (ra_mcubes.hip) -------------------
int ra_mcubes_tile(int which) { return which == 0 ? MC_BLOCK : which == 1 ? LCC_PASSES : which == 2 ? VOL_TILE : which == 3 ? VOL_MAX_K : 0; }
int ra_mesh_extract_stats(const ra_ctx* c, int which) {
    return !c ? -1 : which == 0 ? c->vol_readbacks : which == 1 ? c->mc_query.readbacks : which == 2 ? c->lcc_query.readbacks : which == 3 ? c->lcc_query.passes : 0;
}

// pre: "mc_" the forward's scratch, which holds a pending size query's offsets; "mcg_" that of the backward and the vertex attributes
static int mc_job(ra_ctx* c, const float* vol, int nx, int ny, int nz, float iso, McJob* j, const std::string& pre = "mc_") {
    const size_t n = (size_t)nx * ny * nz;
    int err = 0;
    j->vol = vol; j->nx = nx; j->ny = ny; j->nz = nz; j->iso = iso;
    j->temp_bytes = mc_scan_temp_bytes((int)n + 1);
    j->cnt = c->buf<unsigned long long>(pre + "cnt", n + 1, &err);
    j->off = c->buf<unsigned long long>(pre + "off", n + 1, &err);
    j->mask = c->buf<unsigned char>(pre + "mask", n, &err);
    j->temp = c->buf<char>(pre + "tmp", j->temp_bytes + 16, &err);
    return err;
}

int ra_sdf_volume(ra_ctx* c, const float* xs, int nx, const float* ys, int ny, const float* zs, int nz, int mode, const float* verts, int n_verts,
                  int K, float dist_th, float fill, int pad, float* volume, int* n_kept, void* stream) {
    if (check_ready(c, "ra_sdf_volume")) return 1;
    RA_CHECK(xs && ys && zs && verts && volume, "ra_sdf_volume: null argument");
    RA_CHECK(mode >= RA_VOLUME_CANONICAL && mode <= RA_VOLUME_POSED, "ra_sdf_volume: unknown mode");
    RA_CHECK(nx >= 1 && ny >= 1 && nz >= 1 && pad >= 0 && pad <= 1024 &&
             (long long)(nx + 2 * pad) * (ny + 2 * pad) * (nz + 2 * pad) <= MC_MAX_POINTS, "ra_sdf_volume: bad sizes (the padded volume holds 2^27 points at most)");
    RA_CHECK(n_verts >= K && K >= 1 && K <= VOL_MAX_K, "ra_sdf_volume: bad K (1..4 nearest vertices, no more than there are)");
    RA_CHECK(dist_th == dist_th && fill == fill, "ra_sdf_volume: bad dist_th or fill (NaN)");
    hipStream_t s = (hipStream_t)stream;
    const int n = nx * ny * nz;
    const long long n_pad = (long long)(nx + 2 * pad) * (ny + 2 * pad) * (nz + 2 * pad);
    VolJob j{};
    j.xs = xs; j.ys = ys; j.zs = zs; j.nx = nx; j.ny = ny; j.nz = nz; j.pad = pad; j.verts = verts; j.n_verts = n_verts; j.K = K; j.dist_th = dist_th;
    int err = 0;
    j.temp_bytes = mc_scan_temp_bytes(n + 1);
    j.flag = c->buf<int>("vol_flag", (size_t)n + 1, &err);
    j.off = c->buf<int>("vol_off", (size_t)n + 1, &err);
    j.temp = c->buf<char>("vol_tmp", j.temp_bytes + 16, &err);
    RA_CHECK(!err, "ra_sdf_volume: out of device memory");
    launch_vol_fill(volume, n_pad, fill, s);
    RA_CHECK(launch_vol_filter(j, s) == 0, "ra_sdf_volume: device scan failed");
    RA_HIP(hipGetLastError());
    int kept = 0;       // the one read-back of this stage: the decoders' scratch is sized by it
    c->vol_readbacks = 0;
    RA_HIP(hipMemcpyAsync(&kept, j.off + n, sizeof(int), hipMemcpyDeviceToHost, s));
    RA_HIP(hipStreamSynchronize(s));
    ++c->vol_readbacks;
    if (n_kept) *n_kept = kept;
    if (kept == 0) return 0;
    float* pts = c->buf<float>("vol_pts", (size_t)kept * 3, &err);
    int* cell = c->buf<int>("vol_cell", kept, &err);
    float* sdf = c->buf<float>("vol_sdf", kept, &err);
    RA_CHECK(!err, "ra_sdf_volume: out of device memory");
    launch_vol_compact(j, pts, cell, s);
    RA_CHECK(sdf_points_precise(c, mode, pts, kept, dist_th, sdf, s) == 0, "ra_sdf_volume: out of device memory");
    launch_vol_scatter(sdf, cell, j.off + n, kept, volume, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_marching_cubes(ra_ctx* c, const float* volume, int nx, int ny, int nz, float iso, float* verts, int* faces, int* n_verts, int* n_faces,
                      void* stream) {
    RA_CHECK(c && volume, "ra_marching_cubes: null argument");
    RA_CHECK(nx >= 2 && ny >= 2 && nz >= 2 && (long long)nx * ny * nz <= MC_MAX_POINTS, "ra_marching_cubes: bad sizes (2 per axis at least, 2^27 points at most)");
    RA_CHECK(iso == iso, "ra_marching_cubes: bad iso (NaN)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    McQuery& q = c->mc_query;
    McJob j{};
    if (!verts && !faces) {         // the size query: classify, sum, read the two totals back
        RA_CHECK(n_verts && n_faces, "ra_marching_cubes: null argument (the size query needs n_verts and n_faces)");
        q.valid = false;
        RA_CHECK(!mc_job(c, volume, nx, ny, nz, iso, &j), "ra_marching_cubes: out of device memory");
        RA_CHECK(launch_mc_count(j, s) == 0, "ra_marching_cubes: device scan failed");
        RA_HIP(hipGetLastError());
        unsigned long long total = 0;
        q.readbacks = 0;
        RA_HIP(hipMemcpyAsync(&total, j.off + (size_t)nx * ny * nz, sizeof(total), hipMemcpyDeviceToHost, s));
        RA_HIP(hipStreamSynchronize(s));
        ++q.readbacks;
        q.vol = volume; q.nx = nx; q.ny = ny; q.nz = nz; q.iso = iso;
        q.n_verts = (int)(unsigned)total; q.n_faces = (int)(unsigned)(total >> 32);
        q.valid = true;
        *n_verts = q.n_verts; *n_faces = q.n_faces;
        return 0;
    }
    RA_CHECK(q.valid && q.vol == volume && q.nx == nx && q.ny == ny && q.nz == nz && std::memcmp(&q.iso, &iso, sizeof(float)) == 0,
             "ra_marching_cubes: no size query of this volume, these sizes and this iso precedes the call");
    RA_CHECK((verts || q.n_verts == 0) && (faces || q.n_faces == 0), "ra_marching_cubes: null argument (verts, faces)");
    q.valid = false;                // the scratch holds the offsets of this one query: used once
    if (n_verts) *n_verts = q.n_verts;
    if (n_faces) *n_faces = q.n_faces;
    if (q.n_verts == 0) return 0;   // no crossing: no vertex, no face
    RA_CHECK(!mc_job(c, volume, nx, ny, nz, iso, &j), "ra_marching_cubes: out of device memory");      // the buffers of the query: nothing grows
    launch_mc_emit(j, verts, q.n_verts, faces, q.n_faces, s);
    RA_HIP(hipGetLastError());
    return 0;
}

static bool mcg_sizes_ok(int nx, int ny, int nz, int C, int n_verts) {
    if (nx < 2 || ny < 2 || nz < 2 || (long long)nx * ny * nz > MC_MAX_POINTS || C < 0 || C > MCG_MAX_C || n_verts < 0) return false;
    const long long lim = 1ll << 31, n = (long long)nx * ny * nz;
    return n * (C > 0 ? C : 1) < lim && (long long)n_verts * (C > 3 ? C : 3) < lim;
}

int ra_marching_cubes_attrs(ra_ctx* c, const float* volume, int nx, int ny, int nz, float iso, const float* attrs, int C, int n_verts, float* out,
                            void* stream) {
    RA_CHECK(c && volume, "ra_marching_cubes_attrs: null argument");
    RA_CHECK(mcg_sizes_ok(nx, ny, nz, C, n_verts),
             "ra_marching_cubes_attrs: bad sizes (2 per axis at least, 2^27 points at most, 0 <= C <= 64, element counts below 2^31)");
    RA_CHECK(iso == iso, "ra_marching_cubes_attrs: bad iso (NaN)");
    RA_CHECK(C == 0 || n_verts == 0 || (attrs && out), "ra_marching_cubes_attrs: null argument (attrs, out)");
    if (C == 0 || n_verts == 0) return 0;       // nothing to write
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    McJob j{};
    RA_CHECK(!mc_job(c, volume, nx, ny, nz, iso, &j, "mcg_"), "ra_marching_cubes_attrs: out of device memory");
    RA_CHECK(launch_mc_count(j, s) == 0, "ra_marching_cubes_attrs: device scan failed");
    launch_mcg_attrs(j, attrs, C, n_verts, out, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_marching_cubes_backward(ra_ctx* c, const float* volume, int nx, int ny, int nz, float iso, const float* dverts, int n_verts, const float* attrs,
                               const float* dattr, int C, float* dvolume, float* dattrs_grid, void* stream) {
    RA_CHECK(c && volume && (dvolume || dattrs_grid), "ra_marching_cubes_backward: null argument");
    RA_CHECK(mcg_sizes_ok(nx, ny, nz, C, n_verts),
             "ra_marching_cubes_backward: bad sizes (2 per axis at least, 2^27 points at most, 0 <= C <= 64, element counts below 2^31)");
    RA_CHECK(iso == iso, "ra_marching_cubes_backward: bad iso (NaN)");
    RA_CHECK(C == 0 || n_verts == 0 || (attrs && dattr), "ra_marching_cubes_backward: null argument (attrs, dattr)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)nx * ny * nz;
    if (C == 0) dattrs_grid = nullptr;          // n x 0: nothing to write
    if (n_verts == 0) {                         // no vertex: the outputs are zeros, nothing else runs
        if (dvolume) RA_HIP(hipMemsetAsync(dvolume, 0, n * sizeof(float), s));
        if (dattrs_grid) RA_HIP(hipMemsetAsync(dattrs_grid, 0, n * C * sizeof(float), s));
        return 0;
    }
    if (!dvolume && !dattrs_grid) return 0;
    McJob j{};
    RA_CHECK(!mc_job(c, volume, nx, ny, nz, iso, &j, "mcg_"), "ra_marching_cubes_backward: out of device memory");
    RA_CHECK(launch_mc_count(j, s) == 0, "ra_marching_cubes_backward: device scan failed");
    launch_mcg_backward(j, dverts, n_verts, attrs, dattr, C, dvolume, dattrs_grid, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_mesh_largest_component(ra_ctx* c, const float* verts, int n_verts, const int* faces, int n_faces, float* out_verts, int* out_faces,
                              int* n_out_verts, int* n_out_faces, void* stream) {
    RA_CHECK(c, "ra_mesh_largest_component: null argument");
    RA_CHECK(n_verts >= 0 && n_faces >= 0 && n_faces <= LCC_MAX_FACES && (n_verts > 0 || n_faces == 0),
             "ra_mesh_largest_component: bad sizes (n_faces <= 2^27; faces need vertices)");
    RA_CHECK(n_faces == 0 || (verts && faces), "ra_mesh_largest_component: null argument (verts, faces)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    LccQuery& q = c->lcc_query;
    LccJob j{};
    j.faces = faces; j.n_faces = n_faces; j.n_verts = n_verts;
    auto scratch = [&]() {
        int err = 0;
        const size_t F = (size_t)n_faces, V = (size_t)n_verts;
        const size_t a = lcc_sort_temp_bytes(3 * n_faces), b = mc_scan_temp_bytes((n_faces > n_verts ? n_faces : n_verts) + 1);
        j.temp_bytes = a > b ? a : b;
        j.keys = c->buf<unsigned long long>("lcc_keys", 3 * F, &err);
        j.keys_sorted = c->buf<unsigned long long>("lcc_keys_sorted", 3 * F, &err);
        j.slots = c->buf<int>("lcc_slots", 3 * F, &err);
        j.slots_sorted = c->buf<int>("lcc_slots_sorted", 3 * F, &err);
        j.link = c->buf<int>("lcc_link", 6 * F, &err);
        j.label = c->buf<int>("lcc_label", F, &err);
        j.size = c->buf<int>("lcc_size", F, &err);
        j.kf = c->buf<int>("lcc_kf", F + 1, &err);
        j.of = c->buf<int>("lcc_of", F + 1, &err);
        j.kv = c->buf<int>("lcc_kv", V + 1, &err);
        j.ov = c->buf<int>("lcc_ov", V + 1, &err);
        j.stat = c->buf<int>("lcc_stat", LCC_STAT_INTS, &err);
        j.temp = c->buf<char>("lcc_tmp", j.temp_bytes + 16, &err);
        return err;
    };
    if (!out_verts && !out_faces) {     // the size query: labels, sizes, the winner, the new indices; one read-back per batch of LCC_PASSES passes
        RA_CHECK(n_out_verts && n_out_faces, "ra_mesh_largest_component: null argument (the size query needs n_out_verts and n_out_faces)");
        q.valid = false;
        int nv = 0, nf = 0;
        q.readbacks = q.passes = 0;
        if (n_faces > 0) {
            RA_CHECK(!scratch(), "ra_mesh_largest_component: out of device memory");
            RA_HIP(hipMemsetAsync(j.stat, 0, LCC_STAT_INTS * sizeof(int), s));
            RA_CHECK(launch_lcc_links(j, s) == 0, "ra_mesh_largest_component: device sort failed");
            for (;;) {
                // a batch of passes that stop working by themselves once one of them lowers nothing (ra_mcubes.hip); the flags and the winner start at 0
                RA_HIP(hipMemsetAsync(j.stat + LCC_BEST, 0, (LCC_STAT_INTS - LCC_BEST) * sizeof(int), s));
                launch_lcc_passes(j, s);
                // ... and the selection runs behind it unasked, so that labels that stand cost one read-back in all
                RA_HIP(hipMemsetAsync(j.size, 0, (size_t)n_faces * sizeof(int), s));
                RA_HIP(hipMemsetAsync(j.kf, 0, ((size_t)n_faces + 1) * sizeof(int), s));
                RA_HIP(hipMemsetAsync(j.kv, 0, ((size_t)n_verts + 1) * sizeof(int), s));
                RA_CHECK(launch_lcc_select(j, s) == 0, "ra_mesh_largest_component: device sort failed");
                RA_HIP(hipGetLastError());
                int stat[LCC_STAT_INTS] = {};
                RA_HIP(hipMemcpyAsync(stat, j.stat, sizeof(stat), hipMemcpyDeviceToHost, s));
                RA_HIP(hipMemcpyAsync(&nf, j.of + n_faces, sizeof(int), hipMemcpyDeviceToHost, s));
                RA_HIP(hipMemcpyAsync(&nv, j.ov + n_verts, sizeof(int), hipMemcpyDeviceToHost, s));
                RA_HIP(hipStreamSynchronize(s));
                ++q.readbacks;
                for (int k = 0; k < LCC_PASSES; ++k) q.passes += stat[LCC_FLAGS + k];
                RA_CHECK(stat[LCC_BAD] == 0, "ra_mesh_largest_component: face index outside [0, n_verts)");
                if (!stat[LCC_FLAGS + LCC_PASSES - 1]) break;       // some pass of the batch lowered nothing: the labels stand
            }
        }
        q.verts = verts; q.faces = faces; q.n_verts = n_verts; q.n_faces = n_faces; q.out_verts = nv; q.out_faces = nf;
        q.valid = true;
        *n_out_verts = nv; *n_out_faces = nf;
        return 0;
    }
    RA_CHECK(q.valid && q.verts == verts && q.faces == faces && q.n_verts == n_verts && q.n_faces == n_faces,
             "ra_mesh_largest_component: no size query of this mesh precedes the call");
    RA_CHECK((out_verts || q.out_verts == 0) && (out_faces || q.out_faces == 0), "ra_mesh_largest_component: null argument (out_verts, out_faces)");
    q.valid = false;
    if (n_out_verts) *n_out_verts = q.out_verts;
    if (n_out_faces) *n_out_faces = q.out_faces;
    if (q.out_faces == 0) return 0;
    RA_CHECK(!scratch(), "ra_mesh_largest_component: out of device memory");
    launch_lcc_gather(j, verts, out_verts, q.out_verts, out_faces, q.out_faces, s);
    RA_HIP(hipGetLastError());
    return 0;
}

static void inv3x3(const double* m, double* o) {
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    o[0] = (e * i - f * h) / det; o[1] = (c * h - b * i) / det; o[2] = (b * f - c * e) / det;
    o[3] = (f * g - d * i) / det; o[4] = (a * i - c * g) / det; o[5] = (c * d - a * f) / det;
    o[6] = (d * h - e * g) / det; o[7] = (b * g - a * h) / det; o[8] = (a * e - b * d) / det;
}

int ra_gen_rays(ra_ctx* c, int H, int W, const double* K, const double* R, const double* T, const float* bounds, const float* bounds_dev,
                void* ray_o, void* ray_d, void* near, void* far, void* mask_at_box, int* n_rays, int* n_rays_dev, void* stream) {
    RA_CHECK(c, "ra_gen_rays: null ctx");
    RA_CHECK(H > 0 && W > 0 && (long long)H * W < (1ll << 30), "ra_gen_rays: bad image size");
    RA_CHECK(K && R && T && (bounds || bounds_dev) && ray_o && ray_d && near && far && mask_at_box, "ra_gen_rays: null argument");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    RayCam cam;
    inv3x3(K, cam.Kinv);
    for (int k = 0; k < 9; ++k) cam.R[k] = R[k];
    for (int k = 0; k < 3; ++k) {
        cam.T[k] = T[k];
        cam.o[k] = -(R[k] * T[0] + R[3 + k] * T[1] + R[6 + k] * T[2]);      // -R^T T
        cam.bmin[k] = bounds ? bounds[k] : 0.f;
        cam.bmax[k] = bounds ? bounds[3 + k] : 0.f;
    }
    cam.H = H; cam.W = W;
    cam.bdev = bounds_dev;
    const int n = H * W;
    int err = 0;
    const size_t tb = gen_rays_temp_bytes(n);
    int* pix = c->buf<int>("ray_pix", (size_t)n + 1, &err);
    void* temp = c->buf<char>("ray_tmp", tb ? tb : 16, &err);
    RA_CHECK(!err, "ra_gen_rays: out of device memory");
    int* count_dev = pix + n;
    RA_CHECK(launch_gen_rays(cam, (unsigned char*)mask_at_box, pix, count_dev, temp, tb, (float*)ray_o, (float*)ray_d, (float*)near,
                             (float*)far, s) == 0, "ra_gen_rays: device selection failed");
    if (n_rays_dev) RA_HIP(hipMemcpyAsync(n_rays_dev, count_dev, sizeof(int), hipMemcpyDeviceToDevice, s));     // for a caller that reads it back later
    if (n_rays) {           // the count on the host costs a synchronisation; a caller that knows it (an unbounded box: H * W) passes NULL
        RA_HIP(hipMemcpyAsync(n_rays, count_dev, sizeof(int), hipMemcpyDeviceToHost, s));
        RA_HIP(hipStreamSynchronize(s));
    }
    return 0;
}

}  // extern "C"

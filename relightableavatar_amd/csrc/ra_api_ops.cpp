// C ABI: the stateless and thin entry points (include/relightableavatar.h) — re-shading, the material heads and regularisers, the
// per-frame body state, ray generation, images, metrics, LPIPS and the row gathers.  Each checks its arguments and enqueues a kernel
// or two; the render hot path is ra_api.cpp, and the mesh-side domains have a file each (ra_api_mesh, _topo, _cloth, _raster, _mcubes).
#include "ra_api_impl.hpp"
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

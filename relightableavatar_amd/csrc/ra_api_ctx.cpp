// C ABI, the context itself (include/relightableavatar.h): lifecycle and ownership, configuration, weights with the K3CC self-test,
// the frame, the gate, counters and timing.  The render hot path is ra_api.cpp.
#include "ra_api_impl.hpp"
#include <cstdio>
#include <memory>
#include <mutex>

static thread_local std::string g_err;
void ra_set_error(const std::string& msg) { g_err = msg; }

int DevBuf::ensure(size_t need) {
    if (need <= bytes && p) return 0;
    if (need == 0) need = 16;
    if (p) { hipDeviceSynchronize(); hipFree(p); p = nullptr; bytes = 0; }
    size_t want = need + need / 8 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) { ra_set_error(std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e)); p = nullptr; return 1; }
    bytes = want;
    return 0;
}
void DevBuf::release() { if (p) hipFree(p); p = nullptr; bytes = 0; }

ra_ctx::~ra_ctx() {
    for (auto& e : ev_pool) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    for (int k = 0; k < PinRing::n; ++k) if (pin.ev[k]) hipEventDestroy(pin.ev[k]);
    for (HintSlot& h : hints) { if (h.ev) hipEventDestroy(h.ev); if (h.host) hipHostFree(h.host); }
    if (pin.base) hipHostFree(pin.base);
}

extern "C" {

const char* ra_last_error(void) { return g_err.c_str(); }
int ra_abi_version(void) { return RA_ABI_VERSION; }

int ra_ctx_create(ra_ctx** out, int device) {
    RA_CHECK(out, "ra_ctx_create: null out");
    int n = 0;
    RA_HIP(hipGetDeviceCount(&n));
    RA_CHECK(n > 0, "ra_ctx_create: no HIP device visible (the render path has no CPU fallback)");
    RA_CHECK(device >= 0 && device < n, "ra_ctx_create: bad device index");
    RA_HIP(hipSetDevice(device));
    std::unique_ptr<ra_ctx> c(new ra_ctx());
    c->device = device;
    if (c->dcounters.ensure(1024)) return 1;
    RA_HIP(hipMemset(c->dcounters.p, 0, 1024));
    *out = c.release();
    return 0;
}

int ra_gate_create(ra_gate** out, int device) {
    RA_CHECK(out, "ra_gate_create: null out");
    RA_HIP(hipSetDevice(device));
    std::unique_ptr<ra_gate> g(new ra_gate());
    g->device = device;
    if (hipEventCreateWithFlags(&g->done, hipEventDisableTiming) != hipSuccess) { g->done = nullptr; ra_set_error("ra_gate_create: hipEventCreate failed"); return 1; }
    *out = g.release();
    return 0;
}
int ra_gate_destroy(ra_gate* g) {
    if (!g) return 0;
    hipSetDevice(g->device);
    hipDeviceSynchronize();
    delete g;
    return 0;
}
int ra_set_gate(ra_ctx* c, ra_gate* g) {
    RA_CHECK(c, "ra_set_gate: null context");
    RA_CHECK(!g || g->device == c->device, "ra_set_gate: gate and context live on different devices");
    c->gate = g;
    return 0;
}

int ra_ctx_destroy(ra_ctx* c) {
    if (!c) return 0;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    delete c;
    return 0;
}

int ra_default_config(ra_config* o) {
    RA_CHECK(o, "ra_default_config: null argument");
    *o = ra_config{};
    o->xyz_res = 10; o->sdf_res = 8; o->view_res = 4; o->n_bones = 52; o->relight = 1;
    o->resd_limit = 0.05f; o->blend_radius = 0.075f;
    o->albedo_slope = 1.f; o->albedo_bias = 0.f; o->roughness_slope = 0.9f; o->roughness_bias = 0.09f;
    o->fresnel_f0 = 0.02f; o->shading_albedo = 0.8f; o->albedo_multiplier = 1.f;
    o->tonemapping = 1; o->bg_brightness = 0.f; o->mlp_f16 = 1; o->query_skip = 1; o->k4_batch_slots = 0;
    o->trace_precision = 1; o->clip_near = 0.02f; o->clip_far = 10.f;
    o->only_visibility = 0; o->vis_shade_map = 0; o->use_geodesic_filter = 1;
    o->key_light_share = 0.0078f;
    return 0;
}

int ra_set_config(ra_ctx* c, const ra_config* cfg) {
    RA_CHECK(c && cfg, "ra_set_config: null argument");
    RA_CHECK(cfg->n_bones > 0 && cfg->n_bones <= 256, "ra_set_config: bad n_bones");
    RA_CHECK(cfg->trace_precision >= 0 && cfg->trace_precision <= 2, "ra_set_config: trace_precision must be 0, 1 or 2 (a zero-initialised ra_config is not the default: ra_default_config)");
    RA_CHECK(cfg->clip_far > cfg->clip_near, "ra_set_config: clip_far must exceed clip_near (a zero-initialised ra_config is not the default: ra_default_config)");
    RA_CHECK(cfg->vis_shade_map >= 0 && cfg->vis_shade_map <= 2, "ra_set_config: vis_shade_map must be 0, 1 or 2");
    RA_CHECK(cfg->key_light_share >= 0.f && cfg->key_light_share <= 1.f, "ra_set_config: key_light_share must be a fraction in [0, 1] (0 = no key-light tier)");
    c->cfg = *cfg;
    c->have_cfg = true;
    return 0;
}

int ra_set_weight(ra_ctx* c, const char* name, const float* data, size_t numel) {
    RA_CHECK(c && name && (data || numel == 0), "ra_set_weight: null argument");
    c->state_dict[name] = std::vector<float>(data, data + numel);
    c->have_weights = false;
    return 0;
}

static int upload(DevBuf& b, const void* src, size_t bytes, hipStream_t s) {
    if (b.ensure(bytes)) return 1;
    if (bytes) RA_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s));
    return 0;
}

// K3CC (csrc/ra_k3cc.hpp) keeps 62 weight fragments in flight in AGPRs it addresses by name; that is safe only while the compiler writes no
// AGPR of its own in that kernel — checked on the shipped object's assembly at build time (csrc/Makefile, tools/check_k3cc_isa.py) and
// HERE, on the device: a few hundred points through K3CC and through K3C's 4-wave tiles (the same arithmetic, weights through LDS) must
// agree bit for bit.  On a mismatch the context never launches K3CC (launch_mlp_sdf_comp allow_coop = false) and says so once on stderr.
// The answer is a property of the kernel's code on this device, not of the weights: one test per process and device.
static std::mutex k3cc_mu;
static std::map<int, bool> k3cc_result;
static int k3cc_self_test(ra_ctx* c, hipStream_t s) {
    {
        std::lock_guard<std::mutex> lk(k3cc_mu);
        auto it = k3cc_result.find(c->device);
        if (it != k3cc_result.end()) { c->k3cc_ok = it->second; return 0; }
    }
    constexpr int N = 400;                    // 25 tiles of 16 points, the last tile of K3C's 64-point tiles partly filled
    std::vector<float> x(3 * N);
    unsigned u = 12345u;
    for (float& v : x) { u = u * 1664525u + 1013904223u; v = ((u >> 8) * (1.f / 16777216.f) - 0.5f) * 0.9f; }
    std::vector<int> idx(N);
    for (int i = 0; i < N; ++i) idx[i] = i;
    DevBuf bx, bi, bc, ba, bb, bz;
    if (bx.ensure(x.size() * 4) || bi.ensure(N * 4) || bc.ensure(4) || ba.ensure(N * 4) || bb.ensure(N * 4) || bz.ensure(2048)) return 1;
    RA_HIP(hipMemcpyAsync(bx.p, x.data(), x.size() * 4, hipMemcpyHostToDevice, s));
    RA_HIP(hipMemcpyAsync(bi.p, idx.data(), N * 4, hipMemcpyHostToDevice, s));
    const int n = N;
    RA_HIP(hipMemcpyAsync(bc.p, &n, 4, hipMemcpyHostToDevice, s));
    RA_HIP(hipMemsetAsync(ba.p, 0xff, N * 4, s));
    RA_HIP(hipMemsetAsync(bb.p, 0, N * 4, s));
    RA_HIP(hipMemsetAsync(bz.p, 0, 2048, s));
    FrameState f{};
    f.bias_r0 = bz.as<float>(); f.bias_r4 = bz.as<float>() + 256;          // no frame yet: zero pose biases
    MlpIO io{};
    io.bpts = bx.as<float>(); io.idx = bi.as<int>(); io.count = bc.as<int>(); io.dist_th = 1.f; io.smooth = 0; io.resd_limit = c->cfg.resd_limit;
    io.sdf = ba.as<float>();
    launch_mlp_sdf_comp(c->host.geo, c->sarena_c.p, c->barena.as<float>(), f, io, N, s, true);
    io.sdf = bb.as<float>();
    launch_mlp_sdf_comp(c->host.geo, c->sarena_c.p, c->barena.as<float>(), f, io, N, s, false);
    std::vector<unsigned> a(N), b(N);
    RA_HIP(hipMemcpyAsync(a.data(), ba.p, N * 4, hipMemcpyDeviceToHost, s));
    RA_HIP(hipMemcpyAsync(b.data(), bb.p, N * 4, hipMemcpyDeviceToHost, s));
    RA_HIP(hipStreamSynchronize(s));
    RA_HIP(hipGetLastError());
    c->k3cc_ok = a == b;
    if (!c->k3cc_ok)
        fprintf(stderr, "relightableavatar: K3CC self-test failed (its distances differ from K3C's): the cooperative small-launch kernel is disabled on device %d (ra_k3cc_enabled)\n", c->device);
    std::lock_guard<std::mutex> lk(k3cc_mu);
    k3cc_result[c->device] = c->k3cc_ok;
    return 0;
}

int ra_k3cc_enabled(const ra_ctx* c) { return c && c->have_weights && c->k3cc_ok ? 1 : 0; }

int ra_finalize_weights(ra_ctx* c, void* stream) {
    RA_CHECK(c && c->have_cfg, "ra_finalize_weights: call ra_set_config first");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    std::string err;
    if (ra_pack_weights(c, err)) { ra_set_error("ra_finalize_weights: " + err); return 1; }
    HostNets& H = c->host;
    if (upload(c->sarena, H.sarena_trim.data(), H.sarena_trim.size() * 2, s)) return 1;        // device copy: the trimmed stream (8-wave K3)
    if (upload(c->sarena_pairs, H.sarena_pairs.data(), H.sarena_pairs.size() * 2, s)) return 1;
    if (upload(c->sarena_c, H.sarena_c.data(), H.sarena_c.size() * 2, s)) return 1;
    if (upload(c->fwd_arena, H.fwd_arena.data(), H.fwd_arena.size() * 2, s)) return 1;
    if (upload(c->bwd_arena, H.bwd_arena.data(), H.bwd_arena.size() * 2, s)) return 1;
    if (upload(c->shead_row, H.shead_row.data(), H.shead_row.size() * 4, s)) return 1;
    if (upload(c->barena, H.barena.data(), H.barena.size() * 4, s)) return 1;
    if (upload(c->cond_r0, H.cond_r0.data(), H.cond_r0.size() * 4, s)) return 1;
    if (upload(c->cond_r4, H.cond_r4.data(), H.cond_r4.size() * 4, s)) return 1;
    if (upload(c->b_r0, H.b_r0.data(), H.b_r0.size() * 4, s)) return 1;
    if (upload(c->b_r4, H.b_r4.data(), H.b_r4.size() * 4, s)) return 1;
    if (H.has_color) {
        if (upload(c->cond_c3, H.cond_c3.data(), H.cond_c3.size() * 4, s)) return 1;
        if (upload(c->b_c3, H.b_c3.data(), H.b_c3.size() * 4, s)) return 1;
    }
    if (c->cfg.relight) {
        c->n_lights = (int)H.light_area.size();
        if (upload(c->light_xyz, H.light_xyz.data(), H.light_xyz.size() * 4, s)) return 1;        // the current positions: the loaded ones again
        if (upload(c->light_xyz_loaded, H.light_xyz.data(), H.light_xyz.size() * 4, s)) return 1;
        if (upload(c->light_area, H.light_area.data(), H.light_area.size() * 4, s)) return 1;
        if (upload(c->light_sharp, H.light_sharp.data(), H.light_sharp.size() * 4, s)) return 1;
        if (c->light_dir.ensure(H.light_xyz.size() * 4)) return 1;
        launch_light_dirs(c->light_xyz.as<float>(), c->n_lights, c->light_dir.as<float>(), s);
    }
    RA_HIP(hipStreamSynchronize(s));     // host staging vectors may be reused
    if (k3cc_self_test(c, s)) return 1;
    c->have_weights = true;
    return 0;
}

int ra_set_frame(ra_ctx* c, const ra_frame* f, void* stream) {
    RA_CHECK(c && f, "ra_set_frame: null argument");
    RA_CHECK(c->have_weights, "ra_set_frame: weights not finalized");
    RA_CHECK(f->R && f->Th && f->poses && f->A && f->big_A && f->pverts && f->pnorm && f->tverts && f->weights, "ra_set_frame: null frame array");
    RA_CHECK(f->n_verts >= 3, "ra_set_frame: need at least 3 vertices (K=3 neighbours)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    const int nv = f->n_verts, nb = c->cfg.n_bones, cond = nb * 3;
    if (c->fvertA.ensure((size_t)nv * 24 * 4) || c->fpverts4.ensure((size_t)nv * 16) || c->fbias_r0.ensure(1024) || c->fbias_r4.ensure(1024) ||
        c->fbias_c3.ensure(1024))
        return 1;
    // R, Th, pnorm, tverts are read in place: the caller keeps the frame's arrays alive and unchanged until the next ra_set_frame
    // (include/relightableavatar.h) — four copy launches less per frame
    launch_pack_verts(f->pverts, nv, c->fpverts4.as<float4>(), s);
    launch_vert_blend(f->weights, f->A, f->big_A, nv, nb, c->fvertA.as<float>(), s);
    const int nleaf = c->use_bvh ? bvh_leaf_count(nv) : 0;
    const int nsuper = bvh_super_count(nleaf);
    if (nleaf > 0) {
        // leaves: 512 B each; boxes: super boxes (lo | hi), then per super box the four pair records of its leaf boxes
        if (c->fbvh_pts.ensure((size_t)nleaf * 32 * 16) || c->fbvh_pairs.ensure((size_t)nsuper * (32 + 192)) || c->fbvh_order.ensure((size_t)nv * 4)) return 1;
        launch_bvh_build(c->fpverts4.as<float4>(), nv, c->fbvh_order.as<int>(), c->fbvh_pts.as<float>(), c->fbvh_pairs.as<float4>(), nleaf, nsuper, s);
        RA_HIP(hipGetLastError());
    }
    launch_fold_bias(c->cond_r0.as<float>(), cond, 0, cond, f->poses, c->b_r0.as<float>(), c->fbias_r0.as<float>(), s);
    launch_fold_bias(c->cond_r4.as<float>(), cond, 0, cond, f->poses, c->b_r4.as<float>(), c->fbias_r4.as<float>(), s);
    if (c->host.has_color && f->cond_fix)
        launch_fold_bias(c->cond_c3.as<float>(), cond, 0, cond, f->cond_fix, c->b_c3.as<float>(), c->fbias_c3.as<float>(), s);
    FrameState& fr = c->fr;
    fr.R = (float*)f->R; fr.Th = (float*)f->Th; fr.vertA = c->fvertA.as<float>(); fr.pverts4 = c->fpverts4.as<float4>();
    fr.pnorm = (float*)f->pnorm; fr.tverts = (float*)f->tverts; fr.bias_r0 = c->fbias_r0.as<float>();
    fr.bias_r4 = c->fbias_r4.as<float>(); fr.bias_c3 = c->fbias_c3.as<float>(); fr.n_verts = nv;
    fr.bvh_soa = c->fbvh_pts.as<float>();
    fr.bvh_sbox = c->fbvh_pairs.as<float4>(); fr.bvh_lpair = reinterpret_cast<const float*>(fr.bvh_sbox + (size_t)2 * nsuper); fr.bvh_leaves = nleaf; fr.bvh_supers = nsuper;
    c->have_frame = true;
    c->call_no = 0;             // render calls are numbered from here (launch-variant hints, ra_ctx.hpp HintSlot)
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_get_counters(ra_ctx* c, ra_counters* out, void* stream) {
    RA_CHECK(c && out, "ra_get_counters: null argument");
    RA_HIP(hipSetDevice(c->device));
    RA_HIP(hipStreamSynchronize((hipStream_t)stream));
    unsigned long long h[8];
    RA_HIP(hipMemcpy(h, c->dcounters.p, sizeof(h), hipMemcpyDeviceToHost));
    out->n_coarse = h[0];
    out->n_fine_sdf = h[1];
    out->n_fine_full = h[2];
    out->n_shadow_rays = h[3];
    out->n_hit_pixels = h[4];
    out->n_shaded = c->n_shaded + h[4];
    out->n_fine_sdf_wide = h[5];
    out->n_fine_sdf_comp = h[6];
    return 0;
}

int ra_reset_counters(ra_ctx* c, void* stream) {
    RA_CHECK(c, "ra_reset_counters: null ctx");
    RA_HIP(hipSetDevice(c->device));
    RA_HIP(hipStreamSynchronize((hipStream_t)stream));
    RA_HIP(hipMemset(c->dcounters.p, 0, 64));
    c->n_shaded = 0;
    c->ev_used = 0;
    return 0;
}

int ra_set_knn_mode(ra_ctx* c, int use_bvh) {
    RA_CHECK(c, "ra_set_knn_mode: null ctx");
    c->use_bvh = use_bvh != 0;
    c->have_frame = false;      // takes effect at the next ra_set_frame
    return 0;
}

int ra_enable_timing(ra_ctx* c, int on) {
    RA_CHECK(c, "ra_enable_timing: null ctx");
    c->timing = on != 0;
    return 0;
}

// the kinds ra_get_kernel_time reports (include/relightableavatar.h: 0 every K3, 1 K4, 2 the 8-wave K3, 3 the narrow K3, 4 K3C) in terms
// of what a Timer recorded
static bool kind_counts(int kind, TimerKind k) {
    static const unsigned of_kind[5] = {1u << T_K3_WIDE | 1u << T_K3_NARROW, 1u << T_K4, 1u << T_K3_WIDE, 1u << T_K3_NARROW, 1u << T_K3C};
    return (of_kind[kind] >> k) & 1u;
}

int ra_get_kernel_time(ra_ctx* c, int kind, float* ms, int* n_launches, void* stream) {
    RA_CHECK(c && ms && n_launches, "ra_get_kernel_time: null argument");
    RA_CHECK(kind >= 0 && kind <= 4, "ra_get_kernel_time: kind must be 0 (distance query), 1 (full query), 2 (8-wave distance query), 3 (narrow distance query) or 4 (compensated distance query)");
    RA_HIP(hipSetDevice(c->device));
    RA_HIP(hipStreamSynchronize((hipStream_t)stream));
    float tot = 0.f;
    int n = 0;
    for (size_t i = 0; i < c->ev_used; ++i) {
        if (!kind_counts(kind, c->ev_kind[i])) continue;
        float t = 0.f;
        if (hipEventElapsedTime(&t, c->ev_pool[i].first, c->ev_pool[i].second) == hipSuccess) { tot += t; ++n; }
    }
    *ms = tot;
    *n_launches = n;
    return 0;
}

int ra_get_mlp_time(ra_ctx* c, float* ms, int* n_launches, void* stream) { return ra_get_kernel_time(c, 0, ms, n_launches, stream); }

}  // extern "C"

// C ABI: the ra_debug_* test hooks (include/relightableavatar.h) — stage outputs for the parity tests, not used by the renderers.
#include "ra_api_impl.hpp"
#include <cstdlib>
#include <cstring>

extern "C" {

int ra_debug_key_lights(ra_ctx* c, unsigned char* key_dev, float* share_dev, void* stream) {
    RA_CHECK(c && key_dev && share_dev, "ra_debug_key_lights: null argument");
    RA_CHECK(c->key_valid && c->n_lights > 0, "ra_debug_key_lights: no key lights have been computed (ra_set_key_probes, or a render call with a probe)");
    RA_HIP(hipSetDevice(c->device));
    RA_HIP(hipMemcpyAsync(key_dev, c->key_mask.p, (size_t)c->n_lights, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    RA_HIP(hipMemcpyAsync(share_dev, c->key_share.p, (size_t)c->n_lights * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int ra_debug_mlp(ra_ctx* c, const float* bpts, int n, float* resd, float* sdf, float* feat, void* stream) {
    // stage outputs of the geometry networks from the PRODUCTION forward kernel of the full query (K4 forward with tape)
    if (check_ready(c, "ra_debug_mlp")) return 1;
    if (n <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int err = 0;
    int* idx = c->buf<int>("fine_idx", n, &err);
    char* tape = c->buf<char>("k4_tape", mlp_full_rev_tape_bytes(n), &err);
    if (err) return 1;
    int* cnt = next_fine_counter(c, s);
    launch_iota(idx, n, cnt, s);
    FullIO io = full_io(c);
    io.bpts = bpts; io.idx = idx; io.count = cnt; io.slot0 = 0; io.slot_cap = n;
    io.dbg_resd = resd; io.dbg_sdf = sdf; io.dbg_feat = feat; io.dbg_layer = -1; io.counters = nullptr;
    k4_fwd_launch(c, io, tape, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_debug_full(ra_ctx* c, const float* bpts, int n, float* grad, float* sdf, float* feat, float* raw, void* stream) {
    if (check_ready(c, "ra_debug_full")) return 1;
    if (n <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int err = 0;
    int* cnt = next_fine_counter(c, s);
    int* idx = c->buf<int>("fine_idx", n, &err);
    float* view = c->buf<float>("dbg_view", (size_t)n * 3, &err);
    if (err) return 1;
    launch_iota(idx, n, cnt, s);
    RA_HIP(hipMemsetAsync(view, 0, (size_t)n * 12, s));
    FullIO io = full_io(c);
    io.bpts = bpts; io.mats = nullptr; io.view = view; io.idx = idx; io.count = cnt; io.raw = raw;
    io.dbg_grad = grad; io.dbg_sdf = sdf; io.dbg_feat = feat; io.counters = nullptr;
    io.dbg_layer = -1;
#ifdef RA_TESTING            // debugging aids of tools/dbg_grad.py (test builds only)
    if (getenv("RA_DBG_GC")) { io.dbg_gc = grad; io.dbg_grad = nullptr; }       // d sdf / d cpts instead
    if (getenv("RA_DBG_LAYER")) io.dbg_layer = atoi(getenv("RA_DBG_LAYER"));
    if (getenv("RA_DBG_PE")) { io.dbg_pe = feat; io.dbg_feat = nullptr; RA_HIP(hipMemsetAsync(feat, 0, (size_t)n * 256 * 4, s)); }   // encoding-slot gradients in feat[:, :128]
#endif
    if (full_query(c, io, n, s)) return 1;
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_debug_aabb(ra_ctx* c, const float* o, const float* d, int n, const float* bbox, float* nr, float* fr, void* stream) {
    RA_CHECK(c && n >= 0 && (n == 0 || (o && d && bbox && nr && fr)), "ra_debug_aabb: bad arguments");
    RA_HIP(hipSetDevice(c->device));
    launch_debug_aabb(o, d, n, bbox, nr, fr, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}
int ra_debug_lvis(ra_ctx* c, const float* surf, const float* norm, const float* acc, int n, const float* bbox, const ra_trace_params* shadow,
                  float near_offset, float* lvis_out, float* ldot_out, void* stream) {
    if (check_ready(c, "ra_debug_lvis")) return 1;
    RA_CHECK(c->cfg.relight && c->n_lights > 0, "ra_debug_lvis: needs the relight network's light set");
    RA_CHECK(n >= 0 && shadow && (n == 0 || (surf && norm && acc && bbox && lvis_out && ldot_out)), "ra_debug_lvis: bad arguments");
    if (n == 0) return 0;
    ra_sphere_params p{};
    p.shadow = *shadow; p.shadow_near_offset = near_offset;
    // every point its own hit slot; no probe here: every ray in the plain tier (unless ra_set_key_probes named the key lights)
    return ra_light_visibility(c, surf, norm, acc, n, nullptr, 0, bbox, nullptr, 0, 0, &p, lvis_out, ldot_out, stream);
}
int ra_debug_brdf(ra_ctx* c, const float* p2l, const float* p2c, const float* normal, const float* albedo, const float* rough, int L, int N,
                  float* brdf, void* stream) {
    RA_CHECK(c && c->have_cfg, "ra_debug_brdf: call ra_set_config first");
    RA_CHECK(L >= 0 && N >= 0 && (L * N == 0 || (p2l && p2c && normal && albedo && rough && brdf)), "ra_debug_brdf: bad arguments");
    RA_HIP(hipSetDevice(c->device));
    launch_debug_brdf(p2l, p2c, normal, albedo, rough, L, N, c->cfg, brdf, (hipStream_t)stream);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_debug_bvh_ids(ra_ctx* c, int* ids_host, int capacity, int* n_out, void* stream) {
    if (check_ready(c, "ra_debug_bvh_ids")) return 1;
    RA_CHECK(ids_host && n_out && capacity >= 0, "ra_debug_bvh_ids: bad arguments");
    const int nleaf = c->fr.bvh_leaves;
    *n_out = nleaf * 32;
    if (nleaf == 0) return 0;
    RA_CHECK(capacity >= nleaf * 32, "ra_debug_bvh_ids: capacity too small");
    hipStream_t s = (hipStream_t)stream;
    std::vector<float> leaves((size_t)nleaf * 128);
    RA_HIP(hipMemcpyAsync(leaves.data(), c->fr.bvh_soa, leaves.size() * 4, hipMemcpyDeviceToHost, s));
    RA_HIP(hipStreamSynchronize(s));
    for (int l = 0; l < nleaf; ++l) memcpy(ids_host + (size_t)l * 32, leaves.data() + (size_t)l * 128 + 96, 32 * 4);
    return 0;
}

int ra_debug_hdq(ra_ctx* c, const float* x, int n, float th, float* sdf_coarse, float* sdf_batch, int* nn_batch, float* d2,
                 float* bpts, float* tpts, float* mats, int* fine_count_host, void* stream) {
    if (check_ready(c, "ra_debug_hdq")) return 1;
    if (n <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int err = 0;
    int* fine_idx = c->buf<int>("fine_idx", n, &err);
    float* fb = c->buf<float>("fine_bpts", (size_t)n * 3, &err);
    if (err) return 1;
    RaySet rs{};
    rs.mode = 0; rs.x = x;
    HdqOut out{};
    out.sdf = sdf_coarse; out.fine_count = next_fine_counter(c, s); out.fine_idx = fine_idx; out.bpts = fb;
    out.dbg_sdf_batch = sdf_batch; out.dbg_nn_batch = nn_batch; out.dbg_d2 = d2; out.dbg_bpts = bpts; out.dbg_tpts = tpts; out.dbg_mats = mats;
    out.counters = dcnt(c);
    RA_HIP(hipMemsetAsync(bpts, 0, (size_t)n * 12, s));
    RA_HIP(hipMemsetAsync(tpts, 0, (size_t)n * 12, s));
    RA_HIP(hipMemsetAsync(mats, 0, (size_t)n * 96, s));
    launch_hdq_coarse(c->fr, rs, n, th, c->cfg.blend_radius, out, s, c->cfg.use_geodesic_filter != 0);
    RA_HIP(hipStreamSynchronize(s));
    RA_HIP(hipMemcpy(fine_count_host, out.fine_count, sizeof(int), hipMemcpyDeviceToHost));
    RA_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

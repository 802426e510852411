// C ABI: orchestration of the render hot path (include/relightableavatar.h) — the distance and full queries, the sphere trace, the
// light-visibility stage and the three render chunks.  The context itself is ra_api_ctx.cpp, the thin entry points ra_api_ops.cpp,
// the mesh-side domains ra_api_mesh, _topo, _cloth, _raster and _mcubes.cpp, the test hooks ra_api_debug.cpp.
// Every entry point only enqueues work on the caller's stream; counts that steer later passes
// (fine points, hit pixels, shadow rays) stay on the device and kernels size themselves from them.
#include "ra_api_impl.hpp"
#include <cmath>

int check_ready(ra_ctx* c, const char* who) {
    if (!c) { ra_set_error(std::string(who) + ": null ctx"); return 1; }
    if (!c->have_weights) { ra_set_error(std::string(who) + ": weights not finalized"); return 1; }
    if (!c->have_frame) { ra_set_error(std::string(who) + ": no frame set (ra_set_frame)"); return 1; }
    if (hipSetDevice(c->device) != hipSuccess) { ra_set_error(std::string(who) + ": hipSetDevice failed"); return 1; }
    return 0;
}

// Every hierarchical-distance pass compacts its fine points through a device counter that must start at zero.  Instead of one
// 4-byte memset launch per pass (21 per relit chunk), the counters are a set that ONE memset zeroes per chunk; each pass takes
// the next unused slot.  Stream order makes the refill safe: the memset runs after every earlier user.
static void zero_chunk_counters(ra_ctx* c, hipStream_t s) {
    hipMemsetAsync(icnt(c, 0), 0, CNT_ALL * sizeof(int), s);
    c->fc_next = 0;
    c->fc_wrapped = false;
    c->cnt_zero = true;
}
int* next_fine_counter(ra_ctx* c, hipStream_t s) {
    if (c->fc_next >= CNT_FC_SLOTS) {
        hipMemsetAsync(icnt(c, CNT_FC0), 0, CNT_FC_SLOTS * sizeof(int), s);
        c->fc_next = 0;
        c->fc_wrapped = true;           // slots are being reused: no hints from or for this call
    }
    return icnt(c, CNT_FC0 + c->fc_next++);
}

namespace {

struct Timer {
    ra_ctx* c; hipStream_t s; TimerKind kind; hipEvent_t a = nullptr, b = nullptr;
    Timer(ra_ctx* c_, hipStream_t s_, TimerKind kind_) : c(c_), s(s_), kind(kind_) {
        if (!c->timing) return;
        if (c->ev_used == c->ev_pool.size()) {
            hipEvent_t x, y;
            hipEventCreate(&x); hipEventCreate(&y);
            c->ev_pool.push_back({x, y});
            c->ev_kind.push_back(kind);
        }
        c->ev_kind[c->ev_used] = kind;
        a = c->ev_pool[c->ev_used].first; b = c->ev_pool[c->ev_used].second;
        c->ev_used++;
        hipEventRecord(a, s);
    }
    ~Timer() { if (a) hipEventRecord(b, s); }
};

// one render call's window on the hints (ra_ctx.hpp HintSlot): construction picks the slot of this call and harvests the counts an earlier
// frame left there; destruction queues the copy of this call's fine-count slots behind an event
struct HintScope {
    ra_ctx* c; hipStream_t s;
    HintScope(ra_ctx* c_, hipStream_t s_) : c(c_), s(s_) {
        const int k = c->call_no++;
        if (k >= 64) { c->cur_hint = nullptr; return; }
        if ((int)c->hints.size() <= k) c->hints.resize(k + 1);
        HintSlot& h = c->hints[k];
        if (!h.ev) {
            if (hipEventCreateWithFlags(&h.ev, hipEventDisableTiming) != hipSuccess || hipHostMalloc((void**)&h.host, CNT_FC_SLOTS * sizeof(int)) != hipSuccess) {
                h.ev = nullptr; h.host = nullptr; c->cur_hint = nullptr; (void)hipGetLastError(); return;
            }
        }
        if (h.pending && hipEventQuery(h.ev) == hipSuccess) {
            h.vals.assign(h.host, h.host + h.n_pending);
            h.n_valid = h.n_pending;
            h.pending = false;
        }
        (void)hipGetLastError();            // hipEventQuery's hipErrorNotReady is not an error of the call
        c->cur_hint = &h;
    }
    ~HintScope() {
        HintSlot* h = c->cur_hint;
        c->cur_hint = nullptr;
        if (!h || h->pending || c->fc_next <= 0 || c->fc_wrapped) return;      // an unread copy is still in flight: keep it
        if (hipMemcpyAsync(h->host, icnt(c, CNT_FC0), (size_t)c->fc_next * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) return;
        if (hipEventRecord(h->ev, s) != hipSuccess) return;
        h->n_pending = c->fc_next;
        h->pending = true;
    }
};

// the fine count the pass that takes fine-count slot k found in an earlier frame (-1: unknown)
int fine_hint(const ra_ctx* c, int k) {
    const HintSlot* h = c->cur_hint;
    return (h && !c->fc_wrapped && k < h->n_valid) ? h->vals[k] : -1;
}
// the size the variant choice of a fused MLP launch sees: the bound, or — with a hint — a quarter more than the earlier count
// A hint comes from an EARLIER frame: after a camera cut the count can be many times larger.  Every variant is correct for every count
// (persistent over tiles), but a narrow variant on a grid sized for the hint would be a cliff: the hint picks the workgroup WIDTH only.
int variant_size(int n, int hint) {
    if (hint < 0) return n;
    const long long v = (long long)hint + hint / 4 + 1024;
    return v < n ? (int)v : n;
}
// ... and the size its grid is made for (mlp_grid, ra_common.hpp): never below an eighth of the bound, whatever the hint says
int grid_size(int n, int nv) { return nv > n / 8 ? nv : n / 8; }

void k3_launch(ra_ctx* c, const MlpIO& io, int n, hipStream_t s, int grid_slots = 0) {
    if (c->cfg.mlp_f16) launch_mlp_sdf_stream_f16(c->host.geo, c->sarena.p, c->sarena_pairs.p, c->barena.as<float>(), c->fr, io, n, s, grid_slots);
    else launch_mlp_sdf_stream_bf16(c->host.geo, c->sarena.p, c->sarena_pairs.p, c->barena.as<float>(), c->fr, io, n, s, grid_slots);
}

}  // namespace

void k4_fwd_launch(ra_ctx* c, const FullIO& io, char* tape, hipStream_t s) {
    if (c->cfg.mlp_f16) launch_mlp_fwd_tape_f16(c->host.geo, c->fwd_arena.p, c->barena.as<float>(), c->fr, io, tape, s);
    else launch_mlp_fwd_tape_bf16(c->host.geo, c->fwd_arena.p, c->barena.as<float>(), c->fr, io, tape, s);
}

FullIO full_io(ra_ctx* c) {
    FullIO io{};
    io.C = raw_channels(c);
    io.beta = c->host.beta; io.resd_limit = c->cfg.resd_limit;
    io.albedo_slope = c->cfg.albedo_slope; io.albedo_bias = c->cfg.albedo_bias;
    io.rough_slope = c->cfg.roughness_slope; io.rough_bias = c->cfg.roughness_bias;
    io.relight = c->cfg.relight;
    io.counters = dcnt(c);
    return io;
}

// which distance queries run in compensated arithmetic (ra_config.trace_precision): the surface trace from 1 on, everything at 2
// (the light-visibility rays towards the frame's key lights join them through hdq_pass's second fine list: ra_config.key_light_share)
enum { Q_OTHER = 0, Q_SURFACE = 1, Q_PRECISE = 2 };      // Q_PRECISE: compensated whatever the configuration says (mesh extraction)
static bool precise(const ra_ctx* c, int what) { return what == Q_PRECISE || c->cfg.trace_precision >= 2 || (c->cfg.trace_precision == 1 && what == Q_SURFACE); }
static constexpr int KEY_LIGHTS_MAX = 48;       // per frame; bounds the second ray list of a light-visibility stage (rays <= pixels x this) and the tier's cost
static bool key_tier(const ra_ctx* c) { return c->cfg.trace_precision == 1 && c->cfg.key_light_share > 0.f && c->n_lights > 0; }
// the frame's key-light flags from the probe a render call shades with — unless the caller named the frame's probes itself (ra_set_key_probes)
static int key_mask_from(ra_ctx* c, const float* probe, int ph, int pw, hipStream_t s) {
    if (c->key_external) return 0;
    c->key_valid = false;
    if (!key_tier(c) || !probe) return 0;
    if (c->key_mask.ensure((size_t)c->n_lights) || c->key_share.ensure((size_t)c->n_lights * sizeof(float))) return 1;
    launch_key_lights(probe, 1, ph, pw, c->light_dir.as<float>(), c->light_area.as<float>(), c->n_lights, c->cfg.key_light_share, KEY_LIGHTS_MAX, 0,
                      c->key_share.as<float>(), c->key_mask.as<unsigned char>(), s);
    c->key_valid = true;
    return 0;
}

// the fine level of one query: K3, or K3C where the pass is in the precise tier
// n: upper bound of the device-side count; hint: the count this pass found in an earlier frame (-1: none).  Every variant is correct for
// every count (persistent over tiles); the size only picks the workgroup width and the grid.
static void fine_level(ra_ctx* c, const MlpIO& io, int n, bool comp, hipStream_t s, int hint = -1) {
    const int nv = variant_size(n, hint);
    if (comp) {
        Timer t(c, s, T_K3C);
        launch_mlp_sdf_comp(c->host.geo, c->sarena_c.p, c->barena.as<float>(), c->fr, io, nv, s, c->k3cc_ok, grid_size(n, nv));
    } else {
        Timer t(c, s, k3_waves(nv) == 8 ? T_K3_WIDE : T_K3_NARROW);      // timed per kernel family
        k3_launch(c, io, nv, s, grid_size(n, nv));
    }
}

// one hierarchical distance query over the points of rs; writes sdf[n]
// key / n_key (the key-light tier; shadow rays only): the fine points of rays towards lights with key[light] != 0 — at most n_key — form
// a second fine list that the compensated kernel answers; the pass then is ONE coarse launch + K3 on the first list + K3C / K3CC on the second
static int hdq_pass(ra_ctx* c, const RaySet& rs, int n, float th, int smooth, float* sdf, hipStream_t s, int what = Q_OTHER,
                    const unsigned char* key = nullptr, int n_key = 0) {
    if (n <= 0) return 0;
    int err = 0;
    int* fine_idx = c->buf<int>("fine_idx", n, &err);
    float* bpts = c->buf<float>("fine_bpts", (size_t)n * 3, &err);
    if (err) return 1;
    HdqOut out{};
    out.sdf = sdf; out.fine_count = next_fine_counter(c, s); out.fine_idx = fine_idx; out.bpts = bpts;
    const int hint = fine_hint(c, c->fc_next - 1);
    int hint2 = -1;
    if (key && n_key > 0) {
        out.key = key;
        out.fine_idx2 = c->buf<int>("fine_idx_k", n_key, &err);
        out.bpts2 = c->buf<float>("fine_bpts_k", (size_t)n_key * 3, &err);
        if (err) return 1;
        out.fine_count2 = next_fine_counter(c, s);
        hint2 = fine_hint(c, c->fc_next - 1);
    }
    out.counters = dcnt(c);
    launch_hdq_coarse(c->fr, rs, n, th, c->cfg.blend_radius, out, s, c->cfg.use_geodesic_filter != 0);
    MlpIO io{};
    io.bpts = bpts; io.idx = fine_idx; io.count = out.fine_count; io.sdf = sdf; io.dist_th = th; io.smooth = smooth;
    io.resd_limit = c->cfg.resd_limit; io.counters = dcnt(c);
    fine_level(c, io, n, precise(c, what), s, hint);
    if (out.key) {
        io.bpts = out.bpts2; io.idx = out.fine_idx2; io.count = out.fine_count2;
        fine_level(c, io, n_key, true, s, hint2);
    }
    return 0;
}

// the full query on the compacted fine list: forward with tape + reverse-mode backward + heads, in sub-batches of
// cfg.k4_batch_slots fine slots that share ONE tape (4.9 KB per slot).  n is only the upper bound of the device-side
// count: launch pairs beyond it find no tile and exit at once.
int full_query(ra_ctx* c, FullIO io, int n, hipStream_t s) {
    // frames in flight: a full query that fills the chip (the volume path's) takes its turn at the gate like a light-visibility stage
    const bool gated = c->gate && n > 65536;
    if (gated && c->gate->armed) RA_HIP(hipStreamWaitEvent(s, c->gate->done, 0));
    struct Release {
        ra_ctx* c; hipStream_t s; bool on;
        ~Release() { if (on) { hipEventRecord(c->gate->done, s); c->gate->armed = true; } }
    } release{c, s, gated};
    Timer t(c, s, T_K4);
    const int batch = c->cfg.k4_batch_slots > 0 ? c->cfg.k4_batch_slots : (1 << 20);
    const int cap = n < batch ? n : batch;
    int err = 0;
    char* tape = c->buf<char>("k4_tape", mlp_full_rev_tape_bytes(cap), &err);
    if (err) {
        ra_set_error("full query: no device memory for the activation tape (" + std::to_string(mlp_full_rev_tape_bytes(cap) >> 20) +
                     " MB): lower cfg.k4_batch_slots / cfg.volume_chunk_rays");
        return 1;
    }
    for (int s0 = 0; s0 < n; s0 += cap) {
        io.slot0 = s0;
        io.slot_cap = n - s0 < cap ? n - s0 : cap;
        k4_fwd_launch(c, io, tape, s);
        if (c->cfg.mlp_f16) launch_mlp_bwd_heads_f16(c->host.mat, c->host.col, c->bwd_arena.p, c->barena.as<float>(), c->shead_row.as<float>(), c->fr, io, tape, s);
        else launch_mlp_bwd_heads_bf16(c->host.mat, c->host.col, c->bwd_arena.p, c->barena.as<float>(), c->shead_row.as<float>(), c->fr, io, tape, s);
    }
    return 0;
}

// Network.forward (eval) on n (or *n_dev) points: raw[n][C], zero for non-fine points
static int forward_pass(ra_ctx* c, const float* x, const float* v, int n, const int* n_dev, float th, float* raw, hipStream_t s) {
    if (n <= 0) return 0;
    int err = 0;
    const int C = raw_channels(c);
    int* fine_idx = c->buf<int>("fine_idx", n, &err);
    float* bpts = c->buf<float>("fine_bpts", (size_t)n * 3, &err);
    float* mats = c->buf<float>("fine_mats", (size_t)n * 24, &err);
    float* sdf = c->buf<float>("fwd_sdf", n, &err);
    if (err) return 1;
    RaySet rs{};
    rs.mode = 0; rs.x = x; rs.n_dev = n_dev;
    HdqOut out{};
    out.sdf = sdf; out.fine_count = next_fine_counter(c, s); out.fine_idx = fine_idx; out.bpts = bpts; out.mats = mats;
    out.raw_zero = raw; out.raw_C = C;          // points outside dist_th: zero rows, written by the coarse level itself
    out.counters = dcnt(c);
    launch_hdq_coarse(c->fr, rs, n, th, c->cfg.blend_radius, out, s, c->cfg.use_geodesic_filter != 0);
    FullIO io = full_io(c);
    io.bpts = bpts; io.mats = mats; io.view = v; io.idx = fine_idx; io.count = out.fine_count; io.raw = raw;
    return full_query(c, io, n, s);
}

static TraceState alloc_trace(ra_ctx* c, const std::string& p, int n, bool soft, int* err) {
    TraceState ts{};
    ts.t = c->buf<float>(p + "t", n, err);
    ts.d0 = c->buf<float>(p + "d0", n, err);
    ts.occ = c->buf<float>(p + "occ", n, err);
    ts.ot = c->buf<float>(p + "ot", n, err);
    ts.stuck = c->buf<unsigned char>(p + "stuck", n, err);
    if (!soft) {
        ts.dt = c->buf<float>(p + "dt", n, err);
        ts.st = c->buf<float>(p + "st", n, err);
        ts.cd = c->buf<float>(p + "cd", n, err);
        ts.off = c->buf<float>(p + "off", n, err);
        ts.rlx = c->buf<float>(p + "rlx", n, err);
    }
    return ts;
}

// The decoders of mesh extraction (ra_sdf_volume) on n (or fewer: *count on the device) points, always on the compensated tier: a
// vertex's position is a quotient of two neighbouring values.  mode 0: sdf(x), the canonical field — the distance query with
// resd_limit 0, so that its residual head contributes tanh(z) * 0 and cpts = x exactly; 1: sdf(x + resd(x)), what ra_observed_sdf
// computes; 2: the hierarchical query of world points without the smooth transition, what ra_hdq_sdf(smooth 0) computes.
int sdf_points_precise(ra_ctx* c, int mode, const float* pts, int n, float dist_th, float* sdf, hipStream_t s) {
    if (n <= 0) return 0;
    if (mode == 2) {
        RaySet rs{};
        rs.mode = 0; rs.x = pts;
        return hdq_pass(c, rs, n, dist_th, 0, sdf, s, Q_PRECISE);
    }
    int err = 0;
    int* idx = c->buf<int>("fine_idx", n, &err);
    if (err) return 1;
    int* cnt = next_fine_counter(c, s);
    launch_iota(idx, n, cnt, s);
    MlpIO io{};
    io.bpts = pts; io.idx = idx; io.count = cnt; io.sdf = sdf; io.dist_th = 1.f; io.smooth = 0;
    io.resd_limit = mode == 0 ? 0.f : c->cfg.resd_limit; io.counters = dcnt(c);
    fine_level(c, io, n, true, s);
    return 0;
}

extern "C" {

int ra_raw_channels(const ra_ctx* c) { return c ? raw_channels(c) : 16; }

int ra_hdq_sdf(ra_ctx* c, const float* x, int n, float dist_th, int smooth, float* sdf, void* stream) {
    if (check_ready(c, "ra_hdq_sdf")) return 1;
    RA_CHECK(n >= 0 && (n == 0 || (x && sdf)), "ra_hdq_sdf: bad arguments");
    RaySet rs{};
    rs.mode = 0; rs.x = x;
    if (hdq_pass(c, rs, n, dist_th, smooth, sdf, (hipStream_t)stream)) return 1;
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_observed_sdf(ra_ctx* c, const float* bpts, int n, float* sdf, void* stream) {
    if (check_ready(c, "ra_observed_sdf")) return 1;
    RA_CHECK(n >= 0 && (n == 0 || (bpts && sdf)), "ra_observed_sdf: bad arguments");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int err = 0;
    int* idx = c->buf<int>("fine_idx", n, &err);
    if (err) return 1;
    int* cnt = next_fine_counter(c, s);
    launch_iota(idx, n, cnt, s);
    MlpIO io{};
    io.bpts = bpts; io.idx = idx; io.count = cnt; io.sdf = sdf; io.dist_th = 1.f; io.smooth = 0;
    io.resd_limit = c->cfg.resd_limit; io.counters = dcnt(c);
    fine_level(c, io, n, precise(c, Q_OTHER), s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_bigpose_transform(ra_ctx* c, const float* x, int n, const float* R, const float* Th, int invert, float* out, void* stream) {
    if (check_ready(c, "ra_bigpose_transform")) return 1;
    RA_CHECK(n >= 0 && (n == 0 || (x && out && R && Th)), "ra_bigpose_transform: bad arguments");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int err = 0;
    int* fine_idx = c->buf<int>("fine_idx", n, &err);
    float* fb = c->buf<float>("fine_bpts", (size_t)n * 3, &err);
    float* sdfc = c->buf<float>("bt_sdf", n, &err);
    float* sb = c->buf<float>("bt_sdf_batch", (size_t)n * 3, &err);
    int* nb = c->buf<int>("bt_nn", (size_t)n * 3, &err);
    float* d2 = c->buf<float>("bt_d2", (size_t)n * 3, &err);
    float* bp = c->buf<float>("bt_bpts", (size_t)n * 3, &err);
    float* tp = c->buf<float>("bt_tpts", (size_t)n * 3, &err);
    float* mats = c->buf<float>("bt_mats", (size_t)n * 24, &err);
    if (err) return 1;
    RaySet rs{};
    rs.mode = 0; rs.x = x;
    HdqOut o{};
    o.sdf = sdfc; o.fine_count = next_fine_counter(c, s); o.fine_idx = fine_idx; o.bpts = fb;
    o.dbg_sdf_batch = sb; o.dbg_nn_batch = nb; o.dbg_d2 = d2; o.dbg_bpts = bp; o.dbg_tpts = tp; o.dbg_mats = mats;
    o.counters = dcnt(c);
    launch_hdq_coarse(c->fr, rs, n, 1e9f, c->cfg.blend_radius, o, s, c->cfg.use_geodesic_filter != 0);      // transform=False -> filtering off: dist = 1e9 (:253-259)
    launch_bigpose_compose(mats, d2, n, c->cfg.blend_radius, R, Th, invert, out, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_forward(ra_ctx* c, const float* x, const float* v, int n, float dist_th, float* raw, void* stream) {
    if (check_ready(c, "ra_forward")) return 1;
    RA_CHECK(n >= 0 && (n == 0 || (x && raw)), "ra_forward: bad arguments");
    RA_CHECK(c->cfg.relight || v || n == 0, "ra_forward: the AniSDF colour net needs view directions");
    if (forward_pass(c, x, v, n, nullptr, dist_th, raw, (hipStream_t)stream)) return 1;
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_sphere_trace(ra_ctx* c, const float* ray_o, const float* ray_d, const float* near_, const float* far_, const float* tan_i,
                    int n, const ra_trace_params* p, float* surf, float* occ, float* st, float* ot, void* stream) {
    if (check_ready(c, "ra_sphere_trace")) return 1;
    RA_CHECK(p && n >= 0 && (n == 0 || (ray_o && ray_d && near_ && far_)), "ra_sphere_trace: bad arguments");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int err = 0;
    TraceState ts = alloc_trace(c, "tr_", n, false, &err);   // full state for either mode
    float* sdf = c->buf<float>("tr_sdf", n, &err);
    if (err) return 1;
    ts.near_ = near_; ts.far_ = far_; ts.tan_i = tan_i; ts.light = nullptr;
    launch_trace_init(ts, n, nullptr, *p, s);
    RaySet rs{};
    rs.mode = 1; rs.o = ray_o; rs.d = ray_d; rs.t = ts.t;
    rs.nn_hint = c->buf<int>("tr_nn", (size_t)n * 3, &err);      // every iteration starts from the neighbours of the one before
    if (err) return 1;
    for (int it = 0; it < p->iters; ++it) {
        rs.hint_valid = it > 0;
        if (hdq_pass(c, rs, n, p->dist_th, 1, sdf, s, p->soft_shadow ? Q_OTHER : Q_SURFACE)) return 1;
        launch_trace_update(ts, sdf, n, nullptr, it, *p, s);
    }
    if (occ) RA_HIP(hipMemcpyAsync(occ, ts.occ, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    if (st) RA_HIP(hipMemcpyAsync(st, ts.st, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    if (ot) RA_HIP(hipMemcpyAsync(ot, ts.ot, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    if (surf) {
        float* depth = c->buf<float>("tr_depth", n, &err);
        float* acc = c->buf<float>("tr_acc", n, &err);
        int* hidx = c->buf<int>("tr_hidx", n, &err);
        if (err) return 1;
        launch_surface_finish(ray_o, ray_d, ts.st, ts.occ, n, surf, depth, acc, hidx, icnt(c, CNT_HIT), s);
    }
    RA_HIP(hipGetLastError());
    return 0;
}

// what one light-visibility stage reads and returns
struct LvisStage {
    // the hit slots (surf and acc per ray, normals per slot), the box and the trace of their shadow rays
    const float *surf, *norm_slots, *acc, *bbox;
    const int *hit_idx, *hit_count;
    int P, no_visibility, local_visibility;
    float near_offset;
    const ra_trace_params* shadow;
    // optional: the box table of a call that holds several of the reference's chunks, the neighbours the surface trace found per ray,
    // the ray permutation box_start counts in, the human layer's group split (ShadowGen, ra_kernels.hpp)
    int n_boxes;
    const float* boxes;
    const int *box_start, *pix_nn, *perm;
    bool split_wide_groups;
    // out: slot x L, in the context's scratch
    float *lvis, *ldot;
};
// light_visibility (sphere_tracing_renderer.py:265-344) for the hit slots of one chunk: per (slot, light) cosine and
// visibility; rays that face the light and cross the box are sphere traced with the DFSS state machine (HOT LOOP B).
static int light_visibility_stage(ra_ctx* c, LvisStage& st, hipStream_t s) {
    const int P = st.P;
    const ra_trace_params& shadow = *st.shadow;
    int err = 0;
    const int L = c->n_lights;
    const size_t NR = (size_t)P * L;
    st.lvis = c->buf<float>("lv_lvis", NR, &err);
    st.ldot = c->buf<float>("lv_ldot", NR, &err);
    ShadowGen g{};
    g.surf = st.surf; g.norm = st.norm_slots; g.acc = st.acc; g.hit_idx = st.hit_idx; g.hit_count = st.hit_count; g.ldir = c->light_dir.as<float>();
    for (int k = 0; k < 6; ++k) g.bbox[k] = st.bbox[k];
    g.n_boxes = st.n_boxes > 1 ? st.n_boxes : 0;
    for (int j = 0; j < g.n_boxes; ++j) {
        for (int k = 0; k < 6; ++k) g.boxes[j][k] = st.boxes[6 * j + k];
        g.box_start[j] = st.box_start[j];
    }
    if (g.n_boxes) g.box_start[g.n_boxes] = st.box_start[g.n_boxes];
    g.perm = g.n_boxes ? st.perm : nullptr;
    g.near_offset = st.near_offset; g.L = L; g.no_visibility = st.no_visibility; g.local_visibility = st.local_visibility;
    g.split_wide_groups = st.split_wide_groups ? 1 : 0;
    g.lvis = st.lvis; g.ldot = st.ldot;
    g.ray_count = icnt(c, CNT_RAYS);
    const bool traced = !(st.no_visibility || st.local_visibility);
    TraceState sh{};
    float* ssdf = nullptr;
    if (traced) {
        g.ray_pix = c->buf<int>("lv_pix", NR, &err);
        g.ray_light = c->buf<int>("lv_light", NR, &err);
        g.ray_slot = c->buf<int>("lv_slot", NR, &err);
        g.near_ = c->buf<float>("lv_near", NR, &err);
        g.far_ = c->buf<float>("lv_far", NR, &err);
        sh = alloc_trace(c, "sh_", (int)NR, shadow.soft_shadow != 0, &err);      // hard shadows (cfg.no_dfss) run the surface trace's state machine (:182-197)
        ssdf = c->buf<float>("sh_sdf", NR, &err);
    }
    // the key-light tier: the fine points of the rays towards the frame's key lights (at most KEY_LIGHTS_MAX; flags on the device) form a
    // second fine list in every pass of the loop below, answered by the compensated kernel
    const bool keyed = traced && key_tier(c) && c->key_valid;
    const size_t NK = keyed ? (size_t)P * (size_t)(L < KEY_LIGHTS_MAX ? L : KEY_LIGHTS_MAX) : 0;
    if (err) return 1;
    // frames in flight: this stage (the frame's large launches) starts when the stage submitted before it through the same gate has ended
    if (c->gate && c->gate->armed) RA_HIP(hipStreamWaitEvent(s, c->gate->done, 0));
    launch_shadow_gen(g, P, s, c->cnt_zero);     // the chunk's bulk memset covers the first shadow stage; a second one zeroes its counter itself
    c->cnt_zero = false;
    if (traced) {
        sh.near_ = g.near_; sh.far_ = g.far_; sh.tan_i = c->light_sharp.as<float>(); sh.light = g.ray_light;
        launch_trace_init(sh, (int)NR, g.ray_count, shadow, s);
        RaySet r2{};
        r2.mode = 2; r2.o = st.surf; r2.t = sh.t; r2.pix = g.ray_pix; r2.light = g.ray_light; r2.ldir = c->light_dir.as<float>();
        r2.n_dev = g.ray_count;
        r2.skip = c->cfg.query_skip ? sh.stuck : nullptr;
        r2.nn_hint = c->buf<int>("lv_nn", NR * 3, &err);       // every iteration starts from the neighbours of the one before
        if (err) return 1;
        for (int it = 0; it < shadow.iters; ++it) {
            r2.hint_valid = it > 0;
            // first pass: a shadow ray starts next to its pixel's surface point, whose neighbours the surface trace's last query found
            r2.hint_src = it == 0 ? st.pix_nn : nullptr;
            r2.hint_src_index = it == 0 ? g.ray_pix : nullptr;
            if (hdq_pass(c, r2, (int)NR, shadow.dist_th, 1, ssdf, s, Q_OTHER, keyed ? c->key_mask.as<unsigned char>() : nullptr, (int)NK)) return 1;
            launch_trace_update(sh, ssdf, (int)NR, g.ray_count, it, shadow, s);
        }
        launch_shadow_scatter(sh.occ, g.ray_slot, g.ray_count, (int)NR, st.lvis, s);
        launch_accumulate(g.ray_count, &dcnt(c)->n_shadow_rays, s);
    }
    if (c->gate) { RA_HIP(hipEventRecord(c->gate->done, s)); c->gate->armed = true; }
    return 0;
}

int ra_begin_render(ra_ctx* c) {
    RA_CHECK(c, "ra_begin_render: null ctx");
    c->call_no = 0;          // render calls are numbered from here (launch-variant hints: the k-th call of a frame reads the k-th call's counts of an earlier one)
    return 0;
}

int ra_set_key_probes(ra_ctx* c, const float* probes, int n, int ph, int pw, int accumulate, void* stream) {
    RA_CHECK(c && n >= 0 && (n == 0 || (probes && ph > 0 && pw > 0)), "ra_set_key_probes: bad arguments");
    if (n == 0) { c->key_external = false; c->key_valid = false; return 0; }
    RA_CHECK(c->have_weights && c->n_lights > 0, "ra_set_key_probes: needs the relight network's light set (ra_finalize_weights)");
    RA_HIP(hipSetDevice(c->device));
    const bool acc = accumulate && c->key_external && c->key_valid;
    c->key_external = true;
    if (!key_tier(c)) { c->key_valid = false; return 0; }
    if (c->key_mask.ensure((size_t)c->n_lights) || c->key_share.ensure((size_t)c->n_lights * sizeof(float))) return 1;
    launch_key_lights(probes, n, ph, pw, c->light_dir.as<float>(), c->light_area.as<float>(), c->n_lights, c->cfg.key_light_share, KEY_LIGHTS_MAX,
                      acc ? 1 : 0, c->key_share.as<float>(), c->key_mask.as<unsigned char>(), (hipStream_t)stream);
    c->key_valid = true;
    RA_HIP(hipGetLastError());
    return 0;
}

// reorder the hit list hit_idx of a chunk so that neighbouring slots hold neighbouring surface points (launch_sort_hits); every chunk
// shares the hs_* scratch.  bbox: its lower corner is the keys' origin; who: the entry point, for the message
static int sort_hits(ra_ctx* c, const char* who, const float* surf, const float* acc, int P, const float* bbox, int* hit_idx, hipStream_t s) {
    int err = 0;
    const size_t tb = sort_hits_temp_bytes(P);
    unsigned* k0 = c->buf<unsigned>("hs_k0", P, &err);
    unsigned* k1 = c->buf<unsigned>("hs_k1", P, &err);
    int* v0 = c->buf<int>("hs_v0", P, &err);
    char* tmp = c->buf<char>("hs_tmp", tb + 16, &err);
    if (err) return 1;
    if (launch_sort_hits(surf, acc, P, bbox, k0, k1, v0, hit_idx, tmp, tb, s)) { ra_set_error(std::string(who) + ": radix sort failed"); return 1; }
    return 0;
}
// Morton-sort the primary rays of a chunk by their entry point (launch_sort_rays): the four ray arrays become their sorted copies in the
// rs_* scratch, *perm the caller index of every sorted ray.  bbox: its lower corner is the keys' origin; nullptr (the volume path): the chunk's own extent,
// with the entry points clipped to the configured near / far
static int sort_rays(ra_ctx* c, const char* who, const float** ray_o, const float** ray_d, const float** near_, const float** far_, int P,
                     const float* bbox, const int** perm, hipStream_t s) {
    int err = 0;
    const size_t tb = sort_hits_temp_bytes(P);
    unsigned* k0 = c->buf<unsigned>("hs_k0", P, &err);
    unsigned* k1 = c->buf<unsigned>("hs_k1", P, &err);
    int* v0 = c->buf<int>("hs_v0", P, &err);
    int* pm = c->buf<int>("rs_perm", P, &err);
    char* tmp = c->buf<char>("hs_tmp", tb + 16, &err);
    float* so = c->buf<float>("rs_o", (size_t)P * 3, &err);
    float* sd = c->buf<float>("rs_d", (size_t)P * 3, &err);
    float* sn = c->buf<float>("rs_n", P, &err);
    float* sf = c->buf<float>("rs_f", P, &err);
    if (err) return 1;
    const int rc = bbox ? launch_sort_rays(*ray_o, *ray_d, *near_, *far_, P, bbox, k0, k1, v0, pm, tmp, tb, so, sd, sn, sf, s)
                        : launch_sort_rays(*ray_o, *ray_d, *near_, *far_, P, nullptr, k0, k1, v0, pm, tmp, tb, so, sd, sn, sf, s, c->cfg.clip_near, c->cfg.clip_far);
    if (rc) { ra_set_error(std::string(who) + ": radix sort failed"); return 1; }
    *ray_o = so; *ray_d = sd; *near_ = sn; *far_ = sf; *perm = pm;
    return 0;
}

// the box table of a call that holds several of the reference's chunks (ra_sphere_params / ra_ground_params: n_boxes, boxes, box_start)
static int check_box_table(const std::string& w, int n_boxes, const float* boxes, const int* box_start, const float* bbox, int P) {
    if (n_boxes <= 1) return 0;
    RA_CHECK(n_boxes <= RA_MAX_BOXES && boxes && box_start && bbox, w + ": at most 32 boxes per call, with their tables");
    RA_CHECK(box_start[0] == 0 && box_start[n_boxes] == P, w + ": box_start must run from 0 to P");
    for (int j = 0; j < n_boxes; ++j) RA_CHECK(box_start[j] <= box_start[j + 1], w + ": box_start must ascend");
    return 0;
}

int ra_render_sphere_chunk(ra_ctx* c, const float* ray_o, const float* ray_d, const float* near_, const float* far_, int P,
                           const float* bbox, const float* probe, int ph, int pw, const ra_sphere_params* p,
                           const ra_render_out* out, void* stream) {
    if (check_ready(c, "ra_render_sphere_chunk")) return 1;
    RA_CHECK(p && out && P >= 0, "ra_render_sphere_chunk: bad arguments");
    if (P == 0) return 0;
    RA_CHECK(ray_o && ray_d && near_ && far_, "ra_render_sphere_chunk: null ray arrays");
    const bool relit = p->relighting != 0;
    RA_CHECK(!relit || (c->cfg.relight && probe && bbox && c->n_lights > 0), "ra_render_sphere_chunk: relighting needs the relight network, a probe and a bbox");
    RA_CHECK(p->n_samples >= 1 && p->n_samples <= 16, "ra_render_sphere_chunk: n_samples out of range");
    RA_CHECK(!relit || (long long)P * c->n_lights < (1ll << 31), "ra_render_sphere_chunk: chunk too large (rays x lights must fit an int): lower cfg.render_chunk_size / cfg.sphere_chunk_rays");
    if (check_box_table("ra_render_sphere_chunk", p->n_boxes, p->boxes, p->box_start, bbox, P)) return 1;
    hipStream_t s = (hipStream_t)stream;
    int err = 0;
    const int S = p->n_samples, C = raw_channels(c), L = c->n_lights;
    zero_chunk_counters(c, s);                // ONE memset for every device counter this chunk uses
    HintScope hints(c, s);
    // ---- spatially coherent ray order (per-ray results are order-free; outputs go back through perm)
    const int* perm = nullptr;
    if (bbox && sort_rays(c, "ra_render_sphere_chunk", &ray_o, &ray_d, &near_, &far_, P, bbox, &perm, s)) return 1;
    // ---- surface trace (HOT LOOP A)
    TraceState ts = alloc_trace(c, "sf_", P, false, &err);
    float* sdf = c->buf<float>("sf_sdf", P, &err);
    float* surf = c->buf<float>("sf_surf", (size_t)P * 3, &err);
    float* depth = c->buf<float>("sf_depth", P, &err);
    float* acc = c->buf<float>("sf_acc", P, &err);
    int* hit_idx = c->buf<int>("sf_hit", P, &err);
    int* slot_of_ray = c->buf<int>("sf_slot", P, &err);
    if (err) return 1;
    ts.near_ = near_; ts.far_ = far_;
    launch_trace_init(ts, P, nullptr, p->surface, s);
    RaySet rs{};
    rs.mode = 1; rs.o = ray_o; rs.d = ray_d; rs.t = ts.t; rs.skip = c->cfg.query_skip ? ts.stuck : nullptr;
    rs.nn_hint = c->buf<int>("sf_nn", (size_t)P * 3, &err);      // every iteration starts from the neighbours of the one before
    if (err) return 1;
    for (int it = 0; it < p->surface.iters; ++it) {
        rs.hint_valid = it > 0;
        if (hdq_pass(c, rs, P, p->surface.dist_th, 1, sdf, s, Q_SURFACE)) return 1;
        launch_trace_update(ts, sdf, P, nullptr, it, p->surface, s);
    }
    int* hit_count = icnt(c, CNT_HIT);
    launch_surface_finish(ray_o, ray_d, ts.st, ts.occ, P, surf, depth, acc, hit_idx, hit_count, s, slot_of_ray, true);
    launch_accumulate(hit_count, &dcnt(c)->n_hit_pixels, s);
    // spatially coherent hit order for the shadow trace (results are scattered back, so order-free)
    if (relit && sort_hits(c, "ra_render_sphere_chunk", surf, acc, P, bbox, hit_idx, s)) return 1;
    launch_slot_index(hit_idx, hit_count, P, slot_of_ray, s);          // ray -> hit slot in the final hit order (-1: miss)
    // ---- material query on S samples around each hit (render_human :602-620)
    float* xs = c->buf<float>("mt_x", (size_t)P * S * 3, &err);
    float* vs = c->buf<float>("mt_v", (size_t)P * S * 3, &err);
    float* raw = c->buf<float>("mt_raw", (size_t)P * S * C, &err);
    SurfaceMaps m{};
    m.cpts = c->buf<float>("mp_cpts", (size_t)P * 3, &err);
    m.bpts = c->buf<float>("mp_bpts", (size_t)P * 3, &err);
    m.resd = c->buf<float>("mp_resd", (size_t)P * 3, &err);
    m.norm = c->buf<float>("mp_norm", (size_t)P * 3, &err);
    m.albedo = c->buf<float>("mp_albedo", (size_t)P * 3, &err);
    m.rough = c->buf<float>("mp_rough", P, &err);
    m.rgb = c->buf<float>("mp_rgb", (size_t)P * 3, &err);
    m.valbedo = (out->volume_albedo && c->cfg.relight) ? c->buf<float>("mp_valbedo", (size_t)P * 3, &err) : nullptr;
    if (err) return 1;
    launch_surface_samples(surf, ray_d, hit_idx, hit_count, P, S, p->surf_sample_range, xs, vs, icnt(c, CNT_SAMP), s);
    if (forward_pass(c, xs, vs, P * S, icnt(c, CNT_SAMP), p->dist_th, raw, s)) return 1;
    launch_surface_composite(raw, C, S, hit_count, P, c->cfg.relight, c->cfg, m, s);
    // ---- light visibility + shading (HOT LOOP B)
    float *shade = nullptr, *spec = nullptr;
    LvisStage st{};
    if (relit) {
        if (key_mask_from(c, probe, ph, pw, s)) return 1;
        st.surf = surf; st.norm_slots = m.norm; st.acc = acc; st.hit_idx = hit_idx; st.hit_count = hit_count; st.P = P; st.bbox = bbox;
        st.near_offset = p->shadow_near_offset; st.shadow = &p->shadow; st.no_visibility = p->no_visibility; st.local_visibility = p->local_visibility;
        st.n_boxes = p->n_boxes; st.boxes = p->boxes; st.box_start = p->box_start; st.pix_nn = rs.nn_hint; st.perm = perm; st.split_wide_groups = true;
        if (light_visibility_stage(c, st, s)) return 1;
        m.rgb = c->buf<float>("mp_rgb", (size_t)P * 3, &err);
        shade = c->buf<float>("mp_shade", (size_t)P * 3, &err);
        spec = c->buf<float>("mp_spec", (size_t)P * 3, &err);
        if (err) return 1;
        ShadeIn in{};
        in.ray_o = ray_o; in.surf = surf; in.idx = hit_idx; in.count = hit_count; in.n = P;
        in.norm = m.norm; in.albedo = m.albedo; in.rough = m.rough; in.lvis = st.lvis; in.ldot = st.ldot;
        in.light_xyz = c->light_xyz.as<float>(); in.light_area = c->light_area.as<float>(); in.L = L;
        in.probes = probe; in.n_probes = 1; in.ph = ph; in.pw = pw; in.want_spec = out->spec != nullptr;
        in.rgb = m.rgb; in.shade = shade; in.spec = spec;
        launch_shade(in, c->cfg, s);      // n_shaded: counted on the device via the hit pixels (ra_get_counters)
    }
    // ---- every requested map to the full ray set (zeros elsewhere), premultiplied by acc (alpha_output_): one launch
    const int pm = p->premultiply;
    EmitMaps em{};
    em.slot_of_ray = slot_of_ray; em.acc = acc; em.perm = perm; em.P = P;
    long long total = 0;
    auto scat = [&](float* dst, const float* src, int Cc, bool premul, bool src_full) {
        if (!dst) return;
        if (em.n_jobs == RA_MAX_MAP_JOBS) { launch_emit_maps(em, s); em.n_jobs = 0; total = 0; }
        total += (long long)P * Cc;
        em.job[em.n_jobs] = MapJob{src, dst, Cc, premul ? 1 : 0, src_full ? 1 : 0};
        em.end[em.n_jobs++] = total;
    };
    scat(out->acc, acc, 1, false, true);
    scat(out->depth, depth, 1, pm, true);
    scat(out->surf, surf, 3, pm, true);
    scat(out->ray_o, ray_o, 3, false, true);
    scat(out->norm, m.norm, 3, pm, false);
    scat(out->cpts, m.cpts, 3, pm, false);
    scat(out->bpts, m.bpts, 3, pm, false);
    scat(out->resd, m.resd, 3, false, false);
    scat(out->rgb, m.rgb, 3, pm, false);
    if (c->cfg.relight) {
        scat(out->albedo, m.albedo, 3, pm, false);
        scat(out->roughness, m.rough, 1, pm, false);
        scat(out->volume_albedo, m.valbedo, 3, false, false);
        scat(out->volume_roughness, m.rough, 1, false, false);
    }
    scat(out->raw, raw, S * C, false, false);
    if (relit) {
        scat(out->shade, shade, 3, pm, false);
        scat(out->spec, spec, 3, pm, false);
        scat(out->lvis, st.lvis, L, pm, false);
        scat(out->ldot, st.ldot, L, pm, false);
    }
    launch_emit_maps(em, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_render_ground_chunk(ra_ctx* c, const float* ray_o, const float* ray_d, const float* acc, int P, const float* bbox,
                           const float* probe, int ph, int pw, const ra_ground_params* p, const ra_ground_out* out, void* stream) {
    if (check_ready(c, "ra_render_ground_chunk")) return 1;
    RA_CHECK(p && out && P >= 0, "ra_render_ground_chunk: bad arguments");
    if (P == 0) return 0;
    RA_CHECK(ray_o && ray_d && acc && bbox && probe, "ra_render_ground_chunk: null argument");
    RA_CHECK(c->cfg.relight && c->n_lights > 0, "ra_render_ground_chunk: needs the relight network's light set");
    RA_CHECK((long long)P * c->n_lights < (1ll << 31), "ra_render_ground_chunk: chunk too large (P x lights must fit an int)");
    if (check_box_table("ra_render_ground_chunk", p->n_boxes, p->boxes, p->box_start, bbox, P)) return 1;      // bbox: checked above
    hipStream_t s = (hipStream_t)stream;
    int err = 0;
    zero_chunk_counters(c, s);
    HintScope hints(c, s);
    c->cnt_zero = false;                      // launch_ground_hit zeroes its hit counter itself
    GroundIn g{};
    g.ray_o = ray_o; g.ray_d = ray_d; g.acc = acc; g.P = P;
    const float nn = std::sqrt(p->normal[0] * p->normal[0] + p->normal[1] * p->normal[1] + p->normal[2] * p->normal[2]) + 1e-8f;   // normalize(): x / (|x| + eps)
    for (int k = 0; k < 3; ++k) { g.n[k] = p->normal[k] / nn; g.orig[k] = p->origin[k]; g.albedo[k] = p->albedo[k]; }
    g.attach_envmap = p->attach_envmap; g.env_r = p->env_r; g.shading_multiplier = p->shading_multiplier;
    float* t = c->buf<float>("gd_t", P, &err);
    float* surf = c->buf<float>("gd_surf", (size_t)P * 3, &err);
    float* depth = c->buf<float>("gd_depth", P, &err);
    float* nslots = c->buf<float>("gd_norm", (size_t)P * 3, &err);
    int* hit_idx = c->buf<int>("gd_hit", P, &err);
    if (err) return 1;
    int* hit_count = icnt(c, CNT_HIT);
    launch_ground_hit(g, t, surf, depth, nslots, hit_idx, hit_count, s);
    // spatially coherent order of the traced pixels (results are written back per pixel, so order-free)
    if (sort_hits(c, "ra_render_ground_chunk", surf, acc, P, bbox, hit_idx, s)) return 1;
    if (key_mask_from(c, probe, ph, pw, s)) return 1;
    LvisStage st{};
    st.surf = surf; st.norm_slots = nslots; st.acc = acc; st.hit_idx = hit_idx; st.hit_count = hit_count; st.P = P; st.bbox = bbox;
    st.near_offset = p->shadow_near_offset; st.shadow = &p->shadow; st.no_visibility = p->no_visibility; st.local_visibility = p->local_visibility;
    st.n_boxes = p->n_boxes; st.boxes = p->boxes; st.box_start = p->box_start;
    if (light_visibility_stage(c, st, s)) return 1;
    auto zero = [&](void* dst, int C) { if (dst) hipMemsetAsync(dst, 0, (size_t)P * C * sizeof(float), s); };
    zero(out->rgb, 3); zero(out->albedo, 3); zero(out->shade, 3); zero(out->spec, 3);
    zero(out->lvis, c->n_lights); zero(out->ldot, c->n_lights);
    GroundShade in{};
    in.g = g; in.t = t; in.surf = surf; in.hit_idx = hit_idx; in.hit_count = hit_count; in.lvis = st.lvis;
    in.ldir = c->light_dir.as<float>(); in.light_area = c->light_area.as<float>(); in.L = c->n_lights;
    in.probe = probe; in.ph = ph; in.pw = pw;
    in.rgb = (float*)out->rgb; in.albedo = (float*)out->albedo; in.shade = (float*)out->shade; in.spec = (float*)out->spec;
    in.lvis_out = (float*)out->lvis; in.ldot_out = (float*)out->ldot;
    launch_ground_shade(in, c->cfg, s);
    if (out->surf) RA_HIP(hipMemcpyAsync(out->surf, surf, (size_t)P * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (out->depth) RA_HIP(hipMemcpyAsync(out->depth, depth, (size_t)P * sizeof(float), hipMemcpyDeviceToDevice, s));
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_render_volume_chunk(ra_ctx* c, const float* ray_o, const float* ray_d, const float* near_, const float* far_, int P,
                           int n_samples, float dist_th, const ra_render_out* out, void* stream) {
    if (check_ready(c, "ra_render_volume_chunk")) return 1;
    RA_CHECK(out && P >= 0 && n_samples >= 1, "ra_render_volume_chunk: bad arguments");
    if (P == 0) return 0;
    RA_CHECK(ray_o && ray_d && near_ && far_, "ra_render_volume_chunk: null ray arrays");
    RA_CHECK(!c->cfg.relight, "ra_render_volume_chunk: volume rendering is wired for the AniSDF network (base_renderer)");
    hipStream_t s = (hipStream_t)stream;
    int err = 0;
    zero_chunk_counters(c, s);
    HintScope hints(c, s);
    const int S = n_samples, C = 16;
    const size_t N = (size_t)((P + 63) & ~63) * S;          // samples are laid out per group of 64 rays (padded)
    RA_CHECK(N < (1u << 30), "ra_render_volume_chunk: chunk too large");
    float* xs = c->buf<float>("vl_x", N * 3, &err);
    float* vs = c->buf<float>("vl_v", N * 3, &err);
    float* raw = c->buf<float>("vl_raw", N * C, &err);
    if (err) return 1;
    // spatially coherent ray order (Morton code of the entry point); outputs go back through the permutation
    const int* perm = nullptr;
    if (sort_rays(c, "ra_render_volume_chunk", &ray_o, &ray_d, &near_, &far_, P, nullptr, &perm, s)) return 1;
    launch_volume_samples(ray_o, ray_d, near_, far_, P, S, xs, vs, s);
    if (forward_pass(c, xs, vs, (int)N, nullptr, dist_th, raw, s)) return 1;
    launch_volume_composite(raw, C, near_, far_, P, S, c->cfg.bg_brightness, *out, perm, s);
    RA_HIP(hipGetLastError());
    return 0;
}

// light_visibility on caller-given surface points (also behind ra_debug_lvis): the render chunk's stage with the caller's list as
// its hit slots.  rows == nullptr: every point is its own hit slot.  No HintScope and no zero_chunk_counters: the render calls' hints and
// their numbering stay as they are, and the stage zeroes its ray counter itself.
int ra_light_visibility(ra_ctx* c, const float* surf, const float* norm, const float* acc, int n, const int* rows, int n_rows, const float* bbox,
                        const float* probe, int ph, int pw, const ra_sphere_params* p, float* lvis_out, float* ldot_out, void* stream) {
    if (check_ready(c, "ra_light_visibility")) return 1;
    RA_CHECK(c->cfg.relight && c->n_lights > 0, "ra_light_visibility: needs the relight network's light set");
    RA_CHECK(n >= 0 && p && (!rows || n_rows >= 0) && (!probe || (ph > 0 && pw > 0)), "ra_light_visibility: bad arguments");
    const int P = rows ? n_rows : n;
    if (n == 0 || P == 0) return 0;
    RA_CHECK(surf && norm && acc && bbox && lvis_out && ldot_out, "ra_light_visibility: null input");
    RA_CHECK(P <= n, "ra_light_visibility: more rows than points (rows are distinct indices into the n points)");
    RA_CHECK((long long)P * c->n_lights < (1ll << 31), "ra_light_visibility: too many rays (points x lights must fit an int): trace the frame in row subsets");
    hipStream_t s = (hipStream_t)stream;
    if (key_mask_from(c, probe, ph, pw, s)) return 1;       // the key lights of the probe the caller shades with, as in a render call
    int err = 0;
    int* hit_count = icnt(c, CNT_HIT);
    const int* hit_idx = rows;
    const float* norm_slots = norm;
    if (rows) {      // the stage reads normals per hit slot, surf and acc per point
        float* ns = c->buf<float>("dl_norm", (size_t)P * 3, &err);
        if (err) return 1;
        RA_HIP(hipMemsetD32Async((hipDeviceptr_t)hit_count, P, 1, s));
        launch_gather_rows(rows, hit_count, P, norm, 3, ns, s);
        norm_slots = ns;
    } else {
        int* iota = c->buf<int>("dl_hit", P, &err);
        if (err) return 1;
        launch_iota(iota, P, hit_count, s);
        hit_idx = iota;
    }
    LvisStage st{};
    st.surf = surf; st.norm_slots = norm_slots; st.acc = acc; st.hit_idx = hit_idx; st.hit_count = hit_count; st.P = P; st.bbox = bbox;
    st.near_offset = p->shadow_near_offset; st.shadow = &p->shadow; st.no_visibility = p->no_visibility; st.local_visibility = p->local_visibility;
    if (light_visibility_stage(c, st, s)) return 1;
    RA_HIP(hipMemcpyAsync(lvis_out, st.lvis, (size_t)P * c->n_lights * 4, hipMemcpyDeviceToDevice, s));
    RA_HIP(hipMemcpyAsync(ldot_out, st.ldot, (size_t)P * c->n_lights * 4, hipMemcpyDeviceToDevice, s));
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_set_light_xyz(ra_ctx* c, const float* xyz, void* stream) {
    RA_CHECK(c && c->have_weights && c->cfg.relight, "ra_set_light_xyz: needs a relight ctx with weights");
    RA_CHECK(c->n_lights > 0 && c->light_xyz.p && c->light_xyz_loaded.p, "ra_set_light_xyz: the ctx has no light set");
    RA_HIP(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipMemcpyAsync(c->light_xyz.p, xyz ? (const void*)xyz : c->light_xyz_loaded.p, (size_t)c->n_lights * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    launch_light_dirs(c->light_xyz.as<float>(), c->n_lights, c->light_dir.as<float>(), s);
    c->key_external = false;      // flags named through ra_set_key_probes belong to the old directions
    c->key_valid = false;
    RA_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

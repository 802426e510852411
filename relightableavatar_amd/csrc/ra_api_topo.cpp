// C ABI: the ra_topo handle and what runs on it — connectivity, Taubin smoothing, Loop subdivision, dilation (ra_topo.hip), fitting (ra_fit.hip)
#include "ra_api_impl.hpp"
#include "ra_topo_rules.hpp"
#include "ra_fit_rules.hpp"

extern "C" {

int ra_topo_tile(int which) { return which == 0 ? TOPO_BLOCK : which == 1 ? TOPO_SMOOTH_BLOCK : which == 2 ? TOPO_MAX_CHANNELS : 0; }

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
    RA_CHECK(owned(c->topos, topo), "ra_topo_destroy: not a topology of this ctx");
    for (auto& g : c->cloths) RA_CHECK(g->topo != topo, "ra_topo_destroy: a cloth of this ctx still reads this topology (ra_cloth_destroy first)");
    release_owned(c, c->topos, topo);      // smoothing passes that read it may still be queued
    return 0;
}

int ra_topo_sizes(ra_ctx* c, const ra_topo* topo, int* sizes) {
    RA_CHECK(c && topo && sizes, "ra_topo_sizes: null argument");
    RA_CHECK(owned(c->topos, topo), "ra_topo_sizes: not a topology of this ctx");
    sizes[0] = topo->view.n_faces; sizes[1] = topo->view.n_verts; sizes[2] = topo->view.n_edges;
    sizes[3] = topo->max_nbr; sizes[4] = topo->max_out; sizes[5] = topo->readbacks; sizes[6] = topo->max_count;
    return 0;
}

int ra_topo_array(ra_ctx* c, const ra_topo* topo, int which, int* out, void* stream) {
    RA_CHECK(c && topo, "ra_topo_array: null argument");
    RA_CHECK(owned(c->topos, topo), "ra_topo_array: not a topology of this ctx");
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
    RA_CHECK(owned(c->topos, topo), "ra_mesh_smooth: not a topology of this ctx");
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
    ra_topo* parent = owned(c->topos, topo);
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
    RA_CHECK(owned(c->topos, topo), "ra_topo_dilate: not a topology of this ctx");
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

// ---- mesh fitting: the large-steps operator and solve, normals, AdamUniform (ra_fit.hip; the ICP residual: ra_api_mesh.cpp) -------
int ra_fit_tile(int which) { return which == 0 ? FIT_BLOCK : which == 1 ? FIT_BLOCK : 0; }

int ra_topo_diffuse_apply(ra_ctx* c, const ra_topo* topo, const float* x, int n_verts, int C, float lambda, float* out, void* stream) {
    RA_CHECK(c && topo, "ra_topo_diffuse_apply: null argument");
    RA_CHECK(owned(c->topos, topo), "ra_topo_diffuse_apply: not a topology of this ctx");
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
    RA_CHECK(owned(c->topos, topo), "ra_topo_diffuse_solve: not a topology of this ctx");
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
    RA_CHECK(owned(c->topos, topo), "ra_mesh_normals: not a topology of this ctx");
    RA_CHECK(n_verts == topo->view.n_verts, "ra_mesh_normals: bad sizes (n_verts of the topology)");
    RA_CHECK(face_normal || face_area || vert_normal, "ra_mesh_normals: null argument (all three outputs)");
    if (n_verts == 0) return 0;
    RA_CHECK(verts, "ra_mesh_normals: null argument (verts)");
    RA_HIP(hipSetDevice(c->device));
    launch_mesh_normals(topo->view, verts, face_normal, face_area, vert_normal, (hipStream_t)stream);
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

}  // extern "C"

// C ABI: the ra_cloth handle and the cloth energies — StVK stretch, dihedral bending, gravity, inertia (ra_cloth.hip)
#include "ra_api_impl.hpp"
#include "ra_cloth_rules.hpp"
#include <algorithm>

extern "C" {

int ra_cloth_tile(int which) { return which >= 0 && which <= 2 ? CLOTH_BLOCK : which == 3 ? CLOTH_CHUNK : 0; }

static bool cloth_finite(double x) { return x - x == 0.0; }

int ra_cloth_material_derive(const ra_cloth_material* m, double* out) {
    RA_CHECK(m && out, "ra_cloth_material_derive: null argument");
    cloth_material(m->thickness, m->young_modulus, m->poisson_ratio, m->bending_multiplier, m->stretch_multiplier, m->material_multiplier, out);
    return 0;
}

int ra_cloth_create(ra_ctx* c, const ra_topo* topo, const float* rest, int n_verts, const float* vm, int n_vm, const int* fm, const ra_cloth_material* m,
                    ra_cloth** out, void* stream) {
    RA_CHECK(c && topo && m && out, "ra_cloth_create: null argument");
    RA_CHECK(owned(c->topos, topo), "ra_cloth_create: not a topology of this ctx");
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
    RA_CHECK(owned(c->cloths, cloth), "ra_cloth_destroy: not a cloth of this ctx");
    release_owned(c, c->cloths, cloth);
    return 0;
}

int ra_cloth_array(ra_ctx* c, const ra_cloth* cloth, int which, void* out, void* stream) {
    RA_CHECK(c && cloth, "ra_cloth_array: null argument");
    RA_CHECK(owned(c->cloths, cloth), "ra_cloth_array: not a cloth of this ctx");
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
    RA_CHECK(owned(c->cloths, cloth), "ra_cloth_energy: not a cloth of this ctx");
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

}  // extern "C"

// C ABI: the ra_mesh handle and its queries — exact point-to-mesh distance and its backward, winding numbers, ray casting, the ICP residual
#include "ra_api_impl.hpp"
#include "ra_mesh_grad.hpp"

extern "C" {

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

// the Morton order of a query's points: neighbours in space share a wave, so a wave opens little more than one lane would; the answers
// do not depend on it.  1: out of device memory, 2: the sort failed
static int mesh_point_order(ra_ctx* c, const float* pts, int n, const int** perm, hipStream_t s) {
    MeshBuild b{};
    if (mesh_sort_scratch(c, n, &b)) return 1;
    if (launch_mesh_sort_points(pts, n, b, s)) return 2;
    *perm = b.vals_sorted;
    return 0;
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
    RA_CHECK(owned(c->meshes, mesh), "ra_mesh_destroy: not a mesh of this ctx");
    release_owned(c, c->meshes, mesh);      // queries and the upload of its faces may still be queued
    return 0;
}

int ra_mesh_closest(ra_ctx* c, const ra_mesh* mesh, const float* pts, int n, int flags, float* d2, float* closest, int* face, float* bary,
                    void* stream) {
    RA_CHECK(c && mesh, "ra_mesh_closest: null argument");
    RA_CHECK(owned(c->meshes, mesh), "ra_mesh_closest: not a mesh of this ctx");
    RA_CHECK(n >= 0 && n < (1 << 30), "ra_mesh_closest: bad sizes");
    RA_CHECK((flags & ~(RA_MESH_BRUTE | RA_MESH_UNSORTED)) == 0, "ra_mesh_closest: unknown flag");
    if (n == 0) return 0;       // nothing to read or write: empty arrays have no address
    RA_CHECK(pts && (d2 || closest || face || bary), "ra_mesh_closest: null argument (pts, or all four outputs)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    MeshQuery q{};
    q.pts = pts; q.n = n; q.brute = (flags & RA_MESH_BRUTE) != 0; q.d2 = d2; q.closest = closest; q.face = face; q.bary = bary;
    if (!q.brute && !(flags & RA_MESH_UNSORTED) && n > MESH_SORT_MIN) {       // the exhaustive scan opens everything anyway
        const int rc = mesh_point_order(c, pts, n, &q.perm, s);
        RA_CHECK(rc != 1, "ra_mesh_closest: out of device memory");
        RA_CHECK(rc == 0, "ra_mesh_closest: device sort failed");
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

// few points: the faces are split across workgroups to fill the chip, and a second pass adds the chunk sums in chunk order (the same bits).
// per: the float64 sums per (point, chunk), all within one budget of bytes; name: their scratch.  *partial stays null for one pass
static int winding_split(ra_ctx* c, const ra_mesh* mesh, int n, int flags, int per, const char* name, double** partial) {
    const long long n_chunks = wind_chunk_count(mesh->view.n_leaves), tiles = ((long long)n + WIND_BLOCK - 1) / WIND_BLOCK;
    const bool split = (flags & RA_WINDING_SPLIT) || (!(flags & RA_WINDING_ONE_PASS) && n_chunks > 1 && tiles < WIND_SPLIT_TILES && n * n_chunks * per <= WIND_SPLIT_MAX);
    int err = 0;
    if (split) *partial = c->buf<double>(name, (size_t)(n * n_chunks * per), &err);
    return err;
}

int ra_mesh_winding(ra_ctx* c, const ra_mesh* mesh, const float* pts, int n, int flags, float* winding, void* stream) {
    RA_CHECK(c && mesh, "ra_mesh_winding: null argument");
    RA_CHECK(owned(c->meshes, mesh), "ra_mesh_winding: not a mesh of this ctx");
    RA_CHECK(n >= 0 && n < (1 << 30), "ra_mesh_winding: bad sizes");
    RA_CHECK((flags & ~(RA_WINDING_ONE_PASS | RA_WINDING_SPLIT)) == 0 && flags != (RA_WINDING_ONE_PASS | RA_WINDING_SPLIT), "ra_mesh_winding: unknown flag");
    if (n == 0) return 0;       // nothing to read or write: empty arrays have no address
    RA_CHECK(pts && winding, "ra_mesh_winding: null argument (pts, winding)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    double* partial = nullptr;
    RA_CHECK(!winding_split(c, mesh, n, flags, 1, "winding_partial", &partial), "ra_mesh_winding: out of device memory");
    launch_mesh_winding(mesh->view, pts, n, partial, winding, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_mesh_winding_grad(ra_ctx* c, const ra_mesh* mesh, const float* pts, int n, int flags, float* winding, float* grad, void* stream) {
    RA_CHECK(c && mesh, "ra_mesh_winding_grad: null argument");
    RA_CHECK(owned(c->meshes, mesh), "ra_mesh_winding_grad: not a mesh of this ctx");
    RA_CHECK(n >= 0 && n < (1 << 30), "ra_mesh_winding_grad: bad sizes");
    RA_CHECK((flags & ~(RA_WINDING_ONE_PASS | RA_WINDING_SPLIT)) == 0 && flags != (RA_WINDING_ONE_PASS | RA_WINDING_SPLIT), "ra_mesh_winding_grad: unknown flag");
    if (n == 0) return 0;       // nothing to read or write: empty arrays have no address
    RA_CHECK(pts && grad, "ra_mesh_winding_grad: null argument (pts, grad)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    double* partial = nullptr;
    RA_CHECK(!winding_split(c, mesh, n, flags, 4, "winding_grad_partial", &partial), "ra_mesh_winding_grad: out of device memory");
    launch_mesh_winding_grad(mesh->view, pts, n, partial, winding, grad, s);
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- ray-mesh intersection (ra_raycast.hip) -------------------------------------------------------
int ra_raycast_tile(int which) { return which == 0 ? RAY_BLOCK : which == 1 ? RAY_PAIR_BLOCK : which == 2 ? MESH_SORT_MIN : 0; }

int ra_mesh_raycast(ra_ctx* c, const ra_mesh* mesh, const float* ray_o, const float* ray_d, int n, int flags, float* t, int* face, float* uv,
                    int* count, void* stream) {
    RA_CHECK(c && mesh, "ra_mesh_raycast: null argument");
    RA_CHECK(owned(c->meshes, mesh), "ra_mesh_raycast: not a mesh of this ctx");
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
        const int rc = mesh_point_order(c, ray_o, n, &q.perm, s);
        RA_CHECK(rc != 1, "ra_mesh_raycast: out of device memory");
        RA_CHECK(rc == 0, "ra_mesh_raycast: device sort failed");
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

// ---- the ICP residual of mesh fitting (ra_fit.hip) ------------------------------------------------
int ra_icp_residual(ra_ctx* c, const ra_mesh* mesh, const float* pts, const float* pt_normals, int n, const float* face_normals, float dist_th,
                    float angle_th, double* sums, float* grad, unsigned char* keep, void* stream) {
    RA_CHECK(c && mesh && sums, "ra_icp_residual: null argument");
    RA_CHECK(owned(c->meshes, mesh), "ra_icp_residual: not a mesh of this ctx");
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

}  // extern "C"

// C ABI: mesh extraction — the SDF volume, marching cubes with its attributes and backward, the largest component (ra_mcubes.hip, ra_mcubes_grad.hip)
#include "ra_api_impl.hpp"
#include "ra_mcubes.hpp"
#include "ra_mcubes_grad_rules.hpp"
#include <cstring>

extern "C" {

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

}  // extern "C"

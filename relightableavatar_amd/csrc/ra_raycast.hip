// Ray-mesh intersection (ra_mesh_raycast) and the dense ray x triangle pairs (ra_ray_tri_pairs): the reference's moller_trumbore and
// ray_stabbing (lib/utils/mesh_utils.py:686-738) on the box structure of ra_mesh.hip.
//
// One lane per ray, one wave per workgroup (the waves share nothing).  The sweep is the one of mesh_closest_kernel: groups, leaves
// and face records are walked in stored order with wave-uniform control flow; a box is opened when ANY lane's ray can meet it
// (ballot), and every box and 48-byte face record is fetched with a wave-uniform address (scalar loads, no LDS).  The per-pair
// arithmetic, the hit predicate with its grazing guard and slab clause, and the lemma that makes the sweep exact are in
// ra_raycast_tri.hpp: an accepted pair passes the computed slab test of its leaf and group box with an entry bound <= its t, so
//   - count mode (count != nullptr) skips a box only when no lane's slab test passes: no accepted face is lost, and nothing is
//     pruned by t;
//   - nearest mode also skips a box whose entry bound is STRICTLY above the lane's best t: no face that enters the (t, id) minimum is
//     lost, ties included.
// A lane keeps the lexicographic minimum of (t, original face id) and the number of accepted faces: neither depends on the order the
// faces are seen in, so the result is a function of (ray, mesh) alone and the sweep returns the bits of RA_RAYCAST_BRUTE.
// Clauses (2) and (3) of the predicate run only where some lane passed the reference's test (a wave-uniform branch): hits are rare
// among the pairs a wave computes, so a pair costs little more than raycast_tri — nine differences, two cross products, four dot
// products, one division.
#include "ra_kernels.hpp"
#include "ra_raycast_tri.hpp"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ bool ray_finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__global__ __launch_bounds__(RAY_BLOCK) void mesh_raycast_kernel(MeshView m, RayQuery q) {
    const int i = blockIdx.x * RAY_BLOCK + threadIdx.x;
    const bool in = i < q.n;
    const int ri = in ? (q.perm ? q.perm[i] : i) : 0;
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    if (in) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { o[k] = q.o[3 * (size_t)ri + k]; d[k] = q.d[3 * (size_t)ri + k]; }
    }
    // a non-finite ray computes along as o = d = 0 and never votes: it cannot widen what its wave opens.  Nor does a ray with d = 0,
    // which the guard refuses on every face
    const bool alive = in && ray_finite3(o[0], o[1], o[2]) && ray_finite3(d[0], d[1], d[2]);
    if (!alive) { o[0] = o[1] = o[2] = 0.f; d[0] = d[1] = d[2] = 0.f; }
    const bool votes = alive && (d[0] != 0.f || d[1] != 0.f || d[2] != 0.f);
    const RayPre pre = ray_prepare(d);
    const bool brute = q.brute != 0, prune_t = q.count == nullptr;
    const float nanv = __uint_as_float(0x7fc00000u);
    float best_t = RAY_INF, best_u = nanv, best_v = nanv;
    int bid = 0x7fffffff, cnt = 0;
    for (int g = 0; g < m.n_groups; ++g) {
        if (!brute) {
            float lo_t, hi_t;
            ray_slab(o, pre, m.gbox + 6 * (size_t)g, lo_t, hi_t);
            const bool open = votes && ray_slab_pass(lo_t, hi_t) && !(prune_t && lo_t > best_t);
            if (__ballot(open) == 0ull) continue;
        }
        const int l1 = min(m.n_leaves, (g + 1) * MESH_FAN);
        for (int l = g * MESH_FAN; l < l1; ++l) {
            if (!brute) {
                float lo_t, hi_t;
                ray_slab(o, pre, m.lbox + 6 * (size_t)l, lo_t, hi_t);
                const bool open = votes && ray_slab_pass(lo_t, hi_t) && !(prune_t && lo_t > best_t);
                if (__ballot(open) == 0ull) continue;
            }
            const float* rec = m.recs + (size_t)l * (MESH_LEAF * MESH_REC);
            for (int k = 0; k < MESH_LEAF; ++k, rec += MESH_REC) {
                const int id = __float_as_int(rec[9]);
                if (id < 0) break;              // kept faces come first in sorted order: nothing behind the first empty slot
                const float a[3] = {rec[0], rec[1], rec[2]}, b[3] = {rec[3], rec[4], rec[5]}, c[3] = {rec[6], rec[7], rec[8]};
                const RayTri r = raycast_tri(o, d, a, b, c);
                bool hit = votes && raycast_ref_hit(r);
                if (__ballot(hit) == 0ull) continue;
                hit = hit && raycast_confirm(o, d, pre, a, b, c, r);
                if (hit) {
                    ++cnt;
                    if (r.t < best_t || (r.t == best_t && id < bid)) { best_t = r.t; best_u = r.u; best_v = r.v; bid = id; }
                }
            }
        }
    }
    if (!in) return;
    const bool found = bid != 0x7fffffff;
    if (q.t) q.t[ri] = alive ? best_t : nanv;
    if (q.face) q.face[ri] = found ? bid : -1;
    if (q.uv) { q.uv[2 * (size_t)ri] = best_u; q.uv[2 * (size_t)ri + 1] = best_v; }
    if (q.count) q.count[ri] = alive ? cnt : -1;
}

// u, v, t of every (ray, triangle) pair, no guard: out[i * f + j]
__global__ __launch_bounds__(RAY_PAIR_BLOCK) void ray_tri_pairs_kernel(const float* __restrict__ ro, const float* __restrict__ rd, int n,
                                                                       const float* __restrict__ tris, int f, float* __restrict__ u,
                                                                       float* __restrict__ v, float* __restrict__ t) {
    const long long p = (long long)blockIdx.x * RAY_PAIR_BLOCK + threadIdx.x;
    if (p >= (long long)n * f) return;
    const int i = (int)(p / f), j = (int)(p - (long long)i * f);
    const float* tr = tris + 9 * (size_t)j;
    const float o[3] = {ro[3 * (size_t)i], ro[3 * (size_t)i + 1], ro[3 * (size_t)i + 2]};
    const float d[3] = {rd[3 * (size_t)i], rd[3 * (size_t)i + 1], rd[3 * (size_t)i + 2]};
    const float a[3] = {tr[0], tr[1], tr[2]}, b[3] = {tr[3], tr[4], tr[5]}, c[3] = {tr[6], tr[7], tr[8]};
    const RayTri r = raycast_tri(o, d, a, b, c);
    if (u) u[p] = r.u;
    if (v) v[p] = r.v;
    if (t) t[p] = r.t;
}

}  // namespace

void launch_mesh_raycast(const MeshView& m, const RayQuery& q, hipStream_t s) {
    hipLaunchKernelGGL(mesh_raycast_kernel, dim3((q.n + RAY_BLOCK - 1) / RAY_BLOCK), dim3(RAY_BLOCK), 0, s, m, q);
}

void launch_ray_tri_pairs(const float* o, const float* d, int n, const float* tris, int f, float* u, float* v, float* t, hipStream_t s) {
    const long long pairs = (long long)n * f;
    hipLaunchKernelGGL(ray_tri_pairs_kernel, dim3((unsigned)((pairs + RAY_PAIR_BLOCK - 1) / RAY_PAIR_BLOCK)), dim3(RAY_PAIR_BLOCK), 0, s, o, d, n,
                       tris, f, u, v, t);
}

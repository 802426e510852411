// Exact closest point on a triangle mesh (ra_mesh_create / ra_mesh_closest): the primitive of the reference's mesh evaluator
// (lib/evaluators/mesh_evaluator.py: trimesh.proximity.closest_point) and of its bvh_distance_queries / point_mesh_distance callers.
//
// The structure is the one of the exact 3-NN (ra_hdq.hip) over triangles instead of vertices: faces in Morton order of their centroids,
// leaves of MESH_LEAF faces, groups of MESH_FAN leaves, both with boxes; flat and wide on purpose, so that a wave sweeps it with
// wave-uniform control flow and every box and face record is fetched with a wave-uniform address (scalar loads: a face is ONE
// 48-byte record a.xyz b.xyz c.xyz id — not the x[32] | y[32] | ... planes of the vertex leaves, which are laid out for per-lane packed
// loads).  One lane per query point.
//
// Exactness.  mesh_closest_tri (ra_mesh_tri.hpp) is written once, with every product and sum a named fp32 operation and contraction off,
// so a (point, face) pair has ONE d2 whatever kernel or loop computes it.  A lane keeps the lexicographic minimum of (d2, original
// face id) over the faces it sees, which does not depend on the order it sees them in.  A box is skipped only when its lower bound
// is STRICTLY greater than the bound of every lane of the wave, the bounds being
//   - lower: the squared distance from p to the box, in the same operations as d2.  The boxes are widened by 2^-19 of their largest
//     coordinate at build time, more than the rounding of a computed closest point (a + v ab + w ac, v, w, v + w in [0, 1 + 2^-22]:
//     below 2^-20 of the largest coordinate), so the COMPUTED closest point of every face lies in its box, and since fp32 rounding is
//     monotone the computed d2 of the face is not below the computed bound of the box;
//   - upper: a lane's own best d2 so far, and the smallest far-corner distance of a group box (every group box holds a face whose
//     computed closest point is inside it, so some face has a computed d2 not above that).
// So no face that attains the minimum is ever skipped, ties included, and the sweep returns the bits of RA_MESH_BRUTE.
#include "ra_kernels.hpp"
#include "ra_mesh_tri.hpp"
#include <hipcub/hipcub.hpp>

#pragma clang fp contract(off)

namespace {

constexpr unsigned MESH_KEY_DROPPED = 1u << 30;     // above every 30-bit code: dropped items sort behind the others
constexpr int MESH_BLOCK = 256;
constexpr float MESH_INF = __builtin_huge_valf();

__device__ __forceinline__ unsigned ord_enc(float f) {      // order-preserving float -> unsigned
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord_dec(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// item i of a build: the centroid of face i (faces != nullptr) or point i; false: non-finite
__device__ __forceinline__ bool mesh_item(const float* __restrict__ xyz, const int* __restrict__ faces, int i, float c[3]) {
    if (!faces) {
        c[0] = xyz[3 * (size_t)i]; c[1] = xyz[3 * (size_t)i + 1]; c[2] = xyz[3 * (size_t)i + 2];
        return finite3(c[0], c[1], c[2]);
    }
    bool ok = true;
    c[0] = c[1] = c[2] = 0.f;
    for (int k = 0; k < 3; ++k) {
        const float* v = xyz + 3 * (size_t)faces[3 * (size_t)i + k];
        ok = ok && finite3(v[0], v[1], v[2]);
        c[0] += v[0]; c[1] += v[1]; c[2] += v[2];
    }
    c[0] *= (1.f / 3.f); c[1] *= (1.f / 3.f); c[2] *= (1.f / 3.f);
    return ok && finite3(c[0], c[1], c[2]);
}

// box of the finite items: integer min / max on order-preserving words (bb: 3 x lo preset to ~0, 3 x hi preset to 0)
__global__ __launch_bounds__(MESH_BLOCK) void mesh_bbox_kernel(const float* __restrict__ xyz, const int* __restrict__ faces, int n, unsigned* __restrict__ bb) {
    const int i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    float c[3];
    const bool ok = i < n && mesh_item(xyz, faces, i, c);
    const bool any = __ballot(ok) != 0ull;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float lo = ok ? c[k] : MESH_INF, hi = ok ? c[k] : -MESH_INF;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
        if (any && (threadIdx.x & 63) == 0) { atomicMin(bb + k, ord_enc(lo)); atomicMax(bb + 3 + k, ord_enc(hi)); }
    }
}

__device__ __forceinline__ unsigned mesh_expand10(unsigned v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

__global__ __launch_bounds__(MESH_BLOCK) void mesh_keys_kernel(const float* __restrict__ xyz, const int* __restrict__ faces, int n,
                                                               const unsigned* __restrict__ bb, unsigned* __restrict__ keys, int* __restrict__ vals) {
    const int i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n) return;
    float c[3];
    unsigned key = MESH_KEY_DROPPED;
    if (mesh_item(xyz, faces, i, c)) {
        unsigned q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float lo = ord_dec(bb[k]), e = ord_dec(bb[3 + k]) - lo;
            const float scale = e > 0.f ? 1023.f / e : 0.f;         // a box of no extent in this dimension (one face, a planar mesh): cell 0
            q[k] = (unsigned)fminf(fmaxf((c[k] - lo) * scale, 0.f), 1023.f);
        }
        key = (mesh_expand10(q[0]) << 2) | (mesh_expand10(q[1]) << 1) | mesh_expand10(q[2]);
    }
    keys[i] = key;
    vals[i] = i;
}

// face records in sorted order (slots past the kept faces: id -1, zeros) and the box of every leaf's kept faces
__global__ __launch_bounds__(MESH_BLOCK) void mesh_leaves_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                 const unsigned* __restrict__ keys_sorted, const int* __restrict__ vals_sorted, int n_faces,
                                                                 int n_leaves, float* __restrict__ recs, float* __restrict__ lbox) {
    const int i = blockIdx.x * MESH_BLOCK + threadIdx.x, l = i / MESH_LEAF;
    const bool ok = l < n_leaves && i < n_faces && keys_sorted[i] != MESH_KEY_DROPPED;
    float t[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int id = -1;
    if (ok) {
        id = vals_sorted[i];
        for (int k = 0; k < 3; ++k) {
            const float* v = verts + 3 * (size_t)faces[3 * (size_t)id + k];
            t[3 * k] = v[0]; t[3 * k + 1] = v[1]; t[3 * k + 2] = v[2];
        }
    }
    if (l < n_leaves) {
        float4* r = reinterpret_cast<float4*>(recs + (size_t)i * MESH_REC);
        r[0] = make_float4(t[0], t[1], t[2], t[3]);
        r[1] = make_float4(t[4], t[5], t[6], t[7]);
        r[2] = make_float4(t[8], __int_as_float(id), 0.f, 0.f);
    }
    float lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = ok ? fminf(fminf(t[c], t[3 + c]), t[6 + c]) : MESH_INF;
        hi[c] = ok ? fmaxf(fmaxf(t[c], t[3 + c]), t[6 + c]) : -MESH_INF;
#pragma unroll
        for (int o = MESH_LEAF / 2; o > 0; o >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }
    }
    if (l < n_leaves && (i % MESH_LEAF) == 0) {
        if (lo[0] <= hi[0]) {           // the leaf holds a face: widen by more than a computed closest point can leave the exact box
            float m = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) m = fmaxf(m, fmaxf(fabsf(lo[c]), fabsf(hi[c])));
            const float pad = m * MESH_BOX_PAD;
#pragma unroll
            for (int c = 0; c < 3; ++c) { lo[c] -= pad; hi[c] += pad; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { lbox[6 * (size_t)l + c] = lo[c]; lbox[6 * (size_t)l + 3 + c] = hi[c]; }
    }
}

// a group of empty leaves keeps the empty box (lo = +inf, hi = -inf): infinitely far from everything
__global__ __launch_bounds__(MESH_BLOCK) void mesh_groups_kernel(const float* __restrict__ lbox, int n_leaves, int n_groups, float* __restrict__ gbox) {
    const int g = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (g >= n_groups) return;
    float lo[3] = {MESH_INF, MESH_INF, MESH_INF}, hi[3] = {-MESH_INF, -MESH_INF, -MESH_INF};
    for (int l = g * MESH_FAN; l < n_leaves && l < (g + 1) * MESH_FAN; ++l)
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], lbox[6 * (size_t)l + c]); hi[c] = fmaxf(hi[c], lbox[6 * (size_t)l + 3 + c]); }
#pragma unroll
    for (int c = 0; c < 3; ++c) { gbox[6 * (size_t)g + c] = lo[c]; gbox[6 * (size_t)g + 3 + c] = hi[c]; }
}

constexpr int MESH_QBLOCK = 64;      // one wave per workgroup: the waves share nothing, and a query of 10 000 points still spreads over 157 CUs

__global__ __launch_bounds__(MESH_QBLOCK) void mesh_closest_kernel(MeshView m, MeshQuery q) {
    const int i = blockIdx.x * MESH_QBLOCK + threadIdx.x;
    const bool in = i < q.n;
    const int pi = in ? (q.perm ? q.perm[i] : i) : 0;
    float p[3] = {0.f, 0.f, 0.f};
    if (in) { p[0] = q.pts[3 * (size_t)pi]; p[1] = q.pts[3 * (size_t)pi + 1]; p[2] = q.pts[3 * (size_t)pi + 2]; }
    // a non-finite point computes along on the origin and never votes: it cannot widen what its wave opens
    const bool alive = in && finite3(p[0], p[1], p[2]);
    if (!alive) p[0] = p[1] = p[2] = 0.f;
    const bool brute = q.brute != 0;
    MeshHit best;
    best.d2 = MESH_INF; best.x = best.y = best.z = best.u = best.v = best.w = __uint_as_float(0x7fc00000u);
    int bid = 0x7fffffff;
    float ub = MESH_INF;
    if (!brute)
        for (int g = 0; g < m.n_groups; ++g) ub = fminf(ub, m_box_far(p, m.gbox + 6 * (size_t)g));
    for (int g = 0; g < m.n_groups; ++g) {
        if (!brute) {
            const bool open = alive && !(m_box_near(p, m.gbox + 6 * (size_t)g) > fminf(best.d2, ub));
            if (__ballot(open) == 0ull) continue;
        }
        const int l1 = min(m.n_leaves, (g + 1) * MESH_FAN);
        for (int l = g * MESH_FAN; l < l1; ++l) {
            if (!brute) {
                const bool open = alive && !(m_box_near(p, m.lbox + 6 * (size_t)l) > fminf(best.d2, ub));
                if (__ballot(open) == 0ull) continue;
            }
            const float* rec = m.recs + (size_t)l * (MESH_LEAF * MESH_REC);
            for (int k = 0; k < MESH_LEAF; ++k, rec += MESH_REC) {
                const int id = __float_as_int(rec[9]);
                if (id < 0) break;              // kept faces come first in sorted order: nothing behind the first empty slot
                const float a[3] = {rec[0], rec[1], rec[2]}, b[3] = {rec[3], rec[4], rec[5]}, c[3] = {rec[6], rec[7], rec[8]};
                const MeshHit h = mesh_closest_tri(p, a, b, c);
                if (h.d2 < best.d2 || (h.d2 == best.d2 && id < bid)) { best = h; bid = id; }
            }
        }
    }
    if (!in) return;
    const float nanv = __uint_as_float(0x7fc00000u);
    const bool hit = alive && bid != 0x7fffffff;
    if (q.d2) q.d2[pi] = alive ? best.d2 : nanv;
    if (q.face) q.face[pi] = hit ? bid : -1;
    if (q.closest) { q.closest[3 * (size_t)pi] = hit ? best.x : nanv; q.closest[3 * (size_t)pi + 1] = hit ? best.y : nanv; q.closest[3 * (size_t)pi + 2] = hit ? best.z : nanv; }
    if (q.bary) { q.bary[3 * (size_t)pi] = hit ? best.u : nanv; q.bary[3 * (size_t)pi + 1] = hit ? best.v : nanv; q.bary[3 * (size_t)pi + 2] = hit ? best.w : nanv; }
}

inline int blocks(long long n) { return (int)((n + MESH_BLOCK - 1) / MESH_BLOCK); }

// keys of the n items (faces of verts, or points) and their sorted order into b.keys_sorted / b.vals_sorted
int sort_items(const float* xyz, const int* faces, int n, const MeshBuild& b, hipStream_t s) {
    if (hipMemsetAsync(b.bb, 0xff, 3 * sizeof(unsigned), s) != hipSuccess || hipMemsetAsync(b.bb + 3, 0, 3 * sizeof(unsigned), s) != hipSuccess) return 1;
    hipLaunchKernelGGL(mesh_bbox_kernel, dim3(blocks(n)), dim3(MESH_BLOCK), 0, s, xyz, faces, n, b.bb);
    hipLaunchKernelGGL(mesh_keys_kernel, dim3(blocks(n)), dim3(MESH_BLOCK), 0, s, xyz, faces, n, b.bb, b.keys, b.vals);
    size_t tb = b.temp_bytes;
    return hipcub::DeviceRadixSort::SortPairs(b.temp, tb, b.keys, b.keys_sorted, b.vals, b.vals_sorted, n, 0, 31, s) == hipSuccess ? 0 : 1;
}

}  // namespace

size_t mesh_sort_temp_bytes(int n) {
    size_t bytes = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const unsigned*)nullptr, (unsigned*)nullptr, (const int*)nullptr, (int*)nullptr, n, 0, 31);
    return bytes;
}

int launch_mesh_build(const float* verts, const MeshBuild& b, const MeshView& m, float* recs, float* lbox, float* gbox, hipStream_t s) {
    if (sort_items(verts, b.faces, m.n_faces, b, s)) return 1;
    hipLaunchKernelGGL(mesh_leaves_kernel, dim3(blocks((long long)m.n_leaves * MESH_LEAF)), dim3(MESH_BLOCK), 0, s, verts, b.faces, b.keys_sorted,
                       b.vals_sorted, m.n_faces, m.n_leaves, recs, lbox);
    hipLaunchKernelGGL(mesh_groups_kernel, dim3(blocks(m.n_groups)), dim3(MESH_BLOCK), 0, s, lbox, m.n_leaves, m.n_groups, gbox);
    return 0;
}

int launch_mesh_sort_points(const float* pts, int n, const MeshBuild& b, hipStream_t s) { return sort_items(pts, nullptr, n, b, s); }

void launch_mesh_closest(const MeshView& m, const MeshQuery& q, hipStream_t s) {
    hipLaunchKernelGGL(mesh_closest_kernel, dim3((q.n + MESH_QBLOCK - 1) / MESH_QBLOCK), dim3(MESH_QBLOCK), 0, s, m, q);
}

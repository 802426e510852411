// Mesh connectivity on the device (ra_topo_create) and what runs on it: Taubin smoothing (ra_mesh_smooth), one Loop subdivision
// step with the next level's connectivity (ra_mesh_subdivide) and the neighbour-OR dilation of a vertex mask (ra_topo_dilate) — the
// reference's triangle_to_halfedge, get_edges, get_face_connectivity, laplacian_smoothing and halfedge_loop_subdivision
// (lib/utils/mesh_utils.py:540-611, 898-922, 146-168, 943-1015, 382-514) without a host round trip.
//
// The build.  One 64-bit key per half-edge, (min << 32) | max of its two vertices, sorted with its half-edge index by one stable
// radix sort (as ra_mcubes.hip sorts for the component search).  Equal keys are one edge; a head flag and an exclusive sum number
// the edges in key order, which is the lexicographic (min, max) order the reference's hash.unique numbers them in.  Because the sort
// is stable the half-edges of an edge stand in ascending order: that run is the edge -> half-edge list, a run of exactly two is a
// twin pair (symmetric by construction), any other run of c gets twin = -c.
// The two vertex lists (neighbours from the unique edges, outgoing half-edges) are filled in any order through an integer counter
// per vertex and then sorted ascending inside each vertex's segment by the thread that owns the vertex: the stored lists are a
// function of the faces alone.  A segment is sorted by insertion, quadratic in the valence: meant for meshes, where the valence is
// about 6; a vertex of valence 10^4 costs 10^8 steps of one thread.
// Integer atomics only (counts, maxima, a flag): nothing depends on the order of execution.
//
// Smoothing.  One thread owns one (vertex, channel) result, channels fastest, so the C channels of a neighbour row are read by
// neighbouring lanes.  A pass reads one buffer and writes another (Jacobi, as the reference's L @ v before +=); the arithmetic is
// ra_topo_rules.hpp's taubin_step behind a sum over the neighbours in ascending order.
//
// Subdivision.  Positions: one thread per (output row, channel); an old vertex walks its outgoing half-edges, an edge vertex the
// half-edges of its edge, both ascending, and adds the contributions ra_topo_rules.hpp names.  The child's arrays: one thread per
// parent half-edge writes its four children (twin / vert / edge, the faces, the middle edge 2 E + h with its two half-edges), one
// thread per parent edge the two halves 2 e, 2 e + 1 with their lists and the outgoing list of the edge vertex; the neighbour lists
// follow from the child's edge ends as in the build.  All sizes are arithmetic on the parent's: no sort, no read-back.
#include "ra_kernels.hpp"
#include "ra_topo_rules.hpp"
#include <hipcub/hipcub.hpp>

#pragma clang fp contract(off)

namespace {

using u64 = unsigned long long;

inline int blocks(long long n, int per) { return (int)((n + per - 1) / per); }

__global__ __launch_bounds__(TOPO_BLOCK) void topo_keys_kernel(const int* __restrict__ faces, int n, int n_verts, int* __restrict__ vert,
                                                               u64* __restrict__ keys, int* __restrict__ slots, int* __restrict__ odeg,
                                                               int* __restrict__ stat) {
    const int h = blockIdx.x * TOPO_BLOCK + threadIdx.x;
    if (h >= n) return;
    int a = faces[h], b = faces[topo_next(h)];
    if (a < 0 || a >= n_verts) { atomicOr(stat + TOPO_BAD, 1); a = 0; }      // the call fails after the read-back; until then the index is harmless
    if (b < 0 || b >= n_verts) b = 0;                                        // reported by the thread that owns it
    vert[h] = a;
    keys[h] = topo_edge_key(a, b);
    slots[h] = h;
    atomicAdd(odeg + a, 1);
}

__global__ __launch_bounds__(TOPO_BLOCK) void topo_heads_kernel(const u64* __restrict__ ks, int n, int* __restrict__ head) {
    const int i = blockIdx.x * TOPO_BLOCK + threadIdx.x;
    if (i > n) return;
    head[i] = i < n && (i == 0 || ks[i] != ks[i - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(TOPO_BLOCK) void topo_edges_kernel(const u64* __restrict__ ks, const int* __restrict__ ehe, const int* __restrict__ head,
                                                                const int* __restrict__ off, int n, int* __restrict__ edge, int* __restrict__ edges,
                                                                int* __restrict__ ehe_start, int* __restrict__ deg, int* __restrict__ stat) {
    const int i = blockIdx.x * TOPO_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int e = off[i] + head[i] - 1;      // 0 <= e < E <= n
    edge[ehe[i]] = e;
    if (head[i]) {
        const int lo = topo_key_min(ks[i]), hi = topo_key_max(ks[i]);
        edges[2 * e] = lo;
        edges[2 * e + 1] = hi;
        ehe_start[e] = i;
        atomicAdd(deg + lo, 1);
        atomicAdd(deg + hi, 1);       // an edge (a, a) counts twice, as the reference's coalesced adjacency entry of 2 does
    }
    if (i == 0) {
        const int E = off[n];
        ehe_start[E] = n;
        stat[TOPO_E] = E;
    }
}

__global__ __launch_bounds__(TOPO_BLOCK) void topo_twins_kernel(const int* __restrict__ ehe, const int* __restrict__ head, const int* __restrict__ off,
                                                                const int* __restrict__ ehe_start, int n, int* __restrict__ twin,
                                                                int* __restrict__ counts, int* __restrict__ stat) {
    const int i = blockIdx.x * TOPO_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int e = off[i] + head[i] - 1;
    const int start = ehe_start[e], count = ehe_start[e + 1] - start;
    if (head[i]) { counts[e] = count; atomicMax(stat + TOPO_MAX_COUNT, count); }
    const int p = topo_twin_pos(i, start, count);       // inside [start, start + 2) when count == 2
    twin[ehe[i]] = p >= 0 ? ehe[p] : -count;
}

__global__ __launch_bounds__(TOPO_BLOCK) void topo_fill_nbr_kernel(const int* __restrict__ edges, const int* __restrict__ off, int n,
                                                                   const int* __restrict__ nbr_start, int* __restrict__ fill, int* __restrict__ nbr) {
    const int e = blockIdx.x * TOPO_BLOCK + threadIdx.x;
    if (e >= off[n]) return;        // off[n] = E <= n
    const int a = edges[2 * e], b = edges[2 * e + 1];
    nbr[nbr_start[a] + atomicAdd(fill + a, 1)] = b;     // fill[a] ends at deg[a] = nbr_start[a + 1] - nbr_start[a]
    nbr[nbr_start[b] + atomicAdd(fill + b, 1)] = a;
}

__global__ __launch_bounds__(TOPO_BLOCK) void topo_fill_out_kernel(const int* __restrict__ vert, int n, const int* __restrict__ out_start,
                                                                   int* __restrict__ fill, int* __restrict__ out_he) {
    const int h = blockIdx.x * TOPO_BLOCK + threadIdx.x;
    if (h >= n) return;
    const int a = vert[h];
    out_he[out_start[a] + atomicAdd(fill + a, 1)] = h;
}

// ascending order inside every vertex's segment, and the longest segment
__global__ __launch_bounds__(TOPO_BLOCK) void topo_sort_segments_kernel(const int* __restrict__ start, int n_verts, int* __restrict__ list,
                                                                        int* __restrict__ longest) {
    const int v = blockIdx.x * TOPO_BLOCK + threadIdx.x;
    if (v >= n_verts) return;
    const int s = start[v], e = start[v + 1];
    for (int i = s + 1; i < e; ++i) {
        const int x = list[i];
        int j = i - 1;
        for (; j >= s && list[j] > x; --j) list[j + 1] = list[j];
        list[j + 1] = x;
    }
    if (e - s > 0) atomicMax(longest, e - s);
}

__global__ __launch_bounds__(TOPO_SMOOTH_BLOCK) void topo_smooth_kernel(const int* __restrict__ nbr_start, const int* __restrict__ nbr, long long total, int C,
                                                                        const float* __restrict__ src, const unsigned char* __restrict__ move, float c,
                                                                        float* __restrict__ dst) {
    const long long idx = (long long)blockIdx.x * TOPO_SMOOTH_BLOCK + threadIdx.x;
    if (idx >= total) return;
    const int v = (int)(idx / C), ch = (int)(idx - (long long)v * C);
    const float x = src[idx];
    if (move && !move[v]) { dst[idx] = x; return; }
    const int s = nbr_start[v], e = nbr_start[v + 1];
    float sum = 0.0f;
    for (int k = s; k < e; ++k) sum = sum + src[(long long)nbr[k] * C + ch];
    dst[idx] = taubin_step(x, sum, taubin_inv(e - s), c);
}

__global__ __launch_bounds__(TOPO_SMOOTH_BLOCK) void topo_mark_rows_kernel(const long long* __restrict__ inds, int n_inds, int n_verts,
                                                                           unsigned char* __restrict__ move) {
    const int i = blockIdx.x * TOPO_SMOOTH_BLOCK + threadIdx.x;
    if (i >= n_inds) return;
    const long long v = inds[i];
    if (v >= 0 && v < n_verts) move[v] = 1;       // an index outside the mesh names no row
}

__global__ __launch_bounds__(TOPO_SMOOTH_BLOCK) void topo_dilate_kernel(const int* __restrict__ nbr_start, const int* __restrict__ nbr, int n_verts,
                                                                        const unsigned char* __restrict__ src, unsigned char* __restrict__ dst) {
    const int v = blockIdx.x * TOPO_SMOOTH_BLOCK + threadIdx.x;
    if (v >= n_verts) return;
    unsigned char any = 0;
    for (int k = nbr_start[v]; k < nbr_start[v + 1]; ++k) any |= src[nbr[k]] != 0;
    dst[v] = any;
}

// One Loop step, positions: one thread per (output row, channel), channels fastest; a row adds its half-edges' contributions
// (ra_topo_rules.hpp) in ascending half-edge order, so its value does not depend on the launch
__global__ __launch_bounds__(TOPO_SMOOTH_BLOCK) void loop_positions_kernel(TopoView t, long long total, int C, const float* __restrict__ src,
                                                                           const float* __restrict__ weights, float* __restrict__ dst) {
    const long long idx = (long long)blockIdx.x * TOPO_SMOOTH_BLOCK + threadIdx.x;
    if (idx >= total) return;
    const int row = (int)(idx / C), ch = (int)(idx - (long long)row * C);
    float acc = 0.0f;
    if (row < t.n_verts) {
        const int s = t.out_start[row], e = t.out_start[row + 1], n = e - s;
        bool open = false;
        for (int k = s; k < e; ++k) open = open || t.twin[t.out_he[k]] < 0;
        const float w_self = weights[2 * n], beta = weights[2 * n + 1];      // n <= the largest outgoing count the table was built for
        for (int k = s; k < e; ++k) {
            const int h = t.out_he[k];
            const float v = src[(long long)t.vert[h] * C + ch];
            const float v_next = src[(long long)t.vert[topo_next(h)] * C + ch];
            float c = open ? 0.0f : loop_vert_inner(v, v_next, w_self, beta);
            if (t.twin[h] < 0) c = c + loop_vert_open(v, v_next);
            const int tp = t.twin[topo_prev(h)];
            if (tp >= 0) {
                const int in = topo_prev(tp);       // arrives at this vertex in the neighbouring face
                if (t.twin[in] < 0) c = c + loop_vert_open(src[(long long)t.vert[tp] * C + ch], src[(long long)t.vert[in] * C + ch]);
            }
            acc = acc + c;
        }
    } else {
        const int ed = row - t.n_verts;
        for (int k = t.ehe_start[ed]; k < t.ehe_start[ed + 1]; ++k) {
            const int h = t.ehe[k], tw = t.twin[h];
            const float v = src[(long long)t.vert[h] * C + ch];
            const float c = tw >= 0 ? loop_edge_inner(v, src[(long long)t.vert[topo_prev(h)] * C + ch])
                                    : loop_edge_open(v, src[(long long)t.vert[topo_next(h)] * C + ch], -tw);
            acc = acc + c;
        }
    }
    dst[idx] = acc;
}

// The child's half-edge arrays, its faces, and everything of its middle edges 2 E + h: one thread per parent half-edge
__global__ __launch_bounds__(TOPO_BLOCK) void child_halfedges_kernel(TopoView t, TopoChild c, int* __restrict__ faces_out) {
    const int h = blockIdx.x * TOPO_BLOCK + threadIdx.x;
    const int HE = 3 * t.n_faces, V = t.n_verts, E = t.n_edges;
    if (h >= HE) return;
    const int pv = topo_prev(h), tw = t.twin[h], tp = t.twin[pv], e = t.edge[h], ep = t.edge[pv];
    const int i0 = 3 * h, i1 = 3 * h + 1, i2 = 3 * h + 2, i3 = 3 * HE + h;
    c.twin[i0] = child_twin0(tw); c.twin[i1] = i3; c.twin[i2] = child_twin2(tp); c.twin[i3] = i1;
    c.edge[i0] = child_edge0(e, h, tw); c.edge[i1] = 2 * E + h; c.edge[i2] = child_edge2(ep, pv, tp); c.edge[i3] = 2 * E + h;
    const int a = t.vert[h], m = V + e, mp = V + ep;
    c.vert[i0] = a; c.vert[i1] = m; c.vert[i2] = mp; c.vert[i3] = mp;
    if (faces_out) { faces_out[i0] = a; faces_out[i1] = m; faces_out[i2] = mp; faces_out[i3] = mp; }
    const int ce = 2 * E + h;
    c.counts[ce] = 2;
    c.ehe_start[ce] = 2 * HE + 2 * h;
    c.ehe[2 * HE + 2 * h] = i1;
    c.ehe[2 * HE + 2 * h + 1] = i3;
    c.edges[2 * ce] = m < mp ? m : mp;
    c.edges[2 * ce + 1] = m < mp ? mp : m;
    c.out_he[h] = 3 * t.out_he[h];          // the old vertices keep their lists: child 3 h leaves vert[h]
    if (h == 0) { c.ehe_start[2 * E + HE] = 4 * HE; c.out_start[V + E] = 4 * HE; }
}

__device__ __forceinline__ void topo_insertion_sort(int* list, int n) {
    for (int i = 1; i < n; ++i) {
        const int x = list[i];
        int j = i - 1;
        for (; j >= 0 && list[j] > x; --j) list[j + 1] = list[j];
        list[j + 1] = x;
    }
}

// The two halves 2 e, 2 e + 1 of every parent edge and the outgoing list of its edge vertex: one thread per parent edge.  Runs behind
// child_halfedges_kernel (it reads the child's vert)
__global__ __launch_bounds__(TOPO_BLOCK) void child_edges_kernel(TopoView t, TopoChild c) {
    const int e = blockIdx.x * TOPO_BLOCK + threadIdx.x;
    const int HE = 3 * t.n_faces, V = t.n_verts;
    if (e >= t.n_edges) return;
    const int s = t.ehe_start[e], n = t.ehe_start[e + 1] - s;
    int* half[2] = {c.ehe + 2 * s, c.ehe + 2 * s + n};      // n entries each: 2 s + 2 n <= 2 HE
    int fill[2] = {0, 0};
    int* out = c.out_he + HE + 3 * s;                       // 3 n entries: HE + 3 s + 3 n <= 4 HE
    for (int j = 0; j < n; ++j) {
        const int h = t.ehe[s + j], tw = t.twin[h], nx = topo_next(h);
        const int k0 = child_edge0(e, h, tw) - 2 * e, k2 = child_edge2(e, h, tw) - 2 * e;       // next h's third half-edge lies on this edge
        if (fill[k0] < n) half[k0][fill[k0]++] = 3 * h;
        if (fill[k2] < n) half[k2][fill[k2]++] = 3 * nx + 2;
        out[3 * j] = 3 * h + 1; out[3 * j + 1] = 3 * nx + 2; out[3 * j + 2] = 3 * HE + nx;
    }
    topo_insertion_sort(out, 3 * n);
    c.out_start[V + e] = HE + 3 * s;
    for (int k = 0; k < 2; ++k) {
        topo_insertion_sort(half[k], fill[k]);
        const int ce = 2 * e + k, x = fill[k] > 0 ? half[k][0] : 3 * t.ehe[s];      // each half holds n >= 1: the ends of its lowest half-edge name it
        const int a = c.vert[x], b = c.vert[topo_next(x)];
        c.counts[ce] = n;
        c.ehe_start[ce] = 2 * s + k * n;
        c.edges[2 * ce] = a < b ? a : b;
        c.edges[2 * ce + 1] = a < b ? b : a;
    }
}

__global__ __launch_bounds__(TOPO_BLOCK) void child_out_start_kernel(const int* __restrict__ out_start, int n_verts, int* __restrict__ child_out_start) {
    const int v = blockIdx.x * TOPO_BLOCK + threadIdx.x;
    if (v < n_verts) child_out_start[v] = out_start[v];
}

__global__ __launch_bounds__(TOPO_BLOCK) void topo_edge_degrees_kernel(const int* __restrict__ edges, int n_edges, int* __restrict__ deg) {
    const int e = blockIdx.x * TOPO_BLOCK + threadIdx.x;
    if (e >= n_edges) return;
    atomicAdd(deg + edges[2 * e], 1);
    atomicAdd(deg + edges[2 * e + 1], 1);
}

__global__ __launch_bounds__(TOPO_BLOCK) void topo_fill_nbr_n_kernel(const int* __restrict__ edges, int n_edges, const int* __restrict__ nbr_start,
                                                                     int* __restrict__ fill, int* __restrict__ nbr) {
    const int e = blockIdx.x * TOPO_BLOCK + threadIdx.x;
    if (e >= n_edges) return;
    const int a = edges[2 * e], b = edges[2 * e + 1];
    nbr[nbr_start[a] + atomicAdd(fill + a, 1)] = b;
    nbr[nbr_start[b] + atomicAdd(fill + b, 1)] = a;
}

}  // namespace

size_t topo_temp_bytes(int n_faces, int n_verts) {
    const int n = 3 * n_faces, m = (n > n_verts ? n : n_verts) + 1;
    size_t a = 0, b = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const u64*)nullptr, (u64*)nullptr, (const int*)nullptr, (int*)nullptr, n, 0, 64);
    hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const int*)nullptr, (int*)nullptr, m);
    return a > b ? a : b;
}

// n_faces >= 1 and n_verts >= 1; deg, odeg (V + 1 each), fill (V) and stat are zero on entry
int launch_topo_build(const TopoBuild& b, hipStream_t s) {
    const int n = 3 * b.n_faces, V = b.n_verts;
    size_t tb = b.temp_bytes;
    hipLaunchKernelGGL(topo_keys_kernel, dim3(blocks(n, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, b.faces, n, V, b.vert, b.keys, b.slots, b.odeg, b.stat);
    if (hipcub::DeviceRadixSort::SortPairs(b.temp, tb, b.keys, b.keys_sorted, b.slots, b.ehe, n, 0, 64, s) != hipSuccess) return 1;
    hipLaunchKernelGGL(topo_heads_kernel, dim3(blocks(n + 1, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, b.keys_sorted, n, b.head);
    tb = b.temp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(b.temp, tb, b.head, b.off, n + 1, s) != hipSuccess) return 1;
    hipLaunchKernelGGL(topo_edges_kernel, dim3(blocks(n, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, b.keys_sorted, b.ehe, b.head, b.off, n, b.edge, b.edges,
                       b.ehe_start, b.deg, b.stat);
    hipLaunchKernelGGL(topo_twins_kernel, dim3(blocks(n, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, b.ehe, b.head, b.off, b.ehe_start, n, b.twin, b.counts, b.stat);
    tb = b.temp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(b.temp, tb, b.deg, b.nbr_start, V + 1, s) != hipSuccess) return 1;
    tb = b.temp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(b.temp, tb, b.odeg, b.out_start, V + 1, s) != hipSuccess) return 1;
    hipLaunchKernelGGL(topo_fill_nbr_kernel, dim3(blocks(n, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, b.edges, b.off, n, b.nbr_start, b.fill, b.nbr);
    hipLaunchKernelGGL(topo_sort_segments_kernel, dim3(blocks(V, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, b.nbr_start, V, b.nbr, b.stat + TOPO_MAX_NBR);
    if (hipMemsetAsync(b.fill, 0, (size_t)V * sizeof(int), s) != hipSuccess) return 1;
    hipLaunchKernelGGL(topo_fill_out_kernel, dim3(blocks(n, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, b.vert, n, b.out_start, b.fill, b.out_he);
    hipLaunchKernelGGL(topo_sort_segments_kernel, dim3(blocks(V, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, b.out_start, V, b.out_he, b.stat + TOPO_MAX_OUT);
    return 0;
}

void launch_topo_smooth_pass(const TopoView& t, const float* src, int C, const unsigned char* move, float c, float* dst, hipStream_t s) {
    const long long total = (long long)t.n_verts * C;
    if (total == 0) return;
    hipLaunchKernelGGL(topo_smooth_kernel, dim3(blocks(total, TOPO_SMOOTH_BLOCK)), dim3(TOPO_SMOOTH_BLOCK), 0, s, t.nbr_start, t.nbr, total, C, src, move, c, dst);
}

void launch_topo_mark_rows(const long long* inds, int n_inds, int n_verts, unsigned char* move, hipStream_t s) {
    if (n_inds == 0) return;
    hipLaunchKernelGGL(topo_mark_rows_kernel, dim3(blocks(n_inds, TOPO_SMOOTH_BLOCK)), dim3(TOPO_SMOOTH_BLOCK), 0, s, inds, n_inds, n_verts, move);
}

void launch_topo_dilate_pass(const TopoView& t, const unsigned char* src, unsigned char* dst, hipStream_t s) {
    if (t.n_verts == 0) return;
    hipLaunchKernelGGL(topo_dilate_kernel, dim3(blocks(t.n_verts, TOPO_SMOOTH_BLOCK)), dim3(TOPO_SMOOTH_BLOCK), 0, s, t.nbr_start, t.nbr, t.n_verts, src, dst);
}

void launch_loop_positions(const TopoView& t, const float* src, int C, const float* weights, float* dst, hipStream_t s) {
    const long long total = ((long long)t.n_verts + t.n_edges) * C;
    if (total == 0) return;
    hipLaunchKernelGGL(loop_positions_kernel, dim3(blocks(total, TOPO_SMOOTH_BLOCK)), dim3(TOPO_SMOOTH_BLOCK), 0, s, t, total, C, src, weights, dst);
}

// n_faces >= 1 (hence n_edges >= 1)
int launch_topo_child(const TopoView& t, const TopoChild& c, int* faces_out, hipStream_t s) {
    const int HE = 3 * t.n_faces, V = t.n_verts, E = t.n_edges, V2 = V + E, E2 = 2 * E + HE;
    hipLaunchKernelGGL(child_halfedges_kernel, dim3(blocks(HE, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, t, c, faces_out);
    hipLaunchKernelGGL(child_edges_kernel, dim3(blocks(E, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, t, c);
    hipLaunchKernelGGL(child_out_start_kernel, dim3(blocks(V, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, t.out_start, V, c.out_start);
    // the neighbour lists from the child's edges, as the build makes them from the unique edges
    hipLaunchKernelGGL(topo_edge_degrees_kernel, dim3(blocks(E2, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, c.edges, E2, c.deg);
    size_t tb = c.temp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(c.temp, tb, c.deg, c.nbr_start, V2 + 1, s) != hipSuccess) return 1;
    hipLaunchKernelGGL(topo_fill_nbr_n_kernel, dim3(blocks(E2, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, c.edges, E2, c.nbr_start, c.fill, c.nbr);
    hipLaunchKernelGGL(topo_sort_segments_kernel, dim3(blocks(V2, TOPO_BLOCK)), dim3(TOPO_BLOCK), 0, s, c.nbr_start, V2, c.nbr, c.scratch_stat + TOPO_MAX_NBR);
    return 0;
}

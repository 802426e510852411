// ra_mesh_closest_backward on the device: the gradient of the closest-point query in the points, the mesh's vertices and per-vertex
// attributes.  The arithmetic of a row is ra_mesh_grad_rules.hpp's, which also states the rule.  READ-BACKS: NONE.
//
// mesh_grad_row_kernel.  One lane per row: dpts, and the row's three keys vertex x 3 n + (3 i + k), or the largest key (V x 3 n) three
//     times for a dead row.  The keys are NOT compacted: the inert ones sort to the end and no wave works on them.
// One stable radix sort (hipcub) over the 3 n keys, restricted to the bits in use, groups the slots by vertex, ascending inside a run.
// mesh_grad_mark_kernel marks the sorted indices that start a vertex's run; hipcub::DeviceSelect::Flagged compacts their indices, the count
//     stays on the device.  (Measured against launching a wave per sorted index that leaves unless it heads a run, ra_texture.hip's way:
//     equal on short runs, 2.9 x faster at 3 000 000 slots on 6 890 vertices, the same bits)
// mesh_grad_run_kernel.  One wave per POSSIBLE run, min(3 n, V) of them; wave w takes the run at heads[w] or leaves.  The payload of a
//     slot is recomputed from the row (the same operations as the row kernel's, so the same bits whether dpts was asked for or not);
//     dverts is one group of three channels, dattr goes in groups of MESHG_GROUP; lane l adds slots l, l + 64, ... until it meets a key
//     of another run, the lanes meet in the xor tree 32, 16, .., 1 and lane 0 writes.  The vertex-sized outputs were zeroed before, so
//     a vertex without a slot holds +0.  No float atomics: a result is a function of the inputs in their given order alone.
#include "ra_mesh_grad.hpp"
#include <hipcub/hipcub.hpp>

#pragma clang fp contract(off)

namespace {

using u64 = unsigned long long;

inline int blocks(long long n, int per) { return (int)((n + per - 1) / per); }

__global__ __launch_bounds__(MESHG_BLOCK) void mesh_grad_row_kernel(MeshGradJob j, u64* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * MESHG_BLOCK + threadIdx.x;
    if (i >= j.n) return;
    int idx[3];
    const bool live = mesh_grad_live(j.face[i], j.faces, j.F, j.V, idx);
    if (j.dpts) {
        float d[3] = {0.0f, 0.0f, 0.0f};
        if (live) {
            const float p[3] = {j.pts[3 * i], j.pts[3 * i + 1], j.pts[3 * i + 2]};
            const float q[3] = {j.closest[3 * i], j.closest[3 * i + 1], j.closest[3 * i + 2]};
            mesh_grad_dpts(p, q, j.g_d2[i], d);
        }
        float* dst = j.dpts + 3 * i;
        dst[0] = d[0]; dst[1] = d[1]; dst[2] = d[2];
    }
    if (keys) {
        const u64 slots = 3ull * (u64)j.n, inert = (u64)j.V * slots;
#pragma unroll
        for (int k = 0; k < 3; ++k) keys[3 * i + k] = live ? (u64)idx[k] * slots + (u64)(3 * i + k) : inert;
    }
}

__device__ __forceinline__ float wave_tree(float x) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) x = x + __shfl_xor(x, w, 64);
    return x;
}

// the wave's work on the run of vertex `vert` that starts at sorted index lo
__device__ __forceinline__ void mesh_grad_run(const MeshGradJob& j, const u64* __restrict__ keys, long long n_keys, long long lo, u64 vert) {
    const u64 slots = 3ull * (u64)j.n;
    const int lane = threadIdx.x;
    if (j.dverts) {
        float G[3] = {0.0f, 0.0f, 0.0f};
        for (long long s = lo + lane; s < n_keys; s += 64) {        // the keys are sorted: a lane leaves at the first key of another run
            const u64 key = keys[s];
            if (key / slots != vert) break;
            const long long slot = (long long)(key - vert * slots), i = slot / 3;
            const float p[3] = {j.pts[3 * i], j.pts[3 * i + 1], j.pts[3 * i + 2]};
            const float q[3] = {j.closest[3 * i], j.closest[3 * i + 1], j.closest[3 * i + 2]};
            float d[3];
            mesh_grad_dpts(p, q, j.g_d2[i], d);
            const float b = j.bary[slot];                           // slot = 3 i + k
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float term = mesh_grad_vert_term(b, d[c]);
                G[c] = G[c] + term;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) G[c] = wave_tree(G[c]);
        if (lane == 0)
            for (int c = 0; c < 3; ++c) j.dverts[vert * 3ull + (u64)c] = G[c];
    }
    if (!j.dattr) return;
    for (int c0 = 0; c0 < j.C; c0 += MESHG_GROUP) {
        float G[MESHG_GROUP];
#pragma unroll
        for (int k = 0; k < MESHG_GROUP; ++k) G[k] = 0.0f;
        for (long long s = lo + lane; s < n_keys; s += 64) {
            const u64 key = keys[s];
            if (key / slots != vert) break;
            const long long slot = (long long)(key - vert * slots), i = slot / 3;
            const float b = j.bary[slot];
            const float* ga = j.g_attr + i * j.C;
#pragma unroll
            for (int k = 0; k < MESHG_GROUP; ++k)
                if (c0 + k < j.C) {
                    const float term = mesh_grad_attr_term(b, ga[c0 + k]);
                    G[k] = G[k] + term;
                }
        }
#pragma unroll
        for (int k = 0; k < MESHG_GROUP; ++k) G[k] = wave_tree(G[k]);
        if (lane == 0)
            for (int k = 0; k < MESHG_GROUP; ++k)
                if (c0 + k < j.C) j.dattr[vert * (u64)j.C + (u64)(c0 + k)] = G[k];
    }
}

// 1 where sorted index i starts the run of a vertex (the inert keys start none)
__global__ __launch_bounds__(MESHG_BLOCK) void mesh_grad_mark_kernel(const u64* __restrict__ keys, long long n_keys, u64 slots, u64 V,
                                                                       unsigned char* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * MESHG_BLOCK + threadIdx.x;
    if (i >= n_keys) return;
    const u64 vert = keys[i] / slots;
    flags[i] = vert < V && (i == 0 || keys[i - 1] / slots != vert);
}

// one wave per POSSIBLE run: wave w works on the run that starts at heads[w], or leaves when there are fewer runs (the count stays on the device)
__global__ __launch_bounds__(64) void mesh_grad_run_kernel(MeshGradJob j, const u64* __restrict__ keys, long long n_keys, long long first,
                                                           const unsigned* __restrict__ heads, const unsigned* __restrict__ n_heads) {
    const long long w = first + blockIdx.x;
    if (w >= (long long)*n_heads) return;
    const long long lo = heads[w];
    mesh_grad_run(j, keys, n_keys, lo, keys[lo] / (3ull * (u64)j.n));
}

}  // namespace

size_t mesh_grad_sort_bytes(long long n_keys) {
    size_t b = 0;
    if (n_keys > 0) hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const u64*)nullptr, (u64*)nullptr, (size_t)n_keys, 0, 64);
    return b;
}

size_t mesh_grad_select_bytes(long long n_keys) {
    size_t b = 0;
    if (n_keys > 0)
        hipcub::DeviceSelect::Flagged(nullptr, b, hipcub::CountingInputIterator<unsigned>(0u), (unsigned char*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr,
                                      (size_t)n_keys);
    return b;
}

int launch_mesh_closest_backward(const MeshGradJob& j, const MeshGradScratch& t, hipStream_t s) {
    const bool runs = j.dverts || (j.dattr && j.C > 0);
    if (j.dverts && hipMemsetAsync(j.dverts, 0, (size_t)j.V * 3 * sizeof(float), s) != hipSuccess) return 1;
    if (j.dattr && j.C > 0 && hipMemsetAsync(j.dattr, 0, (size_t)j.V * j.C * sizeof(float), s) != hipSuccess) return 1;
    if (j.n == 0 || (!runs && !j.dpts)) return 0;
    hipLaunchKernelGGL(mesh_grad_row_kernel, dim3(blocks(j.n, MESHG_BLOCK)), dim3(MESHG_BLOCK), 0, s, j, runs ? t.keys : (u64*)nullptr);
    if (!runs) return 0;
    const long long n_keys = 3ll * j.n;
    const u64 largest = (u64)j.V * (u64)n_keys;
    int end_bit = 1;
    size_t sort_bytes = t.sort_bytes, select_bytes = t.select_bytes;
    while (end_bit < 64 && (largest >> end_bit) != 0) ++end_bit;
    if (hipcub::DeviceRadixSort::SortKeys(t.sort_temp, sort_bytes, (const u64*)t.keys, t.sorted, (size_t)n_keys, 0, end_bit, s) != hipSuccess)
        return 1;
    hipLaunchKernelGGL(mesh_grad_mark_kernel, dim3(blocks(n_keys, MESHG_BLOCK)), dim3(MESHG_BLOCK), 0, s, (const u64*)t.sorted, n_keys, (u64)n_keys, (u64)j.V, t.flags);
    if (hipcub::DeviceSelect::Flagged(t.select_temp, select_bytes, hipcub::CountingInputIterator<unsigned>(0u), t.flags, t.heads, t.count,
                                      (size_t)n_keys, s) != hipSuccess)
        return 1;
    const long long waves = n_keys < (long long)j.V ? n_keys : (long long)j.V;      // no more runs than slots, nor than vertices
    for (long long first = 0; first < waves; first += MESHG_MAX_WAVES) {           // a launch stays far below 2^32 threads
        const long long m = waves - first < MESHG_MAX_WAVES ? waves - first : MESHG_MAX_WAVES;
        hipLaunchKernelGGL(mesh_grad_run_kernel, dim3((unsigned)m), dim3(64), 0, s, j, (const u64*)t.sorted, n_keys, first, (const unsigned*)t.heads,
                           (const unsigned*)t.count);
    }
    return 0;
}

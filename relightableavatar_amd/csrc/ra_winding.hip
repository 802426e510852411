// Generalised winding number of a triangle mesh (ra_mesh_winding): the reference's winding_number (lib/utils/mesh_utils.py:614-680,
// Jacobson et al. 2013), the inside / outside test that survives holes, flipped faces and open boundaries.  Dense by definition: every
// point sees every kept face; nothing is pruned.
//
// One lane per point, one wave per workgroup (the waves share nothing).  The faces are the records the mesh already owns (ra_mesh.hip:
// 48 bytes a.xyz b.xyz c.xyz id, Morton order, kept faces first), walked with a wave-uniform address — scalar loads, no LDS, no
// per-lane divergence over faces — and winding_tri (ra_winding_tri.hpp) is all VALU: three reciprocal square roots' worth of
// normalisation, a hypot, two divisions and an arctangent per pair.
//
// Determinism.  A point's result is a function of (point, mesh) alone.  The faces are summed in stored order in chunks of WIND_CHUNK
// records, a constant: every chunk's sum starts from 0 in float64 and the chunk sums are added in chunk order, in float64.  The
// one-pass kernel does both in a lane; where few points would leave the chip idle, the split launch gives every (point tile, chunk)
// its own workgroup, which stores the chunk's sum, and a second kernel adds the stored sums in the same chunk order: the same additions
// in the same order, so the same bits.  No atomics.
#include "ra_kernels.hpp"
#include "ra_winding_tri.hpp"

#pragma clang fp contract(off)

namespace {

constexpr double WIND_INV_4PI = 0.07957747154594767;       // 1 / (4 pi)

__device__ __forceinline__ void wind_point(const float* __restrict__ pts, int n, int i, float p[3]) {
    const int k = i < n ? i : 0;       // idle lanes compute along on point 0 and store nothing (n >= 1)
    p[0] = pts[3 * (size_t)k]; p[1] = pts[3 * (size_t)k + 1]; p[2] = pts[3 * (size_t)k + 2];
}

// the float64 sum of chunk c's solid angles, in stored order from 0
__device__ __forceinline__ double wind_chunk(const MeshView& m, int c, const float p[3]) {
    const int n_slots = m.n_leaves * MESH_LEAF;
    const int k0 = c * WIND_CHUNK, k1 = min(n_slots, k0 + WIND_CHUNK);
    const float* rec = m.recs + (size_t)k0 * MESH_REC;
    double s = 0.0;
    if (k0 >= k1) return s;
    // the next record is requested before this one is used: a pair is some 800 cycles of VALU work, a scalar load a few hundred of latency
    float4 r0 = reinterpret_cast<const float4*>(rec)[0], r1 = reinterpret_cast<const float4*>(rec)[1], r2 = reinterpret_cast<const float4*>(rec)[2];
    for (int k = k0; k < k1; ++k) {
        const float a[3] = {r0.x, r0.y, r0.z}, b[3] = {r0.w, r1.x, r1.y}, cc[3] = {r1.z, r1.w, r2.x};
        if (__float_as_int(r2.y) < 0) break;        // kept faces come first in sorted order: nothing behind the first empty slot
        if (k + 1 < k1) {
            rec += MESH_REC;
            r0 = reinterpret_cast<const float4*>(rec)[0]; r1 = reinterpret_cast<const float4*>(rec)[1]; r2 = reinterpret_cast<const float4*>(rec)[2];
        }
        s += (double)winding_tri(p, a, b, cc);
    }
    return s;
}

__global__ __launch_bounds__(WIND_BLOCK) void winding_kernel(MeshView m, const float* __restrict__ pts, int n, int n_chunks, float* __restrict__ out) {
    const int i = blockIdx.x * WIND_BLOCK + threadIdx.x;
    float p[3];
    wind_point(pts, n, i, p);
    double total = 0.0;
    for (int c = 0; c < n_chunks; ++c) total += wind_chunk(m, c, p);
    if (i < n) out[i] = (float)(total * WIND_INV_4PI);
}

// partial: n_chunks x n float64, chunk-major
__global__ __launch_bounds__(WIND_BLOCK) void winding_split_kernel(MeshView m, const float* __restrict__ pts, int n, double* __restrict__ partial) {
    const int i = blockIdx.x * WIND_BLOCK + threadIdx.x, c = blockIdx.y;
    float p[3];
    wind_point(pts, n, i, p);
    const double s = wind_chunk(m, c, p);
    if (i < n) partial[(size_t)c * n + i] = s;
}

__global__ __launch_bounds__(WIND_BLOCK) void winding_combine_kernel(const double* __restrict__ partial, int n, int n_chunks, float* __restrict__ out) {
    const int i = blockIdx.x * WIND_BLOCK + threadIdx.x;
    if (i >= n) return;
    double total = 0.0;
    for (int c = 0; c < n_chunks; ++c) total += partial[(size_t)c * n + i];
    out[i] = (float)(total * WIND_INV_4PI);
}

}  // namespace

void launch_mesh_winding(const MeshView& m, const float* pts, int n, double* partial, float* out, hipStream_t s) {
    const int tiles = (n + WIND_BLOCK - 1) / WIND_BLOCK, n_chunks = wind_chunk_count(m.n_leaves);
    if (!partial) {
        hipLaunchKernelGGL(winding_kernel, dim3(tiles), dim3(WIND_BLOCK), 0, s, m, pts, n, n_chunks, out);
        return;
    }
    hipLaunchKernelGGL(winding_split_kernel, dim3(tiles, n_chunks), dim3(WIND_BLOCK), 0, s, m, pts, n, partial);
    hipLaunchKernelGGL(winding_combine_kernel, dim3(tiles), dim3(WIND_BLOCK), 0, s, partial, n, n_chunks, out);
}

// The generalised winding number of a triangle mesh WITH its gradient in the query point (ra_mesh_winding_grad): what a fit needs to
// pull a surface onto a level set of a target's winding field.  The gradient is a dense points x faces sweep like the value, and the
// file has ra_winding.hip's structure: one lane per point, one wave per workgroup, the mesh's own face records walked at a
// wave-uniform address (scalar loads, the next record requested before this one is used, no LDS), winding_grad_tri
// (ra_winding_grad_tri.hpp) all VALU.  The value it returns is ra_mesh_winding's, bit for bit: the same per-pair operations, the same
// chunks, the same order.
//
// Determinism.  A row (value, gx, gy, gz) is a function of (point, mesh) alone.  The faces are summed in stored order in chunks of
// WIND_CHUNK records: four float64 sums per lane start from 0 per chunk, and the chunk sums are added in chunk order, in float64.
// The one-pass kernel does both in a lane; the split launch gives every (point tile, chunk) its own workgroup, which stores the
// chunk's four sums, and a second kernel adds the stored sums in the same chunk order: the same additions in the same order, so the
// same bits.  No atomics.  Each output is scaled by 1 / (4 pi) in float64 and rounded once to fp32.
#include "ra_kernels.hpp"
#include "ra_winding_grad_tri.hpp"

#pragma clang fp contract(off)

namespace {

constexpr double WIND_INV_4PI = 0.07957747154594767;       // 1 / (4 pi)

struct WindSum { double w, x, y, z; };

__device__ __forceinline__ void wind_point(const float* __restrict__ pts, int n, int i, float p[3]) {
    const int k = i < n ? i : 0;       // idle lanes compute along on point 0 and store nothing (n >= 1)
    p[0] = pts[3 * (size_t)k]; p[1] = pts[3 * (size_t)k + 1]; p[2] = pts[3 * (size_t)k + 2];
}

// the float64 sums of chunk c's solid angles and of their gradients, in stored order from 0
__device__ __forceinline__ WindSum wind_grad_chunk(const MeshView& m, int c, const float p[3]) {
    const int n_slots = m.n_leaves * MESH_LEAF;
    const int k0 = c * WIND_CHUNK, k1 = min(n_slots, k0 + WIND_CHUNK);
    const float* rec = m.recs + (size_t)k0 * MESH_REC;
    WindSum s = {0.0, 0.0, 0.0, 0.0};
    if (k0 >= k1) return s;
    float4 r0 = reinterpret_cast<const float4*>(rec)[0], r1 = reinterpret_cast<const float4*>(rec)[1], r2 = reinterpret_cast<const float4*>(rec)[2];
    for (int k = k0; k < k1; ++k) {
        const float a[3] = {r0.x, r0.y, r0.z}, b[3] = {r0.w, r1.x, r1.y}, cc[3] = {r1.z, r1.w, r2.x};
        if (__float_as_int(r2.y) < 0) break;        // kept faces come first in sorted order: nothing behind the first empty slot
        if (k + 1 < k1) {                           // the next record, before this one's thousand cycles of VALU work
            rec += MESH_REC;
            r0 = reinterpret_cast<const float4*>(rec)[0]; r1 = reinterpret_cast<const float4*>(rec)[1]; r2 = reinterpret_cast<const float4*>(rec)[2];
        }
        const WindGrad g = winding_grad_tri(p, a, b, cc);
        s.w += (double)g.omega; s.x += (double)g.gx; s.y += (double)g.gy; s.z += (double)g.gz;
    }
    return s;
}

__device__ __forceinline__ void wind_grad_store(const WindSum& t, int i, float* __restrict__ winding, float* __restrict__ grad) {
    if (winding) winding[i] = (float)(t.w * WIND_INV_4PI);
    grad[3 * (size_t)i] = (float)(t.x * WIND_INV_4PI); grad[3 * (size_t)i + 1] = (float)(t.y * WIND_INV_4PI); grad[3 * (size_t)i + 2] = (float)(t.z * WIND_INV_4PI);
}

__global__ __launch_bounds__(WIND_BLOCK) void winding_grad_kernel(MeshView m, const float* __restrict__ pts, int n, int n_chunks, float* __restrict__ winding,
                                                                  float* __restrict__ grad) {
    const int i = blockIdx.x * WIND_BLOCK + threadIdx.x;
    float p[3];
    wind_point(pts, n, i, p);
    WindSum t = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < n_chunks; ++c) {
        const WindSum s = wind_grad_chunk(m, c, p);
        t.w += s.w; t.x += s.x; t.y += s.y; t.z += s.z;
    }
    if (i < n) wind_grad_store(t, i, winding, grad);
}

// partial: n_chunks x 4 x n float64: chunk-major, then the four sums as planes of n
__global__ __launch_bounds__(WIND_BLOCK) void winding_grad_split_kernel(MeshView m, const float* __restrict__ pts, int n, double* __restrict__ partial) {
    const int i = blockIdx.x * WIND_BLOCK + threadIdx.x, c = blockIdx.y;
    float p[3];
    wind_point(pts, n, i, p);
    const WindSum s = wind_grad_chunk(m, c, p);
    if (i >= n) return;
    double* out = partial + (size_t)c * 4 * n + i;
    out[0] = s.w; out[(size_t)n] = s.x; out[2 * (size_t)n] = s.y; out[3 * (size_t)n] = s.z;
}

__global__ __launch_bounds__(WIND_BLOCK) void winding_grad_combine_kernel(const double* __restrict__ partial, int n, int n_chunks, float* __restrict__ winding,
                                                                          float* __restrict__ grad) {
    const int i = blockIdx.x * WIND_BLOCK + threadIdx.x;
    if (i >= n) return;
    WindSum t = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < n_chunks; ++c) {
        const double* in = partial + (size_t)c * 4 * n + i;
        t.w += in[0]; t.x += in[(size_t)n]; t.y += in[2 * (size_t)n]; t.z += in[3 * (size_t)n];
    }
    wind_grad_store(t, i, winding, grad);
}

}  // namespace

void launch_mesh_winding_grad(const MeshView& m, const float* pts, int n, double* partial, float* winding, float* grad, hipStream_t s) {
    const int tiles = (n + WIND_BLOCK - 1) / WIND_BLOCK, n_chunks = wind_chunk_count(m.n_leaves);
    if (!partial) {
        hipLaunchKernelGGL(winding_grad_kernel, dim3(tiles), dim3(WIND_BLOCK), 0, s, m, pts, n, n_chunks, winding, grad);
        return;
    }
    hipLaunchKernelGGL(winding_grad_split_kernel, dim3(tiles, n_chunks), dim3(WIND_BLOCK), 0, s, m, pts, n, partial);
    hipLaunchKernelGGL(winding_grad_combine_kernel, dim3(tiles), dim3(WIND_BLOCK), 0, s, partial, n, n_chunks, winding, grad);
}

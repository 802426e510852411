// Cloth energies on the device: the Saint-Venant-Kirchhoff membrane, dihedral-angle bending, gravity and the inertia terms of the
// reference's garment model (lib/utils/physx_utils.py), with their gradients with respect to the vertex positions.
//
// Build (once per garment).  A face record of 8 words {v0, v1, v2, rest area, Dm_inv[4]} and, per EDGE of the topology, a hinge record
// of 8 words {a0, a1, a2, b0, b1, b2, flags, area0 + area1}: flags = k0 | k1 << 2 | valid << 4, valid only for an edge of exactly two
// half-edges.  Hinges are addressed by their edge id, so nothing is compacted and nothing is read back; in edge order the valid records
// are the reference's face connectivity.  A vertex's (hinge, slot) list is enumerated from its outgoing half-edges (at most three
// hinges per incident face), written to the segment 3 out_start[v] and sorted there by one thread.
//
// Evaluation.  One lane per (row, face) and per (row, edge) writes its element energy and its corner gradients to scratch; one lane
// per (row, vertex) then adds the face corners in ascending half-edge order and the hinge slots in ascending (hinge, slot) order, each
// term on its own, and the terms in the fixed order (stretch + bending) + gravity.  No float atomics.  An energy is the float64 sum of
// a row's fp32 element energies: CLOTH_CHUNK consecutive elements per workgroup in a fixed tree, then the chunk sums in ascending
// strides.  Chunks never span rows, so a row's outputs depend on that row's positions and the garment alone, bit for bit.
#include "ra_kernels.hpp"
#include "ra_cloth_rules.hpp"

#pragma clang fp contract(off)

namespace {

inline int blocks(long long n, int per) { return (int)((n + per - 1) / per); }

__global__ __launch_bounds__(CLOTH_BLOCK) void cloth_check_fm_kernel(const int* __restrict__ fm, long long n, int n_vm, int* __restrict__ bad) {
    const long long i = (long long)blockIdx.x * CLOTH_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int m = fm[i];
    if (m < 0 || m >= n_vm) atomicOr(bad, 1);
}

__global__ __launch_bounds__(CLOTH_BLOCK) void cloth_face_build_kernel(const int* __restrict__ vert, int n_faces, const float* __restrict__ rest,
                                                                      const float* __restrict__ vm, const int* __restrict__ fm, float* __restrict__ frec,
                                                                      float* __restrict__ f_area, float* __restrict__ dm, float* __restrict__ dm_inv) {
    const int f = blockIdx.x * CLOTH_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int v0 = vert[3 * f], v1 = vert[3 * f + 1], v2 = vert[3 * f + 2];
    const float area = cloth_face_area(rest + 3ll * v0, rest + 3ll * v1, rest + 3ll * v2);
    float d[4], inv[4];
    cloth_dm_inv(vm + 2ll * fm[3 * f], vm + 2ll * fm[3 * f + 1], vm + 2ll * fm[3 * f + 2], d, inv);
    float* r = frec + 8ll * f;
    r[0] = __int_as_float(v0); r[1] = __int_as_float(v1); r[2] = __int_as_float(v2); r[3] = area;
    for (int k = 0; k < 4; ++k) { r[4 + k] = inv[k]; dm[4ll * f + k] = d[k]; dm_inv[4ll * f + k] = inv[k]; }
    f_area[f] = area;
}

// per edge: the hinge record, and the exposed face pair / edge vertices (-1 where the edge is no hinge)
__global__ __launch_bounds__(CLOTH_BLOCK) void cloth_hinge_build_kernel(TopoView t, const float* __restrict__ f_area, int* __restrict__ hrec,
                                                                       int* __restrict__ h_faces, int* __restrict__ h_verts) {
    const int e = blockIdx.x * CLOTH_BLOCK + threadIdx.x;
    if (e >= t.n_edges) return;
    int* r = hrec + 8ll * e;
    if (t.counts[e] != 2) {
        for (int k = 0; k < 8; ++k) r[k] = 0;
        h_faces[2 * e] = h_faces[2 * e + 1] = h_verts[2 * e] = h_verts[2 * e + 1] = -1;
        return;
    }
    const int h0 = t.ehe[t.ehe_start[e]], h1 = t.ehe[t.ehe_start[e] + 1];
    const int f0 = h0 / 3, f1 = h1 / 3, k0 = h0 - 3 * f0, k1 = h1 - 3 * f1;
    for (int k = 0; k < 3; ++k) { r[k] = t.vert[3 * f0 + k]; r[3 + k] = t.vert[3 * f1 + k]; }
    r[6] = k0 | (k1 << 2) | 16;
    r[7] = __float_as_int(f_area[f0] + f_area[f1]);
    h_faces[2 * e] = f0; h_faces[2 * e + 1] = f1;
    h_verts[2 * e] = t.vert[h0]; h_verts[2 * e + 1] = t.vert[h1];
}

// per vertex: the mass (its faces' shares in ascending outgoing-half-edge order) and the sorted (hinge, slot) list
__global__ __launch_bounds__(CLOTH_BLOCK) void cloth_vert_build_kernel(TopoView t, const float* __restrict__ f_area, float density, float* __restrict__ mass,
                                                                      float* __restrict__ inv_mass, int* __restrict__ vh, int* __restrict__ vh_count) {
    const int v = blockIdx.x * CLOTH_BLOCK + threadIdx.x;
    if (v >= t.n_verts) return;
    float m = 0.0f;
    int* list = vh + 3ll * t.out_start[v];
    int n = 0;
    for (int k = t.out_start[v]; k < t.out_start[v + 1]; ++k) {
        const int he = t.out_he[k], f = he / 3, corner = he - 3 * f;
        m = m + cloth_mass_share(density, f_area[f]);
        for (int j = 0; j < 3; ++j) {
            const int e = t.edge[3 * f + j];
            if (t.counts[e] != 2) continue;
            const int side = t.ehe[t.ehe_start[e]] == 3 * f + j ? 0 : 1;
            const int key = 6 * e + 3 * side + corner;
            int p = n++;                                    // insertion: the list stays ascending
            while (p > 0 && list[p - 1] > key) { list[p] = list[p - 1]; --p; }
            list[p] = key;
        }
    }
    mass[v] = m;
    inv_mass[v] = 1.0f / m;
    vh_count[v] = n;
}

__global__ __launch_bounds__(CLOTH_BLOCK) void cloth_face_kernel(ClothJob j) {
    const long long idx = (long long)blockIdx.x * CLOTH_BLOCK + threadIdx.x;
    if (idx >= (long long)j.B * j.n_faces) return;
    const int b = (int)(idx / j.n_faces), f = (int)(idx - (long long)b * j.n_faces);
    const float4* rec = reinterpret_cast<const float4*>(j.frec) + 2ll * f;
    const float4 r0 = rec[0], r1 = rec[1];
    const float* x = j.x + 3ll * b * j.n_verts;
    const float m[4] = {r1.x, r1.y, r1.z, r1.w};
    float g[9];
    const float e = cloth_stretch(x + 3ll * __float_as_int(r0.x), x + 3ll * __float_as_int(r0.y), x + 3ll * __float_as_int(r0.z), m, r0.w, j.thickness, j.mu,
                                  j.lambda, j.grad ? g : (float*)nullptr);
    j.e_face[idx] = e;
    if (j.grad) {
        float* o = j.g_face + 9 * idx;
        for (int k = 0; k < 9; ++k) o[k] = g[k];
    }
}

__global__ __launch_bounds__(CLOTH_BLOCK) void cloth_hinge_kernel(ClothJob j) {
    const long long idx = (long long)blockIdx.x * CLOTH_BLOCK + threadIdx.x;
    if (idx >= (long long)j.B * j.n_edges) return;
    const int b = (int)(idx / j.n_edges), e = (int)(idx - (long long)b * j.n_edges);
    const int4* rec = reinterpret_cast<const int4*>(j.hrec) + 2ll * e;
    const int4 r0 = rec[0], r1 = rec[1];
    if (!(r1.z & 16)) {                                     // no hinge on this edge: nothing reads its gradient slots
        j.e_hinge[idx] = 0.0f;
        return;
    }
    const float* x = j.x + 3ll * b * j.n_verts;
    const float* a[3] = {x + 3ll * r0.x, x + 3ll * r0.y, x + 3ll * r0.z};
    const float* c[3] = {x + 3ll * r0.w, x + 3ll * r1.x, x + 3ll * r1.y};
    const int k0 = r1.z & 3, k1 = (r1.z >> 2) & 3;
    if (j.grad) {
        float g[18];
        j.e_hinge[idx] = cloth_bending<true>(a, c, k0, k1, __int_as_float(r1.w), j.bending, g);
        float* o = j.g_hinge + 18 * idx;
#pragma unroll
        for (int k = 0; k < 18; ++k) o[k] = g[k];
    } else {
        j.e_hinge[idx] = cloth_bending<false>(a, c, k0, k1, __int_as_float(r1.w), j.bending, (float*)nullptr);
    }
}

__global__ __launch_bounds__(CLOTH_BLOCK) void cloth_gravity_kernel(ClothJob j) {
    const long long idx = (long long)blockIdx.x * CLOTH_BLOCK + threadIdx.x;
    if (idx >= (long long)j.B * j.n_verts) return;
    const int v = (int)(idx % j.n_verts);
    j.e_vert[idx] = cloth_gravity(j.gravity, j.mass[v], j.x[3 * idx + 1]);
}

__global__ __launch_bounds__(CLOTH_BLOCK) void cloth_vertex_kernel(ClothJob j, TopoView t) {
    const long long idx = (long long)blockIdx.x * CLOTH_BLOCK + threadIdx.x;
    if (idx >= (long long)j.B * j.n_verts) return;
    const int b = (int)(idx / j.n_verts), v = (int)(idx - (long long)b * j.n_verts);
    float gs[3] = {0.0f, 0.0f, 0.0f}, gb[3] = {0.0f, 0.0f, 0.0f}, gg[3] = {0.0f, 0.0f, 0.0f};
    if (j.terms & RA_CLOTH_STRETCH) {
        const float* base = j.g_face + 9ll * b * j.n_faces;
        for (int k = t.out_start[v]; k < t.out_start[v + 1]; ++k) {
            const float* g = base + 3ll * t.out_he[k];      // (face, corner) = the half-edge
            for (int c = 0; c < 3; ++c) gs[c] = gs[c] + g[c];
        }
    }
    if (j.terms & RA_CLOTH_BENDING) {
        const float* base = j.g_hinge + 18ll * b * j.n_edges;
        const int* list = j.vh + 3ll * t.out_start[v];
        const int n = j.vh_count[v];
        for (int k = 0; k < n; ++k) {
            const float* g = base + 3ll * list[k];
            for (int c = 0; c < 3; ++c) gb[c] = gb[c] + g[c];
        }
    }
    if (j.terms & RA_CLOTH_GRAVITY) gg[1] = j.gravity * j.mass[v];
    for (int c = 0; c < 3; ++c) {
        const float sb = gs[c] + gb[c];
        j.grad[3 * idx + c] = sb + gg[c];
    }
}

// float64 sums of fp32 elements: grid (chunks, rows); a chunk is CLOTH_CHUNK consecutive elements of ONE row
__global__ __launch_bounds__(CLOTH_BLOCK) void cloth_chunk_sum_kernel(const float* __restrict__ el, int n, int n_chunks, double* __restrict__ part) {
    __shared__ double sh[CLOTH_BLOCK];
    const int t = threadIdx.x, row = blockIdx.y;
    const long long lo = (long long)blockIdx.x * CLOTH_CHUNK;
    double s = 0.0;
    for (int k = t; k < CLOTH_CHUNK; k += CLOTH_BLOCK) {
        const long long i = lo + k;
        if (i < n) s = s + (double)el[(long long)row * n + i];
    }
    sh[t] = s;
    __syncthreads();
    for (int w = CLOTH_BLOCK / 2; w > 0; w >>= 1) {
        if (t < w) sh[t] = sh[t] + sh[t + w];
        __syncthreads();
    }
    if (t == 0) part[(long long)row * n_chunks + blockIdx.x] = sh[0];
}

// one workgroup per row: thread t adds the chunk sums t, t + CLOTH_BLOCK, ... ascending, then the tree; out[row * stride]
__global__ __launch_bounds__(CLOTH_BLOCK) void cloth_row_sum_kernel(const double* __restrict__ part, int n_chunks, double* __restrict__ out, int stride) {
    __shared__ double sh[CLOTH_BLOCK];
    const int t = threadIdx.x, row = blockIdx.x;
    double s = 0.0;
    for (int k = t; k < n_chunks; k += CLOTH_BLOCK) s = s + part[(long long)row * n_chunks + k];
    sh[t] = s;
    __syncthreads();
    for (int w = CLOTH_BLOCK / 2; w > 0; w >>= 1) {
        if (t < w) sh[t] = sh[t] + sh[t + w];
        __syncthreads();
    }
    if (t == 0) out[(long long)row * stride] = sh[0];
}

__global__ __launch_bounds__(CLOTH_BLOCK) void cloth_inertia_kernel(InertiaJob j) {
    const long long idx = (long long)blockIdx.x * CLOTH_BLOCK + threadIdx.x;
    if (idx >= (long long)j.rows * j.V) return;
    const int v = (int)(idx % j.V);
    float g[3];
    const bool want = j.g_next || j.g_curr || j.g_vel;
    const float val = cloth_inertia(j.x_next + 3 * idx, j.x_curr + 3 * idx, j.v_curr + 3 * idx, j.mass[v], j.dt, j.has_accel ? j.accel : (const float*)nullptr,
                                    want ? g : (float*)nullptr);
    j.el[idx] = val;
    for (int c = 0; c < 3 && want; ++c) {
        if (j.g_next) j.g_next[3 * idx + c] = g[c];
        if (j.g_curr) j.g_curr[3 * idx + c] = -g[c];
        if (j.g_vel) j.g_vel[3 * idx + c] = -(j.dt * g[c]);
    }
}

void row_sums(const float* el, int rows, int n, double* part, double* out, int stride, hipStream_t s) {
    const int n_chunks = blocks(n, CLOTH_CHUNK);
    hipLaunchKernelGGL(cloth_chunk_sum_kernel, dim3(n_chunks, rows), dim3(CLOTH_BLOCK), 0, s, el, n, n_chunks, part);
    hipLaunchKernelGGL(cloth_row_sum_kernel, dim3(rows), dim3(CLOTH_BLOCK), 0, s, (const double*)part, n_chunks, out, stride);
}

}  // namespace

void launch_cloth_check_fm(const int* fm, int n_faces, int n_vm, int* bad, hipStream_t s) {
    const long long n = 3ll * n_faces;
    hipLaunchKernelGGL(cloth_check_fm_kernel, dim3(blocks(n, CLOTH_BLOCK)), dim3(CLOTH_BLOCK), 0, s, fm, n, n_vm, bad);
}

// n_verts >= 1; a topology without faces gives a garment of massless vertices
void launch_cloth_build(const TopoView& t, const ClothBuild& b, hipStream_t s) {
    if (t.n_faces > 0)
        hipLaunchKernelGGL(cloth_face_build_kernel, dim3(blocks(t.n_faces, CLOTH_BLOCK)), dim3(CLOTH_BLOCK), 0, s, t.vert, t.n_faces, b.rest, b.vm, b.fm, b.frec,
                           b.f_area, b.dm, b.dm_inv);
    if (t.n_edges > 0)
        hipLaunchKernelGGL(cloth_hinge_build_kernel, dim3(blocks(t.n_edges, CLOTH_BLOCK)), dim3(CLOTH_BLOCK), 0, s, t, (const float*)b.f_area, b.hrec, b.h_faces,
                           b.h_verts);
    hipLaunchKernelGGL(cloth_vert_build_kernel, dim3(blocks(t.n_verts, CLOTH_BLOCK)), dim3(CLOTH_BLOCK), 0, s, t, (const float*)b.f_area, b.density, b.mass,
                       b.inv_mass, b.vh, b.vh_count);
}

// energy: B x 3 doubles, zero on entry (a term that is not selected, or has no element, stays 0)
void launch_cloth_energy(const TopoView& t, const ClothJob& j, double* energy, hipStream_t s) {
    const dim3 block(CLOTH_BLOCK);
    if ((j.terms & RA_CLOTH_STRETCH) && j.n_faces > 0) {
        hipLaunchKernelGGL(cloth_face_kernel, dim3(blocks((long long)j.B * j.n_faces, CLOTH_BLOCK)), block, 0, s, j);
        row_sums(j.e_face, j.B, j.n_faces, j.part, energy + 0, 3, s);
    }
    if ((j.terms & RA_CLOTH_BENDING) && j.n_edges > 0) {
        hipLaunchKernelGGL(cloth_hinge_kernel, dim3(blocks((long long)j.B * j.n_edges, CLOTH_BLOCK)), block, 0, s, j);
        row_sums(j.e_hinge, j.B, j.n_edges, j.part, energy + 1, 3, s);
    }
    if ((j.terms & RA_CLOTH_GRAVITY) && j.n_verts > 0) {
        hipLaunchKernelGGL(cloth_gravity_kernel, dim3(blocks((long long)j.B * j.n_verts, CLOTH_BLOCK)), block, 0, s, j);
        row_sums(j.e_vert, j.B, j.n_verts, j.part, energy + 2, 3, s);
    }
    if (j.grad && j.n_verts > 0)
        hipLaunchKernelGGL(cloth_vertex_kernel, dim3(blocks((long long)j.B * j.n_verts, CLOTH_BLOCK)), block, 0, s, j, t);
}

// rows, V >= 1
void launch_cloth_inertia(const InertiaJob& j, double* value, hipStream_t s) {
    hipLaunchKernelGGL(cloth_inertia_kernel, dim3(blocks((long long)j.rows * j.V, CLOTH_BLOCK)), dim3(CLOTH_BLOCK), 0, s, j);
    row_sums(j.el, j.rows, j.V, j.part, value, 1, s);
}

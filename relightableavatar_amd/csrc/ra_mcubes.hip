// Iso-surface extraction on the device (ra_marching_cubes) and the largest edge-connected component of a triangle mesh
// (ra_mesh_largest_component): the two steps of the reference's mesh renderer that it leaves to mcubes and trimesh
// (lib/networks/renderer/mesh_renderer.py:74-84).
//
// Marching cubes.  One thread per grid point p = (x * ny + y) * nz + z.  A point owns the three grid edges that leave it towards +x, +y,
// +z and the cell whose minimum corner it is, so every sign-changing edge carries exactly one vertex and the output order is a function
// of the volume alone: vertices by (p, axis), faces by (p, order in the table).  Three passes: classify (a 3-bit mask of the owned
// crossed edges, the vertex and triangle counts packed into one 64-bit word), ONE exclusive sum over the packed words (the low half
// counts vertices, the high half triangles: neither total reaches 2^31, so no carry crosses), emit.  No atomic decides an index.
// A corner is below when v < iso: a NaN is not below.  A vertex is x + t along its edge, t = (iso - a) / (b - a) with a the value at the
// owning point, every step a named fp32 operation so that a host restatement gives the same bits.
//
// Largest component.  Faces that share an undirected edge are connected.  The 3F edges are sorted by key (lo << 32 | hi); equal keys
// are consecutive, and every edge links its face to the faces of its two neighbours in sorted order (a chain through all faces of an
// edge, however many).  Labels start as the face index and fall to the minimum of the component: a pass takes the minimum over a
// face's links, follows it twice more (label of the label) and lowers the face and its former label with integer atomicMin.
// LCC_PASSES passes are queued at once and those behind the fixed point exit at their first instruction.  Labels only
// fall and stay inside the component, so the fixed point — every face holds the lowest face index of its component — does not depend
// on the order the hardware runs the passes in.  A component's size is the number of distinct vertices its faces refer to (a second
// sort, of (label << 32 | vertex) keys, and integer counting); the winner is the maximum of (size << 32 | ~label): the most vertices,
// then the lowest face index.
#include "ra_mcubes.hpp"
#include "ra_mcubes_tables.hpp"
#include <hipcub/hipcub.hpp>

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

inline int blocks(long long n) { return (int)((n + MC_BLOCK - 1) / MC_BLOCK); }

// ------------------------------------------------------------------ the scalar volume: filter, compaction, scatter
// One thread per grid point p = (x * ny + y) * nz + z, the point built from the three axes (the caller's aranges: nothing here re-derives
// their rounding).  The K nearest vertices are found by an exhaustive scan — every workgroup stages the vertices through LDS in tiles
// of VOL_TILE and every thread keeps its K smallest squared distances in ascending order — so they are exact by construction:
// d2 = (dx^2 + dy^2) + dz^2 in named fp32 steps, the same sums in the same order as the oracle's.  The frame's box structure answers
// the same question faster for K = 3; extraction is offline and 5.6 M points x 6890 vertices are 4e10 distances.
// Kept: t = sum_k wn_k d_k < dist_th with d_k = sqrt(d2_k), w_k = 1 / (d_k + 1e-8), wn_k = w_k / sum w: sample_blend_K_closest_points with
// values = None (sample_utils.py:605-611, 631-641), which is what mesh_renderer.py:44-46 filters with.
__global__ __launch_bounds__(VOL_TILE) void vol_filter_kernel(VolJob j) {
    __shared__ float sv[VOL_TILE * 3];
    const int n = j.nx * j.ny * j.nz;
    const int p = blockIdx.x * VOL_TILE + threadIdx.x;
    const bool in = p < n;
    const int pp = in ? p : 0;
    const float qx = j.xs[pp / (j.nz * j.ny)], qy = j.ys[(pp / j.nz) % j.ny], qz = j.zs[pp % j.nz];
    const float inf = __builtin_huge_valf();
    float b0 = inf, b1 = inf, b2 = inf, b3 = inf;      // ascending
    for (int v0 = 0; v0 < j.n_verts; v0 += VOL_TILE) {
        const int nv = min(VOL_TILE, j.n_verts - v0);
        __syncthreads();
        for (int k = threadIdx.x; k < nv * 3; k += VOL_TILE) sv[k] = j.verts[3 * (size_t)v0 + k];
        __syncthreads();
        for (int k = 0; k < nv; ++k) {
            const float dx = __fsub_rn(qx, sv[3 * k]), dy = __fsub_rn(qy, sv[3 * k + 1]), dz = __fsub_rn(qz, sv[3 * k + 2]);
            const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            if (d < b3) {           // insertion into four sorted slots; NaN distances never enter
                if (d < b0) { b3 = b2; b2 = b1; b1 = b0; b0 = d; }
                else if (d < b1) { b3 = b2; b2 = b1; b1 = d; }
                else if (d < b2) { b3 = b2; b2 = d; }
                else b3 = d;
            }
        }
    }
    if (!in) return;
    const float b[VOL_MAX_K] = {b0, b1, b2, b3};
    float d[VOL_MAX_K], w[VOL_MAX_K], sum = 0.f;
#pragma unroll
    for (int k = 0; k < VOL_MAX_K; ++k) {
        d[k] = k < j.K ? __fsqrt_rn(b[k]) : 0.f;
        w[k] = k < j.K ? __fdiv_rn(1.f, __fadd_rn(d[k], 1e-8f)) : 0.f;
        if (k < j.K) sum = __fadd_rn(sum, w[k]);
    }
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < VOL_MAX_K; ++k)
        if (k < j.K) t = __fadd_rn(t, __fmul_rn(__fdiv_rn(w[k], sum), d[k]));
    j.flag[p] = t < j.dist_th ? 1 : 0;
    if (p == 0) j.flag[n] = 0;
}

__global__ __launch_bounds__(MC_BLOCK) void vol_compact_kernel(VolJob j, float* __restrict__ pts, int* __restrict__ cell) {
    const int n = j.nx * j.ny * j.nz;
    const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (p >= n || !j.flag[p]) return;
    const int x = p / (j.nz * j.ny), y = (p / j.nz) % j.ny, z = p % j.nz, i = j.off[p];
    pts[3 * (size_t)i] = j.xs[x]; pts[3 * (size_t)i + 1] = j.ys[y]; pts[3 * (size_t)i + 2] = j.zs[z];
    cell[i] = ((x + j.pad) * (j.ny + 2 * j.pad) + (y + j.pad)) * (j.nz + 2 * j.pad) + (z + j.pad);
}

__global__ __launch_bounds__(MC_BLOCK) void vol_fill_kernel(float* __restrict__ volume, long long n, float fill) {
    const long long i = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i < n) volume[i] = fill;
}

// the volume holds -sdf; count: the kept points on the device, cap: the host's copy of it (the arrays' size)
__global__ __launch_bounds__(MC_BLOCK) void vol_scatter_kernel(const float* __restrict__ sdf, const int* __restrict__ cell, const int* __restrict__ count,
                                                               int cap, float* __restrict__ volume) {
    const int i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i < cap && i < *count) volume[cell[i]] = -sdf[i];
}

// ------------------------------------------------------------------ marching cubes
__global__ __launch_bounds__(MC_BLOCK) void mc_classify_kernel(const float* __restrict__ vol, int nx, int ny, int nz, float iso, u64* __restrict__ cnt,
                                                               unsigned char* __restrict__ mask) {
    const int n = nx * ny * nz;
    const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (p > n) return;
    if (p == n) { cnt[n] = 0ull; return; }       // the slot whose exclusive sum is the totals
    const int z = p % nz, y = (p / nz) % ny, x = p / (nz * ny);
    const int sx = ny * nz, sy = nz;
    const bool hx = x + 1 < nx, hy = y + 1 < ny, hz = z + 1 < nz;
    const bool b0 = vol[p] < iso;
    const bool bx = hx && (vol[p + sx] < iso), by = hy && (vol[p + sy] < iso), bz = hz && (vol[p + 1] < iso);
    const unsigned m = (hx && bx != b0 ? 1u : 0u) | (hy && by != b0 ? 2u : 0u) | (hz && bz != b0 ? 4u : 0u);
    unsigned ntri = 0;
    if (hx && hy && hz) {
        // corners 0..7 of the classic numbering: (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1)
        const unsigned ci = (b0 ? 1u : 0u) | (bx ? 2u : 0u) | (vol[p + sx + sy] < iso ? 4u : 0u) | (by ? 8u : 0u) | (bz ? 16u : 0u) |
                            (vol[p + sx + 1] < iso ? 32u : 0u) | (vol[p + sx + sy + 1] < iso ? 64u : 0u) | (vol[p + sy + 1] < iso ? 128u : 0u);
        ntri = MC_NTRI[ci];
    }
    mask[p] = (unsigned char)m;
    cnt[p] = (u64)__popc(m) | ((u64)ntri << 32);
}

// the one place a vertex coordinate is computed
__device__ __forceinline__ float mc_interp(float base, float a, float b, float iso) {
    return __fadd_rn(base, __fdiv_rn(__fsub_rn(iso, a), __fsub_rn(b, a)));
}

// writes are bounded by the counts the caller allocated for (those of the classify pass): a volume that changed between the two passes
// gives a wrong mesh, never a write outside the arrays
__global__ __launch_bounds__(MC_BLOCK) void mc_emit_kernel(const float* __restrict__ vol, int nx, int ny, int nz, float iso, const u64* __restrict__ off,
                                                           const unsigned char* __restrict__ mask, float* __restrict__ verts, int n_verts,
                                                           int* __restrict__ faces, int n_faces) {
    const int n = nx * ny * nz;
    const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int z = p % nz, y = (p / nz) % ny, x = p / (nz * ny);
    const int sx = ny * nz, sy = nz;
    const u64 o = off[p];
    const unsigned m = mask[p];
    const float a = vol[p];
    if (m) {
        unsigned vi = (unsigned)o;
        const float fx = (float)x, fy = (float)y, fz = (float)z;
        if ((m & 1u) && vi < (unsigned)n_verts) { float* v = verts + 3 * (size_t)vi; v[0] = mc_interp(fx, a, vol[p + sx], iso); v[1] = fy; v[2] = fz; }
        vi += m & 1u;
        if ((m & 2u) && vi < (unsigned)n_verts) { float* v = verts + 3 * (size_t)vi; v[0] = fx; v[1] = mc_interp(fy, a, vol[p + sy], iso); v[2] = fz; }
        vi += (m >> 1) & 1u;
        if ((m & 4u) && vi < (unsigned)n_verts) { float* v = verts + 3 * (size_t)vi; v[0] = fx; v[1] = fy; v[2] = mc_interp(fz, a, vol[p + 1], iso); }
    }
    if (!(x + 1 < nx && y + 1 < ny && z + 1 < nz)) return;
    const unsigned ci = (a < iso ? 1u : 0u) | (vol[p + sx] < iso ? 2u : 0u) | (vol[p + sx + sy] < iso ? 4u : 0u) | (vol[p + sy] < iso ? 8u : 0u) |
                        (vol[p + 1] < iso ? 16u : 0u) | (vol[p + sx + 1] < iso ? 32u : 0u) | (vol[p + sx + sy + 1] < iso ? 64u : 0u) |
                        (vol[p + sy + 1] < iso ? 128u : 0u);
    const unsigned ntri = MC_NTRI[ci];
    const unsigned fbase = (unsigned)(o >> 32);
    for (unsigned t = 0; t < ntri; ++t) {
        if (fbase + t >= (unsigned)n_faces) return;
        int* f = faces + 3 * (size_t)(fbase + t);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const unsigned e = MC_TRI[ci * (3 * MC_MAX_TRI) + 3 * t + j];
            const unsigned own = MC_EDGE_OWNER[e], axis = MC_EDGE_AXIS[e];
            const int q = p + (own & 1u ? sx : 0) + (own & 2u ? sy : 0) + (own & 4u ? 1 : 0);      // inside the cell: a valid grid point
            f[j] = (int)((unsigned)off[q] + __popc((unsigned)mask[q] & ((1u << axis) - 1u)));
        }
    }
}

// ------------------------------------------------------------------ largest component
__global__ __launch_bounds__(MC_BLOCK) void lcc_edges_kernel(const int* __restrict__ faces, int n_faces, int n_verts, u64* __restrict__ keys,
                                                             int* __restrict__ slots, int* __restrict__ label, int* __restrict__ stat) {
    const int f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    int v[3];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) { v[j] = faces[3 * (size_t)f + j]; ok = ok && v[j] >= 0 && v[j] < n_verts; }
    if (!ok) { atomicAdd(stat + LCC_BAD, 1); v[0] = v[1] = v[2] = 0; }      // the call fails after the read-back; until then the face is harmless
    label[f] = f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const unsigned a = (unsigned)v[j], b = (unsigned)v[(j + 1) % 3];
        keys[3 * (size_t)f + j] = ((u64)min(a, b) << 32) | (u64)max(a, b);
        slots[3 * (size_t)f + j] = 3 * f + j;
    }
}

// link[2 * slot + {0, 1}]: the faces of the previous / next equal key in sorted order, -1 without one
__global__ __launch_bounds__(MC_BLOCK) void lcc_link_kernel(const u64* __restrict__ keys_sorted, const int* __restrict__ slots_sorted, int n, int* __restrict__ link) {
    const int i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64 k = keys_sorted[i];
    const int s = slots_sorted[i];
    link[2 * (size_t)s] = (i > 0 && keys_sorted[i - 1] == k) ? slots_sorted[i - 1] / 3 : -1;
    link[2 * (size_t)s + 1] = (i + 1 < n && keys_sorted[i + 1] == k) ? slots_sorted[i + 1] / 3 : -1;
}

// Pass k of a batch.  The host queues LCC_PASSES of them and looks once: a pass behind one that lowered nothing (its flag is still 0) has
// nothing to do and exits, so the batch costs the passes the mesh needs plus empty launches, and no host round trip in between.
// label is read with plain loads while other threads lower it with atomicMin (hence no __restrict__ on it): a stale read only sees a
// HIGHER label than the current one, which delays the fixed point by a pass and never changes it — labels only fall, and every value
// ever stored is a face of the same component.  The flag is a plain store of the same 1 by every writer.
__global__ __launch_bounds__(MC_BLOCK) void lcc_pass_kernel(const int* __restrict__ link, int n_faces, int* label, int* __restrict__ stat, int k) {
    if (k > 0 && stat[LCC_FLAGS + k - 1] == 0) return;
    const int f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int old = label[f];
    int m = old;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const int g = link[6 * (size_t)f + c];
        if (g >= 0) m = min(m, label[g]);
    }
    m = min(m, label[m]);
    m = min(m, label[m]);               // followed twice: chains of labels halve faster than the mesh's diameter grows
    if (m < old) {
        atomicMin(label + f, m);
        atomicMin(label + old, m);      // old is a face of the same component: its whole following comes along
        stat[LCC_FLAGS + k] = 1;
    }
}

// (label << 32 | vertex) per face corner: sorted, the first of every run of equal keys is one distinct vertex of that component.
// At the fixed point every label is its component's lowest face; before it the sizes are provisional and the host asks again
__global__ __launch_bounds__(MC_BLOCK) void lcc_vkeys_kernel(const int* __restrict__ faces, const int* __restrict__ label, int n_faces, int n_verts,
                                                             u64* __restrict__ keys) {
    const int f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const u64 l = (u64)(unsigned)label[f] << 32;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int v = faces[3 * (size_t)f + j];
        keys[3 * (size_t)f + j] = l | (u64)(unsigned)((v >= 0 && v < n_verts) ? v : 0);
    }
}

__global__ __launch_bounds__(MC_BLOCK) void lcc_sizes_kernel(const u64* __restrict__ keys_sorted, int n, int* __restrict__ size) {
    const int i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64 k = keys_sorted[i];
    if (i == 0 || keys_sorted[i - 1] != k) atomicAdd(size + (int)(k >> 32), 1);
}

__global__ __launch_bounds__(MC_BLOCK) void lcc_best_kernel(const int* __restrict__ label, const int* __restrict__ size, int n_faces, int* __restrict__ stat) {
    const int f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= n_faces || label[f] != f) return;
    atomicMax(reinterpret_cast<u64*>(stat + LCC_BEST), ((u64)(unsigned)size[f] << 32) | (u64)(~(unsigned)f));
}

// keep flags: kf[f] for the faces of the winner, kv[v] for the vertices they refer to (every writer stores the same 1); slot n of each: 0
__global__ __launch_bounds__(MC_BLOCK) void lcc_mark_kernel(const int* __restrict__ faces, const int* __restrict__ label, int n_faces, int n_verts,
                                                            const int* __restrict__ stat, int* __restrict__ kf, int* __restrict__ kv) {
    const int f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int best = (int)~(unsigned)(*reinterpret_cast<const u64*>(stat + LCC_BEST));
    const bool keep = label[f] == best;
    kf[f] = keep ? 1 : 0;
    if (!keep) return;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int v = faces[3 * (size_t)f + j];
        if (v >= 0 && v < n_verts) kv[v] = 1;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void lcc_gather_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int n_verts, int n_faces,
                                                              const int* __restrict__ kf, const int* __restrict__ of, const int* __restrict__ kv,
                                                              const int* __restrict__ ov, float* __restrict__ out_verts, int cap_verts,
                                                              int* __restrict__ out_faces, int cap_faces) {
    const int i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i < n_verts && kv[i] && ov[i] < cap_verts) {
        float* o = out_verts + 3 * (size_t)ov[i];
        o[0] = verts[3 * (size_t)i]; o[1] = verts[3 * (size_t)i + 1]; o[2] = verts[3 * (size_t)i + 2];
    }
    if (i < n_faces && kf[i] && of[i] < cap_faces) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int v = faces[3 * (size_t)i + j];      // in range when the size query ran (it fails otherwise); checked again: the array is the caller's
            out_faces[3 * (size_t)of[i] + j] = (v >= 0 && v < n_verts) ? ov[v] : 0;
        }
    }
}

}  // namespace

size_t mc_scan_temp_bytes(int n) {
    size_t a = 0, b = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, a, (const u64*)nullptr, (u64*)nullptr, n);
    hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const int*)nullptr, (int*)nullptr, n);
    return a > b ? a : b;
}

size_t lcc_sort_temp_bytes(int n) {
    size_t a = 0, b = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const u64*)nullptr, (u64*)nullptr, (const int*)nullptr, (int*)nullptr, n, 0, 64);
    hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const u64*)nullptr, (u64*)nullptr, n, 0, 64);
    return a > b ? a : b;
}

int launch_vol_filter(const VolJob& j, hipStream_t s) {
    const int n = j.nx * j.ny * j.nz;
    hipLaunchKernelGGL(vol_filter_kernel, dim3((n + VOL_TILE - 1) / VOL_TILE), dim3(VOL_TILE), 0, s, j);
    size_t tb = j.temp_bytes;
    return hipcub::DeviceScan::ExclusiveSum(j.temp, tb, j.flag, j.off, n + 1, s) == hipSuccess ? 0 : 1;
}

void launch_vol_compact(const VolJob& j, float* pts, int* cell, hipStream_t s) {
    hipLaunchKernelGGL(vol_compact_kernel, dim3(blocks(j.nx * j.ny * j.nz)), dim3(MC_BLOCK), 0, s, j, pts, cell);
}

void launch_vol_fill(float* volume, long long n, float fill, hipStream_t s) {
    hipLaunchKernelGGL(vol_fill_kernel, dim3(blocks(n)), dim3(MC_BLOCK), 0, s, volume, n, fill);
}

void launch_vol_scatter(const float* sdf, const int* cell, const int* count, int cap, float* volume, hipStream_t s) {
    if (cap > 0) hipLaunchKernelGGL(vol_scatter_kernel, dim3(blocks(cap)), dim3(MC_BLOCK), 0, s, sdf, cell, count, cap, volume);
}

int launch_mc_count(const McJob& j, hipStream_t s) {
    const int n = j.nx * j.ny * j.nz;
    hipLaunchKernelGGL(mc_classify_kernel, dim3(blocks((long long)n + 1)), dim3(MC_BLOCK), 0, s, j.vol, j.nx, j.ny, j.nz, j.iso, j.cnt, j.mask);
    size_t tb = j.temp_bytes;
    return hipcub::DeviceScan::ExclusiveSum(j.temp, tb, j.cnt, j.off, n + 1, s) == hipSuccess ? 0 : 1;
}

void launch_mc_emit(const McJob& j, float* verts, int n_verts, int* faces, int n_faces, hipStream_t s) {
    const int n = j.nx * j.ny * j.nz;
    hipLaunchKernelGGL(mc_emit_kernel, dim3(blocks(n)), dim3(MC_BLOCK), 0, s, j.vol, j.nx, j.ny, j.nz, j.iso, j.off, j.mask, verts, n_verts, faces, n_faces);
}

int launch_lcc_links(const LccJob& j, hipStream_t s) {
    const int n3 = 3 * j.n_faces;
    hipLaunchKernelGGL(lcc_edges_kernel, dim3(blocks(j.n_faces)), dim3(MC_BLOCK), 0, s, j.faces, j.n_faces, j.n_verts, j.keys, j.slots, j.label, j.stat);
    size_t tb = j.temp_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(j.temp, tb, j.keys, j.keys_sorted, j.slots, j.slots_sorted, n3, 0, 64, s) != hipSuccess) return 1;
    hipLaunchKernelGGL(lcc_link_kernel, dim3(blocks(n3)), dim3(MC_BLOCK), 0, s, j.keys_sorted, j.slots_sorted, n3, j.link);
    return 0;
}

void launch_lcc_passes(const LccJob& j, hipStream_t s) {
    for (int k = 0; k < LCC_PASSES; ++k)
        hipLaunchKernelGGL(lcc_pass_kernel, dim3(blocks(j.n_faces)), dim3(MC_BLOCK), 0, s, j.link, j.n_faces, j.label, j.stat, k);
}

// from the labels to the keep flags and their exclusive sums; kf / of hold n_faces + 1 ints, kv / ov n_verts + 1, all but of / ov zeroed by the caller
int launch_lcc_select(const LccJob& j, hipStream_t s) {
    const int n3 = 3 * j.n_faces;
    hipLaunchKernelGGL(lcc_vkeys_kernel, dim3(blocks(j.n_faces)), dim3(MC_BLOCK), 0, s, j.faces, j.label, j.n_faces, j.n_verts, j.keys);
    size_t tb = j.temp_bytes;
    if (hipcub::DeviceRadixSort::SortKeys(j.temp, tb, j.keys, j.keys_sorted, n3, 0, 64, s) != hipSuccess) return 1;
    hipLaunchKernelGGL(lcc_sizes_kernel, dim3(blocks(n3)), dim3(MC_BLOCK), 0, s, j.keys_sorted, n3, j.size);
    hipLaunchKernelGGL(lcc_best_kernel, dim3(blocks(j.n_faces)), dim3(MC_BLOCK), 0, s, j.label, j.size, j.n_faces, j.stat);
    hipLaunchKernelGGL(lcc_mark_kernel, dim3(blocks(j.n_faces)), dim3(MC_BLOCK), 0, s, j.faces, j.label, j.n_faces, j.n_verts, j.stat, j.kf, j.kv);
    tb = j.temp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(j.temp, tb, j.kf, j.of, j.n_faces + 1, s) != hipSuccess) return 1;
    tb = j.temp_bytes;
    return hipcub::DeviceScan::ExclusiveSum(j.temp, tb, j.kv, j.ov, j.n_verts + 1, s) == hipSuccess ? 0 : 1;
}

void launch_lcc_gather(const LccJob& j, const float* verts, float* out_verts, int cap_verts, int* out_faces, int cap_faces, hipStream_t s) {
    const int n = j.n_verts > j.n_faces ? j.n_verts : j.n_faces;
    hipLaunchKernelGGL(lcc_gather_kernel, dim3(blocks(n)), dim3(MC_BLOCK), 0, s, verts, j.faces, j.n_verts, j.n_faces, j.kf, j.of, j.kv, j.ov, out_verts,
                       cap_verts, out_faces, cap_faces);
}

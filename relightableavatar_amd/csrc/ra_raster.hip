// A differentiable mesh rasteriser on the device: ra_rasterize, ra_interpolate and their backward passes.  The arithmetic of a
// (pixel, face) pair is ra_raster_rules.hpp's, which also states the rule and proves the complementarity lemma.
//
// Forward, three stages.
//   Set-up: one lane per (view, face) writes the face record (three canonical edge triples, the sign bits, z and w of the corners,
//       the pixel box) and the number of 8 x 8 tiles its box touches.  A vertex index outside [0, V) sets a flag and drops the face.
//   Binning: an exclusive sum of the tile counts (hipcub), one lane per (view, face) emits its (tile, face) keys — (view tile) << 24 |
//       face, F < 2^24 — and one radix sort (hipcub) groups them by tile, faces ascending.  The pair count and the index flag are
//       read back together: the ONE blocking read-back of the call (8 bytes); it sizes the key buffers.
//   Tile kernel: one wave64 per tile, one lane per pixel.  The tile's run of the sorted keys is found by two binary searches; the
//       wave walks it with wave-uniform record fetches and every lane keeps the lexicographic minimum of (zw, face).
//   RA_RASTER_BRUTE: the tile kernel walks all F records of its view instead; no binning.  The same bits, because the pixel box is
//       part of the per-pair rule and the depth rule does not depend on the order in which faces are seen.
//
// Backward.  No float atomics; every output row is a function of its inputs alone.
//   Pixels are grouped by face with one radix sort of the keys (view face) * HW + pixel (an empty pixel sorts behind everything): the
//   run of a (view, face) holds its pixels ascending.  One wave per (view, face) finds its run by binary search; lane l adds the
//   pixels l, l + 64, ... of the run in that order, and the 64 lane sums meet in a fixed xor tree (32, 16, .., 1).  It writes the
//   face's corner gradients to scratch.  A vertex pass adds a vertex's corners in ascending half-edge order through the topology's
//   vertex -> half-edge lists (as ra_cloth.hip does); shared attributes add the views in ascending order, each view's sum first.
#include "ra_kernels.hpp"
#include "ra_raster_rules.hpp"
#include <hipcub/hipcub.hpp>

#pragma clang fp contract(off)

namespace {

using u64 = unsigned long long;

inline int blocks(long long n, int per) { return (int)((n + per - 1) / per); }

__device__ __forceinline__ void raster_store(const RasterFace& r, float4* rec) {
    rec[0] = make_float4(r.c[0], r.c[1], r.c[2], r.c[3]);
    rec[1] = make_float4(r.c[4], r.c[5], r.c[6], r.c[7]);
    rec[2] = make_float4(r.c[8], __int_as_float(r.flags), r.z[0], r.z[1]);
    rec[3] = make_float4(r.z[2], r.w[0], r.w[1], r.w[2]);
    rec[4] = make_float4(__int_as_float(r.box[0]), __int_as_float(r.box[1]), __int_as_float(r.box[2]), __int_as_float(r.box[3]));
}
__device__ __forceinline__ void raster_load(const float4* rec, RasterFace& r) {
    const float4 a = rec[0], b = rec[1], c = rec[2], d = rec[3], e = rec[4];
    r.c[0] = a.x; r.c[1] = a.y; r.c[2] = a.z; r.c[3] = a.w; r.c[4] = b.x; r.c[5] = b.y; r.c[6] = b.z; r.c[7] = b.w; r.c[8] = c.x;
    r.flags = __float_as_int(c.y);
    r.z[0] = c.z; r.z[1] = c.w; r.z[2] = d.x; r.w[0] = d.y; r.w[1] = d.z; r.w[2] = d.w;
    r.box[0] = __float_as_int(e.x); r.box[1] = __float_as_int(e.y); r.box[2] = __float_as_int(e.z); r.box[3] = __float_as_int(e.w);
}

// the tiles a record's box touches: tx0, ty0, tx1, ty1 (inclusive); false when it touches none
__device__ __forceinline__ bool raster_tiles(const RasterFace& r, int* t) {
    if (!(r.flags & RASTER_VALID) || r.box[0] > r.box[2] || r.box[1] > r.box[3]) return false;
    t[0] = r.box[0] / RASTER_TILE; t[1] = r.box[1] / RASTER_TILE; t[2] = r.box[2] / RASTER_TILE; t[3] = r.box[3] / RASTER_TILE;
    return true;
}

// faces: nullptr = the corners of face f are vert[3 f + k] of a topology (checked when it was built)
__device__ __forceinline__ bool raster_face_record(const float* __restrict__ pos, const int* __restrict__ faces, int b, int f, int V, int H, int W,
                                                   RasterFace& r) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) {
        for (int k = 0; k < 9; ++k) r.c[k] = 0.0f;
        for (int k = 0; k < 3; ++k) r.z[k] = r.w[k] = 0.0f;
        r.flags = 0; r.box[0] = r.box[1] = 0; r.box[2] = r.box[3] = -1;
        return false;
    }
    const float* p = pos + 4ll * b * V;
    raster_setup(p + 4ll * i0, p + 4ll * i1, p + 4ll * i2, i0, i1, i2, H, W, r);
    return true;
}

__global__ __launch_bounds__(RASTER_BLOCK) void raster_setup_kernel(RasterJob j) {
    const long long idx = (long long)blockIdx.x * RASTER_BLOCK + threadIdx.x;
    const long long n = (long long)j.B * j.F;
    if (idx >= n) return;
    const int b = (int)(idx / j.F), f = (int)(idx - (long long)b * j.F);
    RasterFace r;
    if (!raster_face_record(j.pos, j.faces, b, f, j.V, j.H, j.W, r)) atomicOr(j.stat + 1, 1);
    raster_store(r, j.recs + 5 * idx);
    if (j.counts) {
        int t[4];
        j.counts[idx] = raster_tiles(r, t) ? (u64)(t[2] - t[0] + 1) * (u64)(t[3] - t[1] + 1) : 0ull;
        if (idx == 0) j.counts[n] = 0ull;
    }
}

__global__ void raster_total_kernel(const u64* __restrict__ off, long long n, int* __restrict__ stat) {
    const u64 total = off[n];
    stat[0] = total > 0x7fffffffull ? 0x7fffffff : (int)total;
}

__global__ __launch_bounds__(RASTER_BLOCK) void raster_emit_kernel(RasterJob j, int tiles_x, int tiles_y, long long n_pairs) {
    const long long idx = (long long)blockIdx.x * RASTER_BLOCK + threadIdx.x;
    if (idx >= (long long)j.B * j.F) return;
    const int b = (int)(idx / j.F), f = (int)(idx - (long long)b * j.F);
    RasterFace r;
    raster_load(j.recs + 5 * idx, r);
    int t[4];
    if (!raster_tiles(r, t)) return;
    u64 at = j.off[idx];
    const u64 base = (u64)b * tiles_x * tiles_y;
    for (int ty = t[1]; ty <= t[3]; ++ty)
        for (int tx = t[0]; tx <= t[2]; ++tx) {
            if (at < (u64)n_pairs) j.keys[at] = ((base + (u64)ty * tiles_x + tx) << 24) | (u64)f;       // at < off[idx + 1] <= n_pairs
            ++at;
        }
}

// the first index of the ascending keys[0, n) that holds a key >= x
__device__ __forceinline__ long long lower_bound(const u64* __restrict__ keys, long long n, u64 x) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void raster_tile_kernel(RasterJob j, const u64* __restrict__ keys, long long n_pairs, int tiles_x, int tiles_y) {
    const long long tile = blockIdx.x;
    const int per_view = tiles_x * tiles_y;
    const int b = (int)(tile / per_view), t = (int)(tile - (long long)b * per_view), ty = t / tiles_x, tx = t - ty * tiles_x;
    const int lane = threadIdx.x, ix = tx * RASTER_TILE + (lane & (RASTER_TILE - 1)), iy = ty * RASTER_TILE + lane / RASTER_TILE;
    const float px = raster_centre(ix, j.W), py = raster_centre(iy, j.H);
    long long lo = 0, hi = j.F;
    if (keys) {
        lo = lower_bound(keys, n_pairs, (u64)tile << 24);
        hi = lower_bound(keys, n_pairs, (u64)(tile + 1) << 24);
    }
    float best_u = 0.0f, best_v = 0.0f, best_zw = 0.0f;
    int best_f = -1;
    const float4* recs = j.recs + 5ll * b * j.F;
    for (long long i = lo; i < hi; ++i) {
        int f = keys ? (int)(keys[i] & 0xffffffull) : (int)i;
        f = __builtin_amdgcn_readfirstlane(f);          // the same for the whole wave: the record is fetched once
        if (f >= j.F) continue;                         // cannot happen with keys this call wrote
        RasterFace r;
        raster_load(recs + 5ll * f, r);
        RasterSample s;
        if (raster_sample(r, ix, iy, px, py, s) && raster_closer(s.zw, f, best_zw, best_f)) {
            best_u = s.u; best_v = s.v; best_zw = s.zw; best_f = f;
        }
    }
    if (ix < j.W && iy < j.H) {
        const long long p = ((long long)b * j.H + iy) * j.W + ix;
        j.uv[2 * p] = best_u; j.uv[2 * p + 1] = best_v;
        j.zw[p] = best_zw;
        j.face[p] = best_f;
    }
}

__global__ __launch_bounds__(RASTER_BLOCK) void interp_kernel(InterpJob j) {
    const long long idx = (long long)blockIdx.x * RASTER_BLOCK + threadIdx.x;
    const long long HW = (long long)j.H * j.W;
    if (idx >= (long long)j.B * HW * j.A) return;
    const long long p = idx / j.A;
    const int ch = (int)(idx - p * j.A), b = (int)(p / HW);
    const int f = j.face[p];
    float o = 0.0f;
    if (f >= 0 && f < j.F) {
        const int i0 = j.faces[3 * f], i1 = j.faces[3 * f + 1], i2 = j.faces[3 * f + 2];
        if (i0 >= 0 && i0 < j.V && i1 >= 0 && i1 < j.V && i2 >= 0 && i2 < j.V) {
            const float* a = j.attr + (j.per_view ? (long long)b * j.V * j.A : 0ll);
            const float u = j.uv[2 * p], v = j.uv[2 * p + 1];
            o = raster_interp(u, v, raster_b2(u, v), a[(long long)i0 * j.A + ch], a[(long long)i1 * j.A + ch], a[(long long)i2 * j.A + ch]);
        }
    }
    j.out[idx] = o;
}

// d loss / d (u, v) of a pixel: the channels in ascending order
__global__ __launch_bounds__(RASTER_BLOCK) void interp_duv_kernel(InterpJob j, const float* __restrict__ dout, float* __restrict__ duv) {
    const long long p = (long long)blockIdx.x * RASTER_BLOCK + threadIdx.x;
    const long long HW = (long long)j.H * j.W;
    if (p >= (long long)j.B * HW) return;
    const int b = (int)(p / HW), f = j.face[p];
    float du = 0.0f, dv = 0.0f;
    if (f >= 0 && f < j.F) {
        const float* a = j.attr + (j.per_view ? (long long)b * j.V * j.A : 0ll);
        const float *a0 = a + (long long)j.faces[3 * f] * j.A, *a1 = a + (long long)j.faces[3 * f + 1] * j.A, *a2 = a + (long long)j.faces[3 * f + 2] * j.A;
        for (int ch = 0; ch < j.A; ++ch) {
            const float d = dout[p * j.A + ch];
            const float e0 = a0[ch] - a2[ch], e1 = a1[ch] - a2[ch];
            du = du + d * e0;
            dv = dv + d * e1;
        }
    }
    duv[2 * p] = du; duv[2 * p + 1] = dv;
}

__global__ __launch_bounds__(RASTER_BLOCK) void pixel_keys_kernel(const int* __restrict__ face, int B, int F, long long HW, u64* __restrict__ keys) {
    const long long p = (long long)blockIdx.x * RASTER_BLOCK + threadIdx.x;
    if (p >= (long long)B * HW) return;
    const int b = (int)(p / HW), f = face[p];
    keys[p] = f >= 0 && f < F ? ((u64)b * F + f) * (u64)HW + (u64)(p - (long long)b * HW) : (u64)B * F * (u64)HW;
}

__device__ __forceinline__ float wave_tree(float x) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) x = x + __shfl_xor(x, w, 64);
    return x;
}

// one wave per (view, face): g_face[((b F + f) 3 + corner) A + ch] = the sum over the face's pixels of b_corner d out
__global__ __launch_bounds__(64) void interp_face_kernel(InterpJob j, const u64* __restrict__ keys, const float* __restrict__ dout, float* __restrict__ g_face) {
    const long long bf = blockIdx.x;
    const u64 HW = (u64)j.H * j.W;
    const long long n = (long long)j.B * (long long)HW;
    const long long lo = lower_bound(keys, n, (u64)bf * HW), hi = lower_bound(keys, n, (u64)(bf + 1) * HW);
    const int lane = threadIdx.x, b = (int)(bf / j.F);
    float* g = g_face + 3ll * bf * j.A;
    if (lo == hi) {
        for (int k = lane; k < 3 * j.A; k += 64) g[k] = 0.0f;
        return;
    }
    for (int ch = 0; ch < j.A; ++ch) {
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
        for (long long i = lo + lane; i < hi; i += 64) {
            const long long p = (long long)b * (long long)HW + (long long)(keys[i] - (u64)bf * HW);
            const float u = j.uv[2 * p], v = j.uv[2 * p + 1], d = dout[p * j.A + ch];
            s0 = s0 + u * d;
            s1 = s1 + v * d;
            s2 = s2 + raster_b2(u, v) * d;
        }
        s0 = wave_tree(s0); s1 = wave_tree(s1); s2 = wave_tree(s2);
        if (lane == 0) { g[ch] = s0; g[j.A + ch] = s1; g[2 * j.A + ch] = s2; }
    }
}

// d attr: one lane per (row, vertex, channel); shared attributes add the views in ascending order
__global__ __launch_bounds__(RASTER_BLOCK) void interp_vertex_kernel(InterpJob j, TopoView t, const float* __restrict__ g_face, float* __restrict__ dattr) {
    const long long idx = (long long)blockIdx.x * RASTER_BLOCK + threadIdx.x;
    const int rows = j.per_view ? j.B : 1;
    if (idx >= (long long)rows * j.V * j.A) return;
    const long long rv = idx / j.A;
    const int ch = (int)(idx - rv * j.A), row = (int)(rv / j.V), v = (int)(rv - (long long)row * j.V);
    float total = 0.0f;
    for (int b = j.per_view ? row : 0; b < (j.per_view ? row + 1 : j.B); ++b) {
        const float* base = g_face + 3ll * b * j.F * j.A;
        float s = 0.0f;
        for (int k = t.out_start[v]; k < t.out_start[v + 1]; ++k) s = s + base[(long long)t.out_he[k] * j.A + ch];      // (face, corner) = the half-edge
        total = total + s;
    }
    dattr[idx] = total;
}

// one wave per (view, face): the nine sums G_k = sum g_k p over the face's pixels, then the corner gradients (x, y, w) to g_face[9 (b F + f)]
__global__ __launch_bounds__(64) void raster_face_bwd_kernel(RasterBwdJob j, TopoView t, const u64* __restrict__ keys, float* __restrict__ g_face) {
    const long long bf = blockIdx.x;
    const u64 HW = (u64)j.H * j.W;
    const long long n = (long long)j.B * (long long)HW;
    const long long lo = lower_bound(keys, n, (u64)bf * HW), hi = lower_bound(keys, n, (u64)(bf + 1) * HW);
    const int lane = threadIdx.x, b = (int)(bf / t.n_faces), f = (int)(bf - (long long)b * t.n_faces);
    float* out = g_face + 9 * bf;
    if (lo == hi) {
        if (lane < 9) out[lane] = 0.0f;
        return;
    }
    RasterFace r;
    raster_face_record(j.pos, t.vert, b, f, t.n_verts, j.H, j.W, r);
    const bool n0 = (r.flags & RASTER_SIGN0) != 0, n1 = (r.flags & RASTER_SIGN1) != 0, n2 = (r.flags & RASTER_SIGN2) != 0;
    float G[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (long long i = lo + lane; i < hi; i += 64) {
        const long long q = (long long)(keys[i] - (u64)bf * HW), p = (long long)b * (long long)HW + q;
        const int iy = (int)(q / j.W), ix = (int)(q - (long long)iy * j.W);
        const float px = raster_centre(ix, j.W), py = raster_centre(iy, j.H);
        const float E0 = raster_edge_at(r.c, px, py), E1 = raster_edge_at(r.c + 3, px, py), E2 = raster_edge_at(r.c + 6, px, py);
        const float e0 = n0 ? -E0 : E0, e1 = n1 ? -E1 : E1, e2 = n2 ? -E2 : E2;
        const float e01 = e0 + e1;
        const float S = e01 + e2;
        float g[3];
        raster_bary_grad(j.uv[2 * p], j.uv[2 * p + 1], S, j.duv[2 * p], j.duv[2 * p + 1], g);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            G[3 * k] = G[3 * k] + g[k] * px;
            G[3 * k + 1] = G[3 * k + 1] + g[k] * py;
            G[3 * k + 2] = G[3 * k + 2] + g[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = wave_tree(G[k]);
    if (lane == 0) {
        const float* p = j.pos + 4ll * b * t.n_verts;
        float V[3][3], o[9];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* c = p + 4ll * t.vert[3 * f + k];
            V[k][0] = c[0]; V[k][1] = c[1]; V[k][2] = c[3];
        }
        raster_corner_grad(G, V[0], V[1], V[2], o);
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = o[k];
    }
}

// d pos: one lane per (view, vertex); the corners in ascending half-edge order; z carries no gradient
__global__ __launch_bounds__(RASTER_BLOCK) void raster_vertex_bwd_kernel(RasterBwdJob j, TopoView t, const float* __restrict__ g_face) {
    const long long idx = (long long)blockIdx.x * RASTER_BLOCK + threadIdx.x;
    if (idx >= (long long)j.B * t.n_verts) return;
    const int b = (int)(idx / t.n_verts), v = (int)(idx - (long long)b * t.n_verts);
    const float* base = g_face + 9ll * b * t.n_faces;
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (int k = t.out_start[v]; k < t.out_start[v + 1]; ++k) {
        const float* g = base + 3ll * t.out_he[k];
        for (int c = 0; c < 3; ++c) s[c] = s[c] + g[c];
    }
    float* o = j.dpos + 4 * idx;
    o[0] = s[0]; o[1] = s[1]; o[2] = 0.0f; o[3] = s[2];
}

int sort_keys(void* temp, size_t temp_bytes, const u64* in, u64* out, long long n, u64 largest, hipStream_t s) {
    int end_bit = 1;
    while (end_bit < 64 && (largest >> end_bit) != 0) ++end_bit;
    return hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, in, out, (int)n, 0, end_bit, s) == hipSuccess ? 0 : 1;
}

}  // namespace

size_t raster_temp_bytes(long long n_scan, long long n_sort) {
    size_t a = 0, b = 0;
    if (n_scan > 0) hipcub::DeviceScan::ExclusiveSum(nullptr, a, (const u64*)nullptr, (u64*)nullptr, (int)n_scan);
    if (n_sort > 0) hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const u64*)nullptr, (u64*)nullptr, (int)n_sort, 0, 64);
    return a > b ? a : b;
}

// B, F, H, W >= 1.  counts == nullptr (the brute scan): records and the index flag only
int launch_raster_setup(const RasterJob& j, hipStream_t s) {
    const long long n = (long long)j.B * j.F;
    hipLaunchKernelGGL(raster_setup_kernel, dim3(blocks(n, RASTER_BLOCK)), dim3(RASTER_BLOCK), 0, s, j);
    if (!j.counts) return 0;
    size_t tb = j.temp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(j.temp, tb, (const u64*)j.counts, j.off, (int)(n + 1), s) != hipSuccess) return 1;
    hipLaunchKernelGGL(raster_total_kernel, dim3(1), dim3(1), 0, s, (const u64*)j.off, n, j.stat);
    return 0;
}

// n_pairs < 0: the brute scan.  Else keys / keys_sorted hold n_pairs entries (n_pairs == 0: every tile is empty)
int launch_raster_tiles(const RasterJob& j, long long n_pairs, hipStream_t s) {
    const int tiles_x = (j.W + RASTER_TILE - 1) / RASTER_TILE, tiles_y = (j.H + RASTER_TILE - 1) / RASTER_TILE;
    const long long n_tiles = (long long)j.B * tiles_x * tiles_y;
    const u64* keys = nullptr;
    if (n_pairs > 0) {
        hipLaunchKernelGGL(raster_emit_kernel, dim3(blocks((long long)j.B * j.F, RASTER_BLOCK)), dim3(RASTER_BLOCK), 0, s, j, tiles_x, tiles_y, n_pairs);
        if (sort_keys(j.temp, j.temp_bytes, j.keys, j.keys_sorted, n_pairs, ((u64)n_tiles << 24) | 0xffffffull, s)) return 1;
    }
    if (n_pairs >= 0) keys = j.keys_sorted;     // n_pairs == 0: both searches of an empty list give 0
    hipLaunchKernelGGL(raster_tile_kernel, dim3((unsigned)n_tiles), dim3(64), 0, s, j, keys, n_pairs > 0 ? n_pairs : 0ll, tiles_x, tiles_y);
    return 0;
}

void launch_interpolate(const InterpJob& j, hipStream_t s) {
    const long long n = (long long)j.B * j.H * j.W * j.A;
    hipLaunchKernelGGL(interp_kernel, dim3(blocks(n, RASTER_BLOCK)), dim3(RASTER_BLOCK), 0, s, j);
}

// the pixels of every (view, face), ascending: keys_sorted (B H W entries)
int launch_raster_pixel_sort(const int* face, int B, int F, int H, int W, u64* keys, u64* keys_sorted, void* temp, size_t temp_bytes, hipStream_t s) {
    const long long HW = (long long)H * W, n = (long long)B * HW;
    hipLaunchKernelGGL(pixel_keys_kernel, dim3(blocks(n, RASTER_BLOCK)), dim3(RASTER_BLOCK), 0, s, face, B, F, HW, keys);
    return sort_keys(temp, temp_bytes, keys, keys_sorted, n, (u64)B * F * (u64)HW, s);
}

// F >= 1 (t.n_faces == j.F), keys_sorted from launch_raster_pixel_sort; dattr / duv nullable
void launch_interpolate_backward(const InterpJob& j, const TopoView& t, const u64* keys_sorted, const float* dout, float* g_face, float* dattr, float* duv,
                                 hipStream_t s) {
    const long long n_pix = (long long)j.B * j.H * j.W;
    if (duv) hipLaunchKernelGGL(interp_duv_kernel, dim3(blocks(n_pix, RASTER_BLOCK)), dim3(RASTER_BLOCK), 0, s, j, dout, duv);
    if (!dattr) return;
    hipLaunchKernelGGL(interp_face_kernel, dim3((unsigned)((long long)j.B * j.F)), dim3(64), 0, s, j, keys_sorted, dout, g_face);
    const long long n = (long long)(j.per_view ? j.B : 1) * j.V * j.A;
    hipLaunchKernelGGL(interp_vertex_kernel, dim3(blocks(n, RASTER_BLOCK)), dim3(RASTER_BLOCK), 0, s, j, t, (const float*)g_face, dattr);
}

// t.n_faces >= 1, t.n_verts >= 1
void launch_rasterize_backward(const RasterBwdJob& j, const TopoView& t, const u64* keys_sorted, float* g_face, hipStream_t s) {
    hipLaunchKernelGGL(raster_face_bwd_kernel, dim3((unsigned)((long long)j.B * t.n_faces)), dim3(64), 0, s, j, t, keys_sorted, g_face);
    hipLaunchKernelGGL(raster_vertex_bwd_kernel, dim3(blocks((long long)j.B * t.n_verts, RASTER_BLOCK)), dim3(RASTER_BLOCK), 0, s, j, t, (const float*)g_face);
}

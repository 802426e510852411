// Silhouette antialiasing on the device: ra_antialias and its two backward passes.  The arithmetic of a pixel pair is
// ra_antialias_rules.hpp's, which also states the rule.
//
// Forward and dcolor.  One thread per (pixel, group of AA_GROUP channels).  The thread evaluates the pixel's four pairs (left, right,
//     up, down) once and walks its channels: a gather, so no atomics and no read-back; both pixels of a pair evaluate the same pure
//     function of the pair and get the same bits.  dcolor is the same gather with the blend transposed.
// dpos.  No float atomics; every output row is a function of its view's inputs alone.
//     Keys: one thread per pair slot (view, 2 pixel + axis) writes ((view HE + half-edge) 2 H W + slot) for an active pair and the
//     largest key for an inert one.  The active keys are compacted in ascending slot order (hipcub DeviceSelect, stable) and their number
//     is read back — the ONE blocking read-back of the backward, 4 bytes; it sizes the sort and the launch.  One radix sort (hipcub) of
//     the ACTIVE keys groups them by (view, half-edge), ascending pair order inside a run: the cost follows the outline, not the mesh.
//     One wave per RUN: the wave at sorted index i works when i starts a run (i == 0 or the half-edge of key i - 1 differs), finds the
//     run's end by binary search, re-evaluates its pairs, and sums d L / d C in the lane and tree order of raster_face_bwd_kernel (lane
//     l: pairs l, l + 64, ...; xor tree 32, 16, .., 1); lane 0 writes the gradients of the half-edge's tail and head (six floats) to
//     scratch, which a memset zeroed before.
//     A vertex pass adds, in ascending order of the vertex's outgoing half-edges h, the tail term of h and then the head term of the
//     half-edge before h in its face (which ends at the vertex); pos_gradient_boost multiplies the finished sum.
#include "ra_antialias.hpp"
#include "ra_antialias_rules.hpp"
#include <hipcub/hipcub.hpp>

#pragma clang fp contract(off)

namespace {

using u64 = unsigned long long;

inline int blocks(long long n, int per) { return (int)((n + per - 1) / per); }

// the four pairs of pixel (x, y) in the order left, right, up, down: does the pair exist, its first pixel, its axis, and which of its two
// pixels (x, y) is
__device__ __forceinline__ bool pixel_pair(int q, int x, int y, int H, int W, int* fx, int* fy, int* vertical, int* me) {
    *vertical = q >> 1;
    *me = (q & 1) ? 0 : 1;              // left / up: (x, y) is the pair's second pixel
    *fx = q == 0 ? x - 1 : x;
    *fy = q == 2 ? y - 1 : y;
    return q == 0 ? x > 0 : q == 1 ? x + 1 < W : q == 2 ? y > 0 : y + 1 < H;
}

// dout == nullptr: out = color blended; else out = the transposed blend of dout
__global__ __launch_bounds__(AA_BLOCK) void antialias_gather_kernel(AaJob j, TopoView t, const float* __restrict__ dout, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * AA_BLOCK + threadIdx.x;
    const int groups = (j.C + AA_GROUP - 1) / AA_GROUP;
    const long long HW = (long long)j.H * j.W;
    if (idx >= (long long)j.B * HW * groups) return;
    const long long p = idx / groups;
    const int grp = (int)(idx - p * groups), b = (int)(p / HW);
    const long long q = p - (long long)b * HW;
    const int y = (int)(q / j.W), x = (int)(q - (long long)y * j.W);
    const int* face = j.face + (long long)b * HW;
    const float* zw = j.zw + (long long)b * HW;
    const float* pos = j.pos + 4ll * b * t.n_verts;
    float w[4];
    long long other[4];
    int role[4];                // 0: the pair does nothing here, 1: (x, y) is the target, 2: it is the source
    for (int k = 0; k < 4; ++k) {
        int fx, fy, vertical, me;
        role[k] = 0; w[k] = 0.0f; other[k] = p;
        if (!pixel_pair(k, x, y, j.H, j.W, &fx, &fy, &vertical, &me)) continue;
        AaPair pr;
        antialias_pair(face, zw, pos, t.vert, t.twin, t.n_faces, j.H, j.W, fx, fy, vertical, pr);
        if (!pr.active) continue;
        const int target = antialias_target(pr);
        role[k] = target == me ? 1 : 2;
        w[k] = antialias_weight(pr);
        const long long first = (long long)b * HW + (long long)fy * j.W + fx, second = vertical ? first + j.W : first + 1;
        other[k] = me ? first : second;
    }
    const int c0 = grp * AA_GROUP, c1 = c0 + AA_GROUP < j.C ? c0 + AA_GROUP : j.C;
    for (int c = c0; c < c1; ++c) {
        if (!dout) {
            const float mine = j.color[p * j.C + c];
            float acc = mine;
            for (int k = 0; k < 4; ++k)
                if (role[k] == 1) acc = antialias_blend(acc, w[k], j.color[other[k] * j.C + c], mine);
            out[p * j.C + c] = acc;
        } else {
            const float mine = dout[p * j.C + c];
            float acc = mine;
            for (int k = 0; k < 4; ++k) {
                if (role[k] == 1) { const float term = w[k] * mine; acc = acc - term; }
                else if (role[k] == 2) { const float term = w[k] * dout[other[k] * j.C + c]; acc = acc + term; }
            }
            out[p * j.C + c] = acc;
        }
    }
}

__global__ __launch_bounds__(AA_BLOCK) void antialias_keys_kernel(AaJob j, TopoView t, u64* __restrict__ keys) {
    const long long idx = (long long)blockIdx.x * AA_BLOCK + threadIdx.x;
    const long long HW = (long long)j.H * j.W, slots = 2 * HW;
    if (idx >= (long long)j.B * slots) return;
    const int b = (int)(idx / slots);
    const long long slot = idx - (long long)b * slots, q = slot >> 1;
    const int vertical = (int)(slot & 1), y = (int)(q / j.W), x = (int)(q - (long long)y * j.W);
    const u64 he_count = 3ull * (u64)t.n_faces;
    u64 key = (u64)j.B * he_count * (u64)slots;
    if (vertical ? y + 1 < j.H : x + 1 < j.W) {
        AaPair pr;
        antialias_pair(j.face + (long long)b * HW, j.zw + (long long)b * HW, j.pos + 4ll * b * t.n_verts, t.vert, t.twin, t.n_faces, j.H, j.W, x, y, vertical, pr);
        if (pr.active) key = ((u64)b * he_count + (u64)pr.he) * (u64)slots + (u64)slot;
    }
    keys[idx] = key;
}

__device__ __forceinline__ long long lower_bound(const u64* __restrict__ keys, long long n, u64 x) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ float wave_tree(float x) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) x = x + __shfl_xor(x, w, 64);
    return x;
}

// one wave per run of the sorted active keys (first + blockIdx.x starts one, or the wave leaves):
// g_he[6 (b HE + he)] = the gradient (x, y, w) of the half-edge's tail, then of its head; zero on entry
__global__ __launch_bounds__(64) void antialias_edge_kernel(AaJob j, TopoView t, const u64* __restrict__ keys, long long n, long long first,
                                                            const float* __restrict__ dout, float* __restrict__ g_he) {
    const long long lo = first + blockIdx.x;
    if (lo >= n) return;
    const long long HW = (long long)j.H * j.W;
    const u64 slots = 2ull * (u64)HW;
    const long long bh = (long long)(keys[lo] / slots);
    if (lo > 0 && (long long)(keys[lo - 1] / slots) == bh) return;          // not the head of its run
    const long long hi = lower_bound(keys, n, (u64)(bh + 1) * slots);
    const int lane = threadIdx.x, he_count = 3 * t.n_faces, b = (int)(bh / he_count), he = (int)(bh - (long long)b * he_count);
    if (b >= j.B) return;                       // cannot happen with keys this call wrote
    float* o = g_he + 6 * bh;
    const int* face = j.face + (long long)b * HW;
    const float* zw = j.zw + (long long)b * HW;
    const float* pos = j.pos + 4ll * b * t.n_verts;
    float G[3] = {0.0f, 0.0f, 0.0f};
    for (long long i = lo + lane; i < hi; i += 64) {
        const long long slot = (long long)(keys[i] - (u64)bh * slots), q = slot >> 1;
        const int vertical = (int)(slot & 1), y = (int)(q / j.W), x = (int)(q - (long long)y * j.W);
        AaPair pr;
        antialias_pair(face, zw, pos, t.vert, t.twin, t.n_faces, j.H, j.W, x, y, vertical, pr);
        if (!pr.active) continue;               // cannot happen with keys this call wrote
        const long long first = (long long)b * HW + q, second = vertical ? first + j.W : first + 1;
        const long long tp = antialias_target(pr) ? second : first, sp = antialias_target(pr) ? first : second;
        float g = 0.0f;
        for (int c = 0; c < j.C; ++c) {
            const float diff = j.color[sp * j.C + c] - j.color[tp * j.C + c];
            const float prod = dout[tp * j.C + c] * diff;
            g = g + prod;
        }
        if (pr.alpha < 0.0f) g = -g;
        float dc[3];
        antialias_dc(pr, vertical, vertical ? j.H : j.W, g, dc);
        G[0] = G[0] + dc[0]; G[1] = G[1] + dc[1]; G[2] = G[2] + dc[2];
    }
    G[0] = wave_tree(G[0]); G[1] = wave_tree(G[1]); G[2] = wave_tree(G[2]);
    if (lane == 0) {
        const int f = he / 3, c = he - 3 * f;
        const int tail = t.vert[he], head = t.vert[3 * f + (c + 1) % 3];
        const bool tail_first = tail < head;
        const float *a = pos + 4ll * (tail_first ? tail : head), *bb = pos + 4ll * (tail_first ? head : tail);
        float da[3], db[3];
        antialias_ends(a, bb, G, da, db);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = tail_first ? da[k] : db[k];
            o[3 + k] = tail_first ? db[k] : da[k];
        }
    }
}

// d pos: one lane per (view, vertex)
__global__ __launch_bounds__(AA_BLOCK) void antialias_vertex_kernel(TopoView t, int B, const float* __restrict__ g_he, float boost, float* __restrict__ dpos) {
    const long long idx = (long long)blockIdx.x * AA_BLOCK + threadIdx.x;
    if (idx >= (long long)B * t.n_verts) return;
    const int b = (int)(idx / t.n_verts), v = (int)(idx - (long long)b * t.n_verts);
    const float* base = g_he + 18ll * b * t.n_faces;
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (int k = t.out_start[v]; k < t.out_start[v + 1]; ++k) {
        const int h = t.out_he[k], f = h / 3, c = h - 3 * f, prev = 3 * f + (c + 2) % 3;
        const float *tail = base + 6ll * h, *head = base + 6ll * prev + 3;
        for (int q = 0; q < 3; ++q) s[q] = s[q] + tail[q];
        for (int q = 0; q < 3; ++q) s[q] = s[q] + head[q];
    }
    float* o = dpos + 4 * idx;
    o[0] = s[0] * boost; o[1] = s[1] * boost; o[2] = 0.0f; o[3] = s[2] * boost;
}

}  // namespace

struct AaActive {
    u64 inert;
    __host__ __device__ __forceinline__ bool operator()(const u64& k) const { return k != inert; }
};

// the scratch of the compaction (n_select > 0) or of the sort (n_sort > 0)
size_t antialias_temp_bytes(long long n_select, long long n_sort) {
    size_t a = 0, b = 0;
    if (n_select > 0) hipcub::DeviceSelect::If(nullptr, a, (const u64*)nullptr, (u64*)nullptr, (int*)nullptr, (int)n_select, AaActive{0});
    if (n_sort > 0) hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const u64*)nullptr, (u64*)nullptr, (int)n_sort, 0, 64);
    return a > b ? a : b;
}

void launch_antialias_gather(const AaJob& j, const TopoView& t, const float* dout, float* out, hipStream_t s) {
    const long long n = (long long)j.B * j.H * j.W * ((j.C + AA_GROUP - 1) / AA_GROUP);
    hipLaunchKernelGGL(antialias_gather_kernel, dim3(blocks(n, AA_BLOCK)), dim3(AA_BLOCK), 0, s, j, t, dout, out);
}

static u64 antialias_inert_key(const AaJob& j, const TopoView& t) { return 3ull * (u64)j.B * (u64)t.n_faces * (2ull * (u64)j.H * (u64)j.W); }

// the key of every pair slot to keys (2 B H W), the active ones in ascending slot order to compact, their number to *count (device)
int launch_antialias_keys(const AaJob& j, const TopoView& t, u64* keys, u64* compact, int* count, void* temp, size_t temp_bytes, hipStream_t s) {
    const long long n = 2ll * j.B * j.H * j.W;
    hipLaunchKernelGGL(antialias_keys_kernel, dim3(blocks(n, AA_BLOCK)), dim3(AA_BLOCK), 0, s, j, t, keys);
    return hipcub::DeviceSelect::If(temp, temp_bytes, (const u64*)keys, compact, count, (int)n, AaActive{antialias_inert_key(j, t)}, s) == hipSuccess ? 0 : 1;
}

// n_active >= 0 keys in compact; sorted: as many; g_he: B x 3 F x 6, zeroed here
int launch_antialias_dpos(const AaJob& j, const TopoView& t, const float* dout, float boost, const u64* compact, u64* sorted, long long n_active, void* temp,
                          size_t temp_bytes, float* g_he, float* dpos, hipStream_t s) {
    if (hipMemsetAsync(g_he, 0, 18ull * (size_t)j.B * t.n_faces * sizeof(float), s) != hipSuccess) return 1;
    if (n_active > 0) {
        const u64 largest = antialias_inert_key(j, t);
        int end_bit = 1;
        while (end_bit < 64 && (largest >> end_bit) != 0) ++end_bit;
        if (hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, compact, sorted, (int)n_active, 0, end_bit, s) != hipSuccess) return 1;
        for (long long first = 0; first < n_active; first += AA_MAX_WAVES) {           // a launch stays far below 2^32 threads
            const long long m = n_active - first < AA_MAX_WAVES ? n_active - first : AA_MAX_WAVES;
            hipLaunchKernelGGL(antialias_edge_kernel, dim3((unsigned)m), dim3(64), 0, s, j, t, (const u64*)sorted, n_active, first, dout, g_he);
        }
    }
    hipLaunchKernelGGL(antialias_vertex_kernel, dim3(blocks((long long)j.B * t.n_verts, AA_BLOCK)), dim3(AA_BLOCK), 0, s, t, j.B, (const float*)g_he, boost, dpos);
    return 0;
}

// The rasteriser's texture path on the device: pixel differentials, the mip chain, ra_texture and its backward.  The arithmetic of a
// pixel is ra_texture_rules.hpp's, which also states the rule.  READ-BACKS: NONE in any entry point of this file.
//
// raster_db_kernel.  One lane per pixel: the face's three corners, the canonical edges as the forward computes them, texture_db.  An
//     empty pixel, a face id outside [0, F) or a vertex index outside [0, V) writes 0.
// interp_da_kernel.  One lane per pixel walks the selected channels: (da/dX, da/dY) per channel, nvdiffrast's layout.
// texture_mip_kernel.  One lane per value of level l + 1: the 2 x 2 mean of level l; one launch per level.
// texture_pixel_kernel (the forward, and duv when it is given dout).  One lane per pixel: texture_pixel decides the level pair and the
//     taps once, then the channels ascend: gathers, no atomics.
// dtex.  No float atomics; a result is a function of its inputs alone.
//     Keys: one lane per pixel writes its T = 1 / 4 / 8 tap slots (nearest / linear / trilinear): (view total + level offset + texel)
//     HWT + (pixel T + tap), or the largest key for a tap that is not read (a non-finite uv, the second level with f == 0).  The tap
//     count is NOT compacted: the inert keys sort to the end and no wave works on them, so nothing is read back.
//     One stable radix sort (hipcub) groups the taps by (view, level, texel), the slots ascending inside a run.
//     One wave per RUN (the wave at sorted index i works when i starts a run): per group of TEX_GROUP channels lane l adds taps l,
//     l + 64, ... until it meets a key of another run (no search for the run's end: most runs of a minified texture hold one tap), and
//     the lanes meet in the xor tree 32, 16, .., 1; lane 0 writes g[view][level][texel][channel], which a memset zeroed before.
//     Fold: one lane per level-0 value walks the chain from the coarsest level down, acc = g_l[y >> l, x >> l] + 0.25 acc; a shared
//     texture adds the views' results in ascending order, a per-view texture takes its own view.
#include "ra_texture.hpp"
#include <hipcub/hipcub.hpp>

#pragma clang fp contract(off)

namespace {

using u64 = unsigned long long;

inline int blocks(long long n, int per) { return (int)((n + per - 1) / per); }

__global__ __launch_bounds__(TEX_BLOCK) void raster_db_kernel(const float* __restrict__ pos, int B, int V, const int* __restrict__ faces, int F,
                                                              const int* __restrict__ face, int H, int W, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * TEX_BLOCK + threadIdx.x;
    const long long HW = (long long)H * W;
    if (idx >= (long long)B * HW) return;
    const int b = (int)(idx / HW);
    const long long q = idx - (long long)b * HW;
    const int y = (int)(q / W), x = (int)(q - (long long)y * W);
    float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int f = face[idx];
    if (f >= 0 && f < F) {
        const int i0 = faces[3ll * f], i1 = faces[3ll * f + 1], i2 = faces[3ll * f + 2];
        if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
            const float* p = pos + 4ll * b * V;
            texture_db(p + 4ll * i0, p + 4ll * i1, p + 4ll * i2, i0, i1, i2, raster_centre(x, W), raster_centre(y, H), H, W, o);
        }
    }
    float* dst = out + 4 * idx;
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2]; dst[3] = o[3];
}

__global__ __launch_bounds__(TEX_BLOCK) void interp_da_kernel(TexDaJob j, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * TEX_BLOCK + threadIdx.x;
    const long long HW = (long long)j.H * j.W;
    if (idx >= (long long)j.B * HW) return;
    const int b = (int)(idx / HW);
    float* dst = out + 2ll * j.n * idx;
    const int f = j.face[idx];
    int i0 = -1, i1 = -1, i2 = -1;
    if (f >= 0 && f < j.F) { i0 = j.faces[3ll * f]; i1 = j.faces[3ll * f + 1]; i2 = j.faces[3ll * f + 2]; }
    if (i0 < 0 || i0 >= j.V || i1 < 0 || i1 >= j.V || i2 < 0 || i2 >= j.V) {
        for (int k = 0; k < 2 * j.n; ++k) dst[k] = 0.0f;
        return;
    }
    const float* a = j.attr + (j.per_view ? (long long)b * j.V * j.A : 0ll);
    const float* src = j.rast_db + 4 * idx;
    const float db[4] = {src[0], src[1], src[2], src[3]};
    for (int k = 0; k < j.n; ++k) {
        const int c = j.ch[k];
        texture_attr_da(db, a[(long long)i0 * j.A + c], a[(long long)i1 * j.A + c], a[(long long)i2 * j.A + c], dst + 2 * k);
    }
}

__global__ __launch_bounds__(TEX_BLOCK) void texture_mip_kernel(const float* __restrict__ src, long long src_stride, float* __restrict__ dst, long long dst_stride,
                                                                int Bt, int h, int w, int C) {
    const long long idx = (long long)blockIdx.x * TEX_BLOCK + threadIdx.x;
    const long long per = (long long)h * w * C;
    if (idx >= (long long)Bt * per) return;
    const int bt = (int)(idx / per);
    const long long r = idx - (long long)bt * per;
    const int c = (int)(r % C);
    const long long t = r / C;
    const int y = (int)(t / w), x = (int)(t - (long long)y * w);
    const float* s = src + (long long)bt * src_stride;
    const long long sw = 2ll * w, row0 = (2ll * y) * sw + 2ll * x, row1 = row0 + sw;
    dst[(long long)bt * dst_stride + r] = texture_mean(s[row0 * C + c], s[(row0 + 1) * C + c], s[row1 * C + c], s[(row1 + 1) * C + c]);
}

// channel 0 of texel 0 of level l of texture bt
__device__ __forceinline__ const float* tex_level(const TexJob& j, int bt, int l) {
    if (l == 0) return j.tex + (long long)bt * j.L.off[1] * j.C;
    return j.mips + ((long long)bt * (j.L.off[j.L.n] - j.L.off[1]) + (j.L.off[l] - j.L.off[1])) * j.C;
}

__device__ __forceinline__ void tex_pixel(const TexJob& j, long long idx, TexPixel& p) {
    const float u = j.uv[2 * idx], v = j.uv[2 * idx + 1];
    float da[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (j.filter == TEX_TRILINEAR) {
        const float* s = j.uv_da + 4 * idx;
        da[0] = s[0]; da[1] = s[1]; da[2] = s[2]; da[3] = s[3];
    }
    texture_pixel(u, v, da, j.L, j.filter, j.boundary, p);
}

// dout == nullptr: o = out (C per pixel); else o = duv (2 per pixel)
__global__ __launch_bounds__(TEX_BLOCK) void texture_pixel_kernel(TexJob j, const float* __restrict__ dout, float* __restrict__ o) {
    const long long idx = (long long)blockIdx.x * TEX_BLOCK + threadIdx.x;
    const long long HW = (long long)j.H * j.W;
    if (idx >= (long long)j.B * HW) return;
    const int b = (int)(idx / HW), bt = j.Bt == 1 ? 0 : b;
    TexPixel p;
    tex_pixel(j, idx, p);
    if (dout) {
        float* dst = o + 2 * idx;
        dst[0] = 0.0f; dst[1] = 0.0f;
        if (!p.ok || j.filter == TEX_NEAREST) return;
        const int l1 = p.two ? p.l0 + 1 : p.l0;
        texture_duv(p, tex_level(j, bt, p.l0), tex_level(j, bt, l1), dout + idx * j.C, j.C, j.L.w[p.l0], j.L.h[p.l0], j.L.w[l1], j.L.h[l1], dst);
        return;
    }
    float* dst = o + idx * j.C;
    if (!p.ok) {
        for (int c = 0; c < j.C; ++c) dst[c] = 0.0f;
        return;
    }
    const float* a = tex_level(j, bt, p.l0);
    if (j.filter == TEX_NEAREST) {
        const float* t = a + (long long)p.t[0].idx[0] * j.C;
        for (int c = 0; c < j.C; ++c) dst[c] = t[c];
        return;
    }
    const float* bb = p.two ? tex_level(j, bt, p.l0 + 1) : a;
    for (int c = 0; c < j.C; ++c) dst[c] = texture_value(p, a + c, bb + c, j.C);
}

__global__ __launch_bounds__(TEX_BLOCK) void texture_keys_kernel(TexJob j, int T, u64* __restrict__ keys) {
    const long long idx = (long long)blockIdx.x * TEX_BLOCK + threadIdx.x;
    const long long HW = (long long)j.H * j.W;
    if (idx >= (long long)j.B * HW) return;
    const int b = (int)(idx / HW);
    const long long pix = idx - (long long)b * HW;
    const u64 slots = (u64)HW * (u64)T, total = (u64)j.L.off[j.L.n];
    const u64 inert = (u64)j.B * total * slots;
    TexPixel p;
    tex_pixel(j, idx, p);
    u64* dst = keys + idx * T;
    for (int k = 0; k < T; ++k) {
        u64 key = inert;
        const int second = k >> 2;
        if (p.ok && (second == 0 || p.two)) {
            const int l = p.l0 + second;
            const u64 group = (u64)b * total + (u64)j.L.off[l] + (u64)p.t[second].idx[k & 3];
            key = group * slots + (u64)pix * (u64)T + (u64)k;
        }
        dst[k] = key;
    }
}

__device__ __forceinline__ float wave_tree(float x) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) x = x + __shfl_xor(x, w, 64);
    return x;
}

// one wave per run of the sorted keys (first + blockIdx.x starts one, or the wave leaves): g[group C + c], zero on entry
__global__ __launch_bounds__(64) void texture_run_kernel(TexJob j, int T, const u64* __restrict__ keys, long long n, long long first,
                                                         const float* __restrict__ dout, float* __restrict__ g) {
    const long long lo = first + blockIdx.x;
    if (lo >= n) return;
    const long long HW = (long long)j.H * j.W;
    const u64 slots = (u64)HW * (u64)T, total = (u64)j.L.off[j.L.n];
    const u64 group = keys[lo] / slots;
    if (group >= (u64)j.B * total) return;                          // the inert keys
    if (lo > 0 && keys[lo - 1] / slots == group) return;            // not the head of its run
    const int lane = threadIdx.x, b = (int)(group / total);
    for (int c0 = 0; c0 < j.C; c0 += TEX_GROUP) {
        float G[TEX_GROUP];
#pragma unroll
        for (int k = 0; k < TEX_GROUP; ++k) G[k] = 0.0f;
        for (long long i = lo + lane; i < n; i += 64) {          // the keys are sorted: a lane leaves at the first key of another run
            const u64 key = keys[i];
            if (key / slots != group) break;
            const u64 slot = key - group * slots;
            const long long pix = (long long)(slot / (u64)T);
            const int tap = (int)(slot - (u64)pix * (u64)T);
            const long long gp = (long long)b * HW + pix;
            float wgt = 1.0f;
            if (j.filter != TEX_NEAREST) {
                TexPixel p;
                tex_pixel(j, gp, p);
                wgt = texture_tap_weight(p.f, tap >> 2, p.t[tap >> 2].w[tap & 3]);
            }
            const float* d = dout + gp * j.C;
#pragma unroll
            for (int k = 0; k < TEX_GROUP; ++k)
                if (c0 + k < j.C) {
                    const float term = wgt * d[c0 + k];
                    G[k] = G[k] + term;
                }
        }
#pragma unroll
        for (int k = 0; k < TEX_GROUP; ++k) G[k] = wave_tree(G[k]);
        if (lane == 0)
            for (int k = 0; k < TEX_GROUP; ++k)
                if (c0 + k < j.C) g[group * (u64)j.C + (u64)(c0 + k)] = G[k];
    }
}

__global__ __launch_bounds__(TEX_BLOCK) void texture_fold_kernel(TexJob j, const float* __restrict__ g, float* __restrict__ dtex) {
    const long long idx = (long long)blockIdx.x * TEX_BLOCK + threadIdx.x;
    const long long per = j.L.off[1] * j.C, total = j.L.off[j.L.n];
    if (idx >= (long long)j.Bt * per) return;
    const int bt = (int)(idx / per);
    const long long r = idx - (long long)bt * per;
    const int c = (int)(r % j.C);
    const long long t = r / j.C;
    const int y = (int)(t / j.L.w[0]), x = (int)(t - (long long)y * j.L.w[0]);
    const bool shared = j.Bt == 1;
    const int b0 = shared ? 0 : bt, b1 = shared ? j.B : bt + 1;
    float sum = 0.0f;
    for (int b = b0; b < b1; ++b) {
        const float* gb = g + (long long)b * total * j.C;
        const int top = j.L.n - 1;
        float acc = gb[(j.L.off[top] + (long long)(y >> top) * j.L.w[top] + (x >> top)) * j.C + c];
        for (int l = top - 1; l >= 0; --l) {
            const float q = 0.25f * acc;
            acc = gb[(j.L.off[l] + (long long)(y >> l) * j.L.w[l] + (x >> l)) * j.C + c] + q;
        }
        sum = b == b0 ? acc : sum + acc;
    }
    dtex[idx] = sum;
}

}  // namespace

size_t texture_temp_bytes(long long n_sort) {
    size_t b = 0;
    if (n_sort > 0) hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const u64*)nullptr, (u64*)nullptr, (int)n_sort, 0, 64);
    return b;
}

void launch_raster_db(const float* pos, int B, int V, const int* faces, int F, const int* face, int H, int W, float* rast_db, hipStream_t s) {
    hipLaunchKernelGGL(raster_db_kernel, dim3(blocks((long long)B * H * W, TEX_BLOCK)), dim3(TEX_BLOCK), 0, s, pos, B, V, faces, F, face, H, W, rast_db);
}

void launch_interpolate_da(const TexDaJob& j, float* out, hipStream_t s) {
    hipLaunchKernelGGL(interp_da_kernel, dim3(blocks((long long)j.B * j.H * j.W, TEX_BLOCK)), dim3(TEX_BLOCK), 0, s, j, out);
}

void launch_texture_mip(const float* src, long long src_stride, float* dst, long long dst_stride, int Bt, int h, int w, int C, hipStream_t s) {
    hipLaunchKernelGGL(texture_mip_kernel, dim3(blocks((long long)Bt * h * w * C, TEX_BLOCK)), dim3(TEX_BLOCK), 0, s, src, src_stride, dst, dst_stride, Bt, h, w, C);
}

void launch_texture(const TexJob& j, float* out, hipStream_t s) {
    hipLaunchKernelGGL(texture_pixel_kernel, dim3(blocks((long long)j.B * j.H * j.W, TEX_BLOCK)), dim3(TEX_BLOCK), 0, s, j, (const float*)nullptr, out);
}

void launch_texture_duv(const TexJob& j, const float* dout, float* duv, hipStream_t s) {
    hipLaunchKernelGGL(texture_pixel_kernel, dim3(blocks((long long)j.B * j.H * j.W, TEX_BLOCK)), dim3(TEX_BLOCK), 0, s, j, dout, duv);
}

int launch_texture_dtex(const TexJob& j, const float* dout, u64* keys, u64* sorted, void* temp, size_t temp_bytes, float* g, float* dtex, hipStream_t s) {
    const int T = texture_taps_per_pixel(j.filter);
    const long long n_pix = (long long)j.B * j.H * j.W, n = n_pix * T;
    const u64 total = (u64)j.L.off[j.L.n];
    if (hipMemsetAsync(g, 0, (size_t)j.B * total * j.C * sizeof(float), s) != hipSuccess) return 1;
    if (n > 0) {
        hipLaunchKernelGGL(texture_keys_kernel, dim3(blocks(n_pix, TEX_BLOCK)), dim3(TEX_BLOCK), 0, s, j, T, keys);
        const u64 largest = (u64)j.B * total * ((u64)j.H * j.W * T);
        int end_bit = 1;
        while (end_bit < 64 && (largest >> end_bit) != 0) ++end_bit;
        if (hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, (const u64*)keys, sorted, (int)n, 0, end_bit, s) != hipSuccess) return 1;
        for (long long first = 0; first < n; first += TEX_MAX_WAVES) {           // a launch stays far below 2^32 threads
            const long long m = n - first < TEX_MAX_WAVES ? n - first : TEX_MAX_WAVES;
            hipLaunchKernelGGL(texture_run_kernel, dim3((unsigned)m), dim3(64), 0, s, j, T, (const u64*)sorted, n, first, dout, g);
        }
    }
    hipLaunchKernelGGL(texture_fold_kernel, dim3(blocks((long long)j.Bt * j.L.off[1] * j.C, TEX_BLOCK)), dim3(TEX_BLOCK), 0, s, j, (const float*)g, dtex);
    return 0;
}

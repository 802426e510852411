// Silhouette antialiasing (ra_antialias.hip): the launchers behind ra_antialias / ra_antialias_backward
#pragma once
#include "ra_kernels.hpp"

constexpr int AA_BLOCK = 256;           // (pixel, channel group) / pair / (view, vertex) elements per workgroup; the half-edge pass uses one wave
constexpr int AA_GROUP = 4;             // channels per thread of the forward and of dcolor: the pair decisions are made once per group
struct AaJob {
    const float* color;                 // B x H x W x C, the INPUT of the forward
    const float* pos;                   // B x V x 4 clip-space positions
    const float* zw;                    // B x H x W
    const int* face;                    // B x H x W, -1: empty
    int B, H, W, C;
};
constexpr long long AA_MAX_WAVES = 1ll << 24;      // waves per launch of the run pass: 2^30 threads
size_t antialias_temp_bytes(long long n_select, long long n_sort);
// out = the blend (dout == nullptr), or dcolor = its transpose applied to dout
void launch_antialias_gather(const AaJob& j, const TopoView& t, const float* dout, float* out, hipStream_t s);
// dpos (B x V x 4) in two steps around the one read-back.  keys, compact: 2 B H W entries; count: 1 int on the device;
// sorted: n_active entries; g_he: B x 3 F x 6; t.n_faces, t.n_verts, B H W >= 1
int launch_antialias_keys(const AaJob& j, const TopoView& t, unsigned long long* keys, unsigned long long* compact, int* count, void* temp, size_t temp_bytes,
                          hipStream_t s);
int launch_antialias_dpos(const AaJob& j, const TopoView& t, const float* dout, float boost, const unsigned long long* compact, unsigned long long* sorted,
                          long long n_active, void* temp, size_t temp_bytes, float* g_he, float* dpos, hipStream_t s);

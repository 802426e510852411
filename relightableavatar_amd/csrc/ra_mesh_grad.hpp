// The closest-point query's backward (ra_mesh_grad.hip): the launcher behind ra_mesh_closest_backward
#pragma once
#include "ra_kernels.hpp"
#include "ra_mesh_grad_rules.hpp"

constexpr int MESHG_BLOCK = 256;        // rows per workgroup of the row kernel; the run pass uses one wave
constexpr int MESHG_GROUP = 4;          // channels a wave of the run pass sums per trip over its run
constexpr long long MESHG_MAX_WAVES = 1ll << 24;
struct MeshGradJob {
    const int* faces;                   // F x 3
    const float* pts;                   // n x 3
    const float* closest;               // n x 3
    const int* face;                    // n
    const float* bary;                  // n x 3
    const float* g_d2;                  // n; nullable when neither dpts nor dverts is asked for
    const float* g_attr;                // n x C; nullable when dattr is not asked for
    int F, V, n, C;
    float *dpts, *dverts, *dattr;       // n x 3, V x 3, V x C; each nullable
};
struct MeshGradScratch {                // all on the device; read only when dverts or dattr is asked for
    unsigned long long *keys, *sorted;  // 3 n entries each
    unsigned char* flags;               // 3 n: 1 where a sorted index starts a vertex's run
    unsigned* heads;                    // 3 n at most: the indices of the run heads, compacted
    unsigned* count;                    // 1: how many there are
    void *sort_temp, *select_temp;
    size_t sort_bytes, select_bytes;    // mesh_grad_sort_bytes / mesh_grad_select_bytes of 3 n
};
size_t mesh_grad_sort_bytes(long long n_keys);
size_t mesh_grad_select_bytes(long long n_keys);
// the vertex-sized outputs are zeroed here
int launch_mesh_closest_backward(const MeshGradJob& j, const MeshGradScratch& t, hipStream_t s);

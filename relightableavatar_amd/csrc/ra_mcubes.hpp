// Marching cubes and the largest edge-connected component of a mesh (ra_mcubes.hip): what the host entry points (ra_api_ops.cpp) see
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

constexpr int MC_BLOCK = 256;                    // grid points / faces / edges per workgroup
constexpr int MC_MAX_POINTS = 1 << 27;           // 3 vertices and 5 faces of 3 indices per point stay below 2^31
constexpr int LCC_MAX_FACES = 1 << 27;
constexpr int LCC_PASSES = 64;                   // label passes queued per look at the labels' state; a pass behind one that changed nothing exits at once
struct McJob {
    const float* vol;       // nx x ny x nz, x slowest
    int nx, ny, nz;
    float iso;
    unsigned long long *cnt, *off;      // n + 1 packed (vertices | triangles << 32) counts and their exclusive sum; off[n]: the totals
    unsigned char* mask;    // n: which of the point's three edges carry a vertex
    void* temp;
    size_t temp_bytes;
};
struct LccJob {
    const int* faces;       // n_faces x 3
    int n_faces, n_verts;
    unsigned long long *keys, *keys_sorted;     // 3 n_faces
    int *slots, *slots_sorted;                  // 3 n_faces
    int* link;              // 6 n_faces: per face corner the faces before / behind it on its edge
    int *label, *size;      // n_faces
    int *kf, *of;           // n_faces + 1: keep flag and new index of a face
    int *kv, *ov;           // n_verts + 1: of a vertex
    int* stat;              // LCC_STAT_INTS ints
    void* temp;
    size_t temp_bytes;
};
// stat: [0] faces with an index outside [0, n_verts)   [2..3] the winner, (size << 32 | ~label) as one 64-bit word
// [LCC_FLAGS + k] pass k of the batch lowered a label
enum { LCC_BAD = 0, LCC_BEST = 2, LCC_FLAGS = 4, LCC_STAT_INTS = LCC_FLAGS + LCC_PASSES };
// The scalar volume of mesh extraction (ra_sdf_volume): the K-NN filter over the grid points, their compaction, the scatter
constexpr int VOL_MAX_K = 4;                     // nearest vertices the filter can weigh (cfg.sample_vert_cnt is 3)
constexpr int VOL_TILE = 256;                    // vertices staged in LDS per step of the filter = its workgroup size
struct VolJob {
    const float *xs, *ys, *zs;      // the axes: nx, ny, nz coordinates
    int nx, ny, nz, pad;
    const float* verts;     // n_verts x 3: what the filter measures against
    int n_verts, K;
    float dist_th;
    int *flag, *off;        // n + 1: kept flag of a grid point and its exclusive sum; off[n]: the kept count
    void* temp;
    size_t temp_bytes;
};
int launch_vol_filter(const VolJob& j, hipStream_t s);
// pts[3 i], cell[i] of kept point i (cell: its linear index in the padded volume)
void launch_vol_compact(const VolJob& j, float* pts, int* cell, hipStream_t s);
void launch_vol_fill(float* volume, long long n, float fill, hipStream_t s);
void launch_vol_scatter(const float* sdf, const int* cell, const int* count, int cap, float* volume, hipStream_t s);
size_t mc_scan_temp_bytes(int n);
size_t lcc_sort_temp_bytes(int n);
int launch_mc_count(const McJob& j, hipStream_t s);
void launch_mc_emit(const McJob& j, float* verts, int n_verts, int* faces, int n_faces, hipStream_t s);
// The backward of marching cubes and its vertex attributes (ra_mcubes_grad.hip), behind launch_mc_count on a McJob whose buffers are the
// backward's own, so that a pending size query of the forward keeps its offsets
void launch_mcg_attrs(const McJob& j, const float* attrs, int C, int n_verts, float* out, hipStream_t s);
void launch_mcg_backward(const McJob& j, const float* dverts, int n_verts, const float* attrs, const float* dattr, int C, float* dvolume, float* dattrs_grid,
                         hipStream_t s);
int launch_lcc_links(const LccJob& j, hipStream_t s);
void launch_lcc_passes(const LccJob& j, hipStream_t s);
int launch_lcc_select(const LccJob& j, hipStream_t s);
void launch_lcc_gather(const LccJob& j, const float* verts, float* out_verts, int cap_verts, int* out_faces, int cap_faces, hipStream_t s);

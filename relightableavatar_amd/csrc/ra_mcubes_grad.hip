// The backward of marching cubes and the grid attributes carried to its vertices (ra_marching_cubes_backward, ra_marching_cubes_attrs).
// The rule is ra_mcubes_grad_rules.hpp; this file is its schedule.
//
// One thread per grid point p = (x * ny + y) * nz + z, z fastest, as in the forward: a wave reads and writes 64 consecutive points.
// A call is the forward's own classify pass and exclusive sum (launch_mc_count of ra_mcubes.hip: ONE place decides which edges are
// crossed and what their vertices' indices are) into scratch of the backward's own, then one pass over the grid points and no read-back:
//   attrs      a point writes the attributes of the vertices it owns, in the forward's vertex order;
//   backward   a point GATHERS over the at most six crossed edges that end in it — its own three, then those owned by its three lower
//              neighbours — in that fixed order from +0.  d vertex / d volume has two entries per vertex, so its transpose is this
//              gather: no atomic, one summation order, the same bits on every run.  The channel loop runs inside the lane; the six
//              edge records live in registers.
// Every vertex access is bounded by n_verts: a volume that changed since the forward gives a wrong result, never an access outside
// the arrays.  Every output element is written by exactly one lane, zeros included.
#include "ra_mcubes.hpp"
#include "ra_mcubes_grad_rules.hpp"

#pragma clang fp contract(off)

namespace {

inline int blocks(long long n) { return (int)((n + MC_BLOCK - 1) / MC_BLOCK); }

__global__ __launch_bounds__(MC_BLOCK) void mcg_attrs_kernel(McJob j, const float* __restrict__ A, int C, int n_verts, float* __restrict__ out) {
    const int n = j.nx * j.ny * j.nz;
    const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (p >= n) return;
    const unsigned m = j.mask[p];
    if (!m) return;
    const unsigned o = (unsigned)j.off[p];       // the low half: the vertex offset
    const float a = j.vol[p];
    const int stride[3] = {j.ny * j.nz, j.nz, 1};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned vi = o + mcg_slot(m, k);
        if (!((m >> k) & 1u) || vi >= (unsigned)n_verts) continue;
        const int q = p + stride[k];
        McgEdge e;
        mcg_edge(a, j.vol[q], j.iso, e);
        const float *Ap = A + (size_t)p * C, *Aq = A + (size_t)q * C;
        float* dst = out + (size_t)vi * C;
        for (int c = 0; c < C; ++c) dst[c] = mcg_attr(e, Ap[c], Aq[c]);
    }
}

__global__ __launch_bounds__(MC_BLOCK) void mcg_backward_kernel(McJob j, const float* __restrict__ dverts, int n_verts, const float* __restrict__ A,
                                                                const float* __restrict__ dattr, int C, float* __restrict__ dvol, float* __restrict__ dA) {
    const int n = j.nx * j.ny * j.nz;
    const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int coord[3] = {p / (j.nz * j.ny), (p / j.nz) % j.ny, p % j.nz};
    const int stride[3] = {j.ny * j.nz, j.nz, 1};
    const float a0 = j.vol[p];
    // slots 0..2: the edges this point owns (it is their a end), 3..5: those arriving from -x, -y, -z (it is their b end)
    McgEdge e[6];
    bool on[6];
    unsigned v[6];
    int other[6];
    const unsigned m = j.mask[p], o = (unsigned)j.off[p];       // the low half of the packed sum: the vertex offset
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        on[k] = false; v[k] = 0; other[k] = p;
        if ((m >> k) & 1u) {                    // set only where the neighbour exists
            v[k] = o + mcg_slot(m, k);
            other[k] = p + stride[k];
            if (v[k] < (unsigned)n_verts) on[k] = mcg_edge(a0, j.vol[other[k]], j.iso, e[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        on[3 + k] = false; v[3 + k] = 0; other[3 + k] = p;
        if (coord[k] > 0) {
            const int pm = p - stride[k];
            const unsigned mm = j.mask[pm];
            if ((mm >> k) & 1u) {
                v[3 + k] = (unsigned)j.off[pm] + mcg_slot(mm, k);
                other[3 + k] = pm;
                if (v[3 + k] < (unsigned)n_verts) on[3 + k] = mcg_edge(j.vol[pm], a0, j.iso, e[3 + k]);
            }
        }
    }
    float gt[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) gt[i] = (on[i] && dverts) ? dverts[3 * (size_t)v[i] + (i % 3)] : 0.0f;
    const bool any = on[0] || on[1] || on[2] || on[3] || on[4] || on[5];
    if (C > 0) {
        float* dst = dA ? dA + (size_t)p * C : nullptr;
        if (!any) {
            if (dst) for (int c = 0; c < C; ++c) dst[c] = 0.0f;
        } else {
            const float* Ag = A + (size_t)p * C;
            for (int c = 0; c < C; ++c) {
                const float mine = Ag[c];
                float acc = 0.0f;
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    if (!on[i]) continue;
                    const float theirs = A[(size_t)other[i] * C + c], g = dattr[(size_t)v[i] * C + c];
                    if (i < 3) { gt[i] = mcg_gt_add(gt[i], g, mine, theirs); acc = acc + mcg_dAp(e[i], g); }
                    else       { gt[i] = mcg_gt_add(gt[i], g, theirs, mine); acc = acc + mcg_dAq(e[i], g); }
                }
                if (dst) dst[c] = acc;
            }
        }
    }
    if (dvol) {
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if (!on[i]) continue;
            const float s = mcg_s(e[i], gt[i]);
            acc = acc + (i < 3 ? mcg_ca(e[i], s) : mcg_cb(e[i], s));
        }
        dvol[p] = acc;
    }
}

}  // namespace

void launch_mcg_attrs(const McJob& j, const float* attrs, int C, int n_verts, float* out, hipStream_t s) {
    hipLaunchKernelGGL(mcg_attrs_kernel, dim3(blocks(j.nx * j.ny * j.nz)), dim3(MC_BLOCK), 0, s, j, attrs, C, n_verts, out);
}

void launch_mcg_backward(const McJob& j, const float* dverts, int n_verts, const float* attrs, const float* dattr, int C, float* dvolume, float* dattrs_grid,
                         hipStream_t s) {
    hipLaunchKernelGGL(mcg_backward_kernel, dim3(blocks(j.nx * j.ny * j.nz)), dim3(MC_BLOCK), 0, s, j, dverts, n_verts, attrs, dattr, C, dvolume, dattrs_grid);
}

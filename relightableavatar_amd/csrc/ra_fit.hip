// Mesh fitting on the device: the large-steps operator M = I + lambda L and its solve (ra_topo_diffuse_apply / _solve), vertex and face
// normals (ra_mesh_normals), the ICP residual behind a closest-point query (ra_icp_residual) and the AdamUniform step
// (ra_adam_uniform_step) — what the reference's bidirectional_icp_fitting (lib/utils/mesh_utils.py:265-379) takes from largesteps,
// pytorch3d and bvh_distance_queries.
//
// Arithmetic.  fp32 in and out, float64 state, every operation a named one of ra_fit_rules.hpp, contraction off.  One thread owns one
// (vertex, channel) result and adds its neighbours in ascending order, as the smoothing pass does.
//
// The solve is Jacobi-preconditioned conjugate gradients, the C channels C independent systems.  Its kernels run on a grid of
// (vertex tiles, channels): a workgroup holds FIT_BLOCK vertices of ONE channel, so a sum over a channel is FIT_BLOCK-wide tree sums
// in LDS (a fixed order) written as one partial per (channel, tile); one workgroup per channel then adds them, thread t the partials
// t, t + FIT_BLOCK, ... in ascending order, and the same tree over the threads.  The float64 state is channel-major, so a workgroup's
// rows are contiguous.  No float atomics, and no kernel waits for another: an iteration is four launches,
//     q:      p = z + beta p_old (every thread recomputes its neighbours' p from z and p_old: one rule, one value), q = M p, partials of p.q
//     alpha:  alpha = rz / p.q
//     update: x += alpha p, r -= alpha q, z = r / diag, partials of r.z and r.r
//     beta:   beta = rz' / rz, the iteration count, and the stopping test |r| <= tol |b|
// and the host queues max_iter of them without reading anything back.  A channel that has stopped is frozen: every workgroup of its
// row of the grid returns at once, so its result depends on its own b, x0, the topology, lambda, tol and max_iter alone.
#include "ra_kernels.hpp"
#include "ra_fit_rules.hpp"

#pragma clang fp contract(off)

namespace {

inline int blocks(long long n, int per) { return (int)((n + per - 1) / per); }

// the sum of the workgroup's FIT_BLOCK values in a fixed tree order; valid in every thread
__device__ __forceinline__ double fit_block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = FIT_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

// deg (neighbours other than v) and their ascending sum of src[. * C + ch] (float or double)
template <typename T>
__device__ __forceinline__ double fit_nbr_sum(const int* __restrict__ nbr_start, const int* __restrict__ nbr, int v, int C, int ch, const T* __restrict__ src,
                                              int* deg) {
    double s = 0.0;
    int d = 0;
    for (int k = nbr_start[v]; k < nbr_start[v + 1]; ++k) {
        const int j = nbr[k];
        if (j == v) continue;
        ++d;
        if (src) s = s + (double)src[(long long)j * C + ch];
    }
    *deg = d;
    return s;
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_apply_kernel(const int* __restrict__ nbr_start, const int* __restrict__ nbr, long long total, int C,
                                                             const float* __restrict__ x, double lambda, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * FIT_BLOCK + threadIdx.x;
    if (idx >= total) return;
    const int v = (int)(idx / C), ch = (int)(idx - (long long)v * C);
    int deg;
    const double s = fit_nbr_sum(nbr_start, nbr, v, C, ch, x, &deg);
    out[idx] = (float)fit_diffuse((double)x[idx], s, deg, lambda);
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_init_kernel(FitSolve f) {
    __shared__ double sh[FIT_BLOCK];
    const int v = blockIdx.x * FIT_BLOCK + threadIdx.x, ch = blockIdx.y;
    double rz = 0.0, rr = 0.0, bb = 0.0;
    if (v < f.n_verts) {
        const long long idx = (long long)v * f.C + ch;
        const double bv = (double)f.b[idx], xv = f.x0 ? (double)f.x0[idx] : 0.0;
        int deg;
        const double s = fit_nbr_sum(f.nbr_start, f.nbr, v, f.C, ch, f.x0, &deg);
        const double mx = fit_diffuse(xv, s, deg, f.lambda);
        const double rv = bv - mx, dg = fit_diag(deg, f.lambda);
        const double zv = rv / dg;
        const long long in = (long long)ch * f.n_verts + v;      // the state is channel-major: a workgroup's rows are contiguous
        f.x[in] = xv; f.r[in] = rv; f.z[in] = zv; f.p0[in] = zv;
        f.diag[v] = dg;                                          // every channel writes the same value
        rz = rv * zv; rr = rv * rv; bb = bv * bv;
    }
    const size_t slot = (size_t)ch * f.n_tiles + blockIdx.x, q = (size_t)f.C * f.n_tiles;
    const double a = fit_block_sum(rz, sh);
    if (threadIdx.x == 0) f.part[slot] = a;
    const double b = fit_block_sum(rr, sh);
    if (threadIdx.x == 0) f.part[q + slot] = b;
    const double c = fit_block_sum(bb, sh);
    if (threadIdx.x == 0) f.part[2 * q + slot] = c;
}

// the second stage, by a whole workgroup: thread t adds the partials t, t + FIT_BLOCK, ... in ascending order from 0, then the tree; valid
// in every thread
__device__ __forceinline__ double fit_tile_sum(const double* __restrict__ part, int n_tiles, double* sh) {
    double s = 0.0;
    for (int k = threadIdx.x; k < n_tiles; k += FIT_BLOCK) s = s + part[k];
    return fit_block_sum(s, sh);
}

__device__ __forceinline__ bool fit_finite(double x) { return x - x == 0.0; }

// one workgroup per channel; thread 0 keeps the channel's scalars
__global__ __launch_bounds__(FIT_BLOCK) void fit_start_kernel(FitSolve f) {
    __shared__ double sh[FIT_BLOCK];
    const int ch = blockIdx.x;
    const size_t q = (size_t)f.C * f.n_tiles;
    const double* part = f.part + (size_t)ch * f.n_tiles;
    const double rz = fit_tile_sum(part, f.n_tiles, sh), rr = fit_tile_sum(part + q, f.n_tiles, sh), bb = fit_tile_sum(part + 2 * q, f.n_tiles, sh);
    if (threadIdx.x != 0) return;
    FitState s{};
    s.rz = rz; s.bb = bb;
    if (!(fit_finite(rz) && fit_finite(rr) && fit_finite(bb))) { s.stop = FIT_STOP_NAN; s.relres = rr - rr + (bb - bb); }     // NaN
    else if (bb == 0.0) s.stop = FIT_STOP_ZERO;
    else {
        const double nr = sqrt(rr), nb = sqrt(bb);
        s.relres = nr / nb;
        if (nr <= f.tol * nb) s.stop = FIT_STOP_CONVERGED;
    }
    f.st[ch] = s;
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_q_kernel(FitSolve f, const double* __restrict__ p_old, double* __restrict__ p_new) {
    __shared__ double sh[FIT_BLOCK];
    const int v = blockIdx.x * FIT_BLOCK + threadIdx.x, ch = blockIdx.y;
    if (f.st[ch].stop) return;      // the whole workgroup: one channel
    const double beta = f.st[ch].beta;
    double pq = 0.0;
    if (v < f.n_verts) {
        const long long row = (long long)ch * f.n_verts, idx = row + v;
        const double bp = beta * p_old[idx];
        const double pv = f.z[idx] + bp;
        double s = 0.0;
        int deg = 0;
        for (int k = f.nbr_start[v]; k < f.nbr_start[v + 1]; ++k) {
            const int j = f.nbr[k];
            if (j == v) continue;
            ++deg;
            const long long jd = row + j;
            const double bj = beta * p_old[jd];
            const double pj = f.z[jd] + bj;
            s = s + pj;
        }
        const double qv = fit_diffuse(pv, s, deg, f.lambda);
        p_new[idx] = pv;
        f.q[idx] = qv;
        pq = pv * qv;
    }
    const double a = fit_block_sum(pq, sh);
    if (threadIdx.x == 0) f.part[(size_t)ch * f.n_tiles + blockIdx.x] = a;
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_alpha_kernel(FitSolve f) {
    __shared__ double sh[FIT_BLOCK];
    const int ch = blockIdx.x;
    if (f.st[ch].stop) return;      // the whole workgroup
    const double pq = fit_tile_sum(f.part + (size_t)ch * f.n_tiles, f.n_tiles, sh);
    if (threadIdx.x != 0) return;
    if (!(pq > 0.0)) { f.st[ch].stop = FIT_STOP_BREAKDOWN; return; }      // M is positive definite: only p = 0 or a non-finite value gets here
    f.st[ch].alpha = f.st[ch].rz / pq;
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_update_kernel(FitSolve f, const double* __restrict__ p) {
    __shared__ double sh[FIT_BLOCK];
    const int v = blockIdx.x * FIT_BLOCK + threadIdx.x, ch = blockIdx.y;
    if (f.st[ch].stop) return;
    const double alpha = f.st[ch].alpha;
    double rz = 0.0, rr = 0.0;
    if (v < f.n_verts) {
        const long long idx = (long long)ch * f.n_verts + v;
        const double ap = alpha * p[idx];
        const double aq = alpha * f.q[idx];
        const double xv = f.x[idx] + ap;
        const double rv = f.r[idx] - aq;
        const double zv = rv / f.diag[v];
        f.x[idx] = xv; f.r[idx] = rv; f.z[idx] = zv;
        rz = rv * zv; rr = rv * rv;
    }
    const size_t slot = (size_t)ch * f.n_tiles + blockIdx.x, q = (size_t)f.C * f.n_tiles;
    const double a = fit_block_sum(rz, sh);
    if (threadIdx.x == 0) f.part[q + slot] = a;
    const double b = fit_block_sum(rr, sh);
    if (threadIdx.x == 0) f.part[2 * q + slot] = b;
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_beta_kernel(FitSolve f) {
    __shared__ double sh[FIT_BLOCK];
    const int ch = blockIdx.x;
    if (f.st[ch].stop) return;      // the whole workgroup
    const size_t q = (size_t)f.C * f.n_tiles;
    const double rz = fit_tile_sum(f.part + q + (size_t)ch * f.n_tiles, f.n_tiles, sh), rr = fit_tile_sum(f.part + 2 * q + (size_t)ch * f.n_tiles, f.n_tiles, sh);
    if (threadIdx.x != 0) return;
    FitState s = f.st[ch];
    s.iters += 1;
    if (!(fit_finite(rz) && fit_finite(rr))) { s.stop = FIT_STOP_NAN; s.relres = rr - rr + (rz - rz); }
    else {
        const double nr = sqrt(rr), nb = sqrt(s.bb);
        s.relres = nr / nb;
        if (nr <= f.tol * nb) s.stop = FIT_STOP_CONVERGED;
        s.beta = rz / s.rz;
        s.rz = rz;
    }
    f.st[ch] = s;
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_store_kernel(FitSolve f, float* __restrict__ out, FitInfo* __restrict__ info) {
    const int v = blockIdx.x * FIT_BLOCK + threadIdx.x, ch = blockIdx.y;
    const FitState s = f.st[ch];
    if (info && v == 0) { info[ch].iters = s.iters; info[ch].stop = s.stop; info[ch].relres = s.relres; }
    if (v >= f.n_verts) return;
    out[(long long)v * f.C + ch] = s.stop == FIT_STOP_NAN ? __builtin_nanf("") : s.stop == FIT_STOP_ZERO ? 0.0f : (float)f.x[(long long)ch * f.n_verts + v];
}

// ---- normals ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fit_face_raw(const int* __restrict__ vert, const float* __restrict__ verts, int f, double* n) {
    const float *a = verts + 3ll * vert[3 * f], *b = verts + 3ll * vert[3 * f + 1], *c = verts + 3ll * vert[3 * f + 2];
    fit_face_normal_raw(a, b, c, n);
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_face_normals_kernel(const int* __restrict__ vert, int n_faces, const float* __restrict__ verts,
                                                                    float* __restrict__ fn, float* __restrict__ area) {
    const int f = blockIdx.x * FIT_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    if (fn) {
        double n[3];
        fit_face_raw(vert, verts, f, n);
        fit_face_normal(n, fn + 3ll * f);
    }
    if (area) area[f] = fit_face_area(verts + 3ll * vert[3 * f], verts + 3ll * vert[3 * f + 1], verts + 3ll * vert[3 * f + 2]);
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_vert_normals_kernel(const int* __restrict__ vert, const int* __restrict__ out_start,
                                                                    const int* __restrict__ out_he, int n_verts, const float* __restrict__ verts,
                                                                    float* __restrict__ vn) {
    const int v = blockIdx.x * FIT_BLOCK + threadIdx.x;
    if (v >= n_verts) return;
    double sum[3] = {0.0, 0.0, 0.0};
    for (int k = out_start[v]; k < out_start[v + 1]; ++k) {
        double n[3];
        fit_face_raw(vert, verts, out_he[k] / 3, n);
        for (int i = 0; i < 3; ++i) sum[i] = sum[i] + n[i];
    }
    fit_vert_normal(sum, vn + 3ll * v);
}

// ---- ICP residual -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FIT_BLOCK) void icp_rows_kernel(IcpJob j) {
    __shared__ double sh[FIT_BLOCK];
    const int i = blockIdx.x * FIT_BLOCK + threadIdx.x;
    double sq = 0.0, cnt = 0.0;
    if (i < j.n) {
        const float* p = j.pts + 3ll * i;
        const float* c = j.closest + 3ll * i;
        const int f = j.face[i];
        bool keep = f >= 0 && f < j.n_faces && fit_finite((double)p[0]) && fit_finite((double)p[1]) && fit_finite((double)p[2]);
        keep = keep && fit_icp_keep(j.d2[i], j.dist_th, j.face_normals + 3ll * f, j.pt_normals + 3ll * i, j.angle_th);
        double d[3] = {0.0, 0.0, 0.0};
        if (keep) {
            for (int k = 0; k < 3; ++k) d[k] = (double)p[k] - (double)c[k];
            sq = fit_dot(d, d);
            cnt = 1.0;
        }
        j.keep[i] = keep;
    }
    const double a = fit_block_sum(sq, sh);
    if (threadIdx.x == 0) j.part[blockIdx.x] = a;
    const double b = fit_block_sum(cnt, sh);
    if (threadIdx.x == 0) j.part[j.n_tiles + blockIdx.x] = b;
}

__global__ __launch_bounds__(FIT_BLOCK) void icp_sums_kernel(const double* __restrict__ part, int n_tiles, double* __restrict__ sums) {
    __shared__ double sh[FIT_BLOCK];
    const double sq = fit_tile_sum(part, n_tiles, sh), cnt = fit_tile_sum(part + n_tiles, n_tiles, sh);
    if (threadIdx.x == 0) { sums[0] = sq; sums[1] = cnt; }
}

__global__ __launch_bounds__(FIT_BLOCK) void icp_grad_kernel(IcpJob j, const double* __restrict__ sums, float* __restrict__ grad) {
    const long long idx = (long long)blockIdx.x * FIT_BLOCK + threadIdx.x;
    if (idx >= 3ll * j.n) return;
    const int i = (int)(idx / 3);
    const double count = sums[1];
    float g = 0.0f;
    if (j.keep[i] && count > 0.0) g = fit_icp_grad((double)j.pts[idx] - (double)j.closest[idx], count);
    grad[idx] = g;
}

// ---- AdamUniform ------------------------------------------------------------------------------------------------------------------
// max |grad| as the maximum of the bit patterns with the sign cleared: the order of the floats, NaN above all; integer maxima only
__global__ __launch_bounds__(FIT_BLOCK) void adam_max_kernel(const float* __restrict__ grad, long long n, const float* __restrict__ g2, unsigned* __restrict__ scratch) {
    __shared__ unsigned sh[FIT_BLOCK];
    const long long stride = (long long)gridDim.x * FIT_BLOCK;
    unsigned m = 0;
    for (long long i = (long long)blockIdx.x * FIT_BLOCK + threadIdx.x; i < n; i += stride) {
        const unsigned b = __float_as_uint(grad[i]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int s = FIT_BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] > sh[threadIdx.x + s] ? sh[threadIdx.x] : sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(scratch, sh[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) scratch[1] = __float_as_uint(*g2);      // the state the update reads, while it writes the new one
}

__global__ __launch_bounds__(FIT_BLOCK) void adam_update_kernel(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ g1, float* __restrict__ g2,
                                                               long long n, const unsigned* __restrict__ scratch, double lr, double b1, double b2, double c1,
                                                               double c2) {
    const long long i = (long long)blockIdx.x * FIT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double m = (double)__uint_as_float(scratch[0]);
    const float g2n = fit_adam_moment(__uint_as_float(scratch[1]), m * m, b2);
    const float g1n = fit_adam_moment(g1[i], (double)grad[i], b1);
    g1[i] = g1n;
    param[i] = fit_adam_param(param[i], g1n, g2n, lr, c1, c2);
    if (i == 0) *g2 = g2n;
}

}  // namespace

void launch_fit_apply(const TopoView& t, const float* x, int C, double lambda, float* out, hipStream_t s) {
    const long long total = (long long)t.n_verts * C;
    if (total == 0) return;
    hipLaunchKernelGGL(fit_apply_kernel, dim3(blocks(total, FIT_BLOCK)), dim3(FIT_BLOCK), 0, s, t.nbr_start, t.nbr, total, C, x, lambda, out);
}

// n_verts >= 1
void launch_fit_solve(const FitSolve& f, int max_iter, float* out, FitInfo* info, hipStream_t s) {
    const dim3 grid(f.n_tiles, f.C), block(FIT_BLOCK), one(f.C), chans(FIT_BLOCK);      // `one`: one workgroup per channel
    hipLaunchKernelGGL(fit_init_kernel, grid, block, 0, s, f);
    hipLaunchKernelGGL(fit_start_kernel, one, chans, 0, s, f);
    for (int k = 0; k < max_iter; ++k) {
        const double* p_old = k & 1 ? f.p1 : f.p0;
        double* p_new = k & 1 ? f.p0 : f.p1;
        hipLaunchKernelGGL(fit_q_kernel, grid, block, 0, s, f, p_old, p_new);
        hipLaunchKernelGGL(fit_alpha_kernel, one, chans, 0, s, f);
        hipLaunchKernelGGL(fit_update_kernel, grid, block, 0, s, f, (const double*)p_new);
        hipLaunchKernelGGL(fit_beta_kernel, one, chans, 0, s, f);
    }
    hipLaunchKernelGGL(fit_store_kernel, grid, block, 0, s, f, out, info);
}

void launch_mesh_normals(const TopoView& t, const float* verts, float* fn, float* area, float* vn, hipStream_t s) {
    if ((fn || area) && t.n_faces > 0)
        hipLaunchKernelGGL(fit_face_normals_kernel, dim3(blocks(t.n_faces, FIT_BLOCK)), dim3(FIT_BLOCK), 0, s, t.vert, t.n_faces, verts, fn, area);
    if (vn && t.n_verts > 0)
        hipLaunchKernelGGL(fit_vert_normals_kernel, dim3(blocks(t.n_verts, FIT_BLOCK)), dim3(FIT_BLOCK), 0, s, t.vert, t.out_start, t.out_he, t.n_verts, verts, vn);
}

// n >= 1
void launch_icp_residual(const IcpJob& j, double* sums, float* grad, hipStream_t s) {
    hipLaunchKernelGGL(icp_rows_kernel, dim3(j.n_tiles), dim3(FIT_BLOCK), 0, s, j);
    hipLaunchKernelGGL(icp_sums_kernel, dim3(1), dim3(FIT_BLOCK), 0, s, (const double*)j.part, j.n_tiles, sums);
    if (grad) hipLaunchKernelGGL(icp_grad_kernel, dim3(blocks(3ll * j.n, FIT_BLOCK)), dim3(FIT_BLOCK), 0, s, j, (const double*)sums, grad);
}

// n >= 1; scratch: 2 words, the first zero on entry
void launch_adam_uniform(float* param, const float* grad, float* g1, float* g2, long long n, unsigned* scratch, double lr, double b1, double b2, double c1,
                         double c2, hipStream_t s) {
    const int nb = blocks(n, FIT_BLOCK);
    hipLaunchKernelGGL(adam_max_kernel, dim3(nb < 1024 ? nb : 1024), dim3(FIT_BLOCK), 0, s, grad, n, (const float*)g2, scratch);
    hipLaunchKernelGGL(adam_update_kernel, dim3(nb), dim3(FIT_BLOCK), 0, s, param, grad, g1, g2, n, (const unsigned*)scratch, lr, b1, b2, c1, c2);
}

// Gaussian-histogram entropy of an n x 3 sample (albedo) with its gradient: the sparsity regulariser of the relighting stage.
//
//   reference: gaussian_entropy / gaussian_histogram     lib/utils/loss_utils.py:51-76 (under torch autograd)
//              its use                                    lib/train/trainers/relight_trainer.py:70-81
//
// Per channel c, with N rows, 15 bins on [0, 1] (centres mu_b = (b + 0.5) / 15, delta = 1 / 15):
//     m = mean(x),  s = sum (x - m)^2 / (N - 1)            the VARIANCE is the kernel width: the reference's quirk, kept
//     k_nb = exp(-0.5 ((x_n - mu_b) / s)^2) / (s sqrt(2 pi)) * delta,   h_b = sum_n k_nb,   S = sum_b h_b
//     p_b = h_b / S + 1e-6,   E_c = -sum_b p_b log p_b,   E = sum_c E_c
//     q_b = -(log p_b + 1),   g_b = (q_b - sum_b' q_b' h_b' / S) / S,   T_b = sum_n k_nb ((x_n - mu_b)^2 / s^3 - 1 / s)
//     dE/dx_n = sum_b g_b k_nb (-(x_n - mu_b) / s^2) + (sum_b g_b T_b) 2 (x_n - m) / (N - 1)
// (the second term is the path through s = var(x)).  A channel with S <= 1e-6, s == 0 or a non-finite s contributes 0 and an exactly zero
// gradient (include/relightableavatar.h: where the reference's autograd returns NaN).
//
// Passes, every one a launch whose grid depends on n alone:
//     sums -> [mean] centred squares -> [variance] h, T (15 x 3 x 2 sums) -> one-workgroup finalisation (E, g, the variance path's factor)
//     -> per-element gradient.
// The bracketed reductions are done by the consuming pass itself (three values per slab).  No float atomics: every workgroup writes its
// partial sums to its own slab and the consumer adds the slabs in slab order, so two identical calls are bit-identical.
// Arithmetic: x is read and d_x written as fp32; everything between is double.  dE/ds weighs a relative error of s with
// ((x - mu) / s)^2 — up to ~170 before the kernel underflows — so fp32 moments would cost two digits of the gradient on a narrow
// distribution; the volume is small (45 exponentials per row and pass), nowhere near the fp64 rate of the part.
#include "ra_kernels.hpp"

namespace {

constexpr int EN_T = 256;                     // threads per workgroup
constexpr int EN_ROWS = 1024;                 // rows per workgroup the grid is sized for
constexpr int EN_BINS = 15;
constexpr int EN_HT = 2 * EN_BINS;            // h | T of one channel
// scratch (doubles): [moments: grid x 3][squares: grid x 3][ht: grid x 3 x 30][params: 3 x EN_PARAMS]
constexpr int EN_PARAMS = 4 + EN_BINS;        // valid, m, s, variance-path factor, g_b

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the workgroup's sum of NV per-thread values -> out[0..NV) (fixed tree: lanes by butterfly, then the four waves in order)
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* lds, double* out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double w = wave_sum(v[k]);
        if (lane == 0) lds[wave * NV + k] = w;
    }
    __syncthreads();
    if (tid < NV) out[tid] = ((lds[tid] + lds[NV + tid]) + lds[2 * NV + tid]) + lds[3 * NV + tid];
    __syncthreads();
}

// sum of the slabs' value c in slab order (c < 3); every thread that calls it gets the same bits
__device__ __forceinline__ double slab_sum3(const double* slabs, int nslabs, int c) {
    double a = 0.0;
    for (int g = 0; g < nslabs; ++g) a += slabs[3 * g + c];
    return a;
}

__global__ __launch_bounds__(EN_T) void entropy_sums_kernel(const float* __restrict__ x, int n, double* __restrict__ slabs) {
    __shared__ double lds[4 * 3];
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = blockIdx.x * EN_T + threadIdx.x; i < n; i += gridDim.x * EN_T) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] += (double)x[3 * (size_t)i + c];
    }
    block_sum<3>(v, lds, slabs + 3 * blockIdx.x);
}

__global__ __launch_bounds__(EN_T) void entropy_squares_kernel(const float* __restrict__ x, int n, const double* __restrict__ sums, double* __restrict__ slabs) {
    __shared__ double lds[4 * 3];
    double m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) m[c] = slab_sum3(sums, gridDim.x, c) / (double)n;
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = blockIdx.x * EN_T + threadIdx.x; i < n; i += gridDim.x * EN_T) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { const double d = (double)x[3 * (size_t)i + c] - m[c]; v[c] += d * d; }
    }
    block_sum<3>(v, lds, slabs + 3 * blockIdx.x);
}

__device__ __forceinline__ bool width_ok(double s) { return s > 0.0 && s <= 1.0e300; }      // false for NaN too

__global__ __launch_bounds__(EN_T) void entropy_hist_kernel(const float* __restrict__ x, int n, const double* __restrict__ squares, double* __restrict__ slabs) {
    __shared__ double lds[4 * EN_HT];
    for (int c = 0; c < 3; ++c) {
        const double s = slab_sum3(squares, gridDim.x, c) / (double)(n - 1);
        double v[EN_HT];
#pragma unroll
        for (int k = 0; k < EN_HT; ++k) v[k] = 0.0;
        if (width_ok(s)) {
            const double inv_s = 1.0 / s, norm = (1.0 / EN_BINS) / (s * 2.5066282746310002), inv_s3 = inv_s * inv_s * inv_s;
            for (int i = blockIdx.x * EN_T + threadIdx.x; i < n; i += gridDim.x * EN_T) {
                const double xv = (double)x[3 * (size_t)i + c];
#pragma unroll
                for (int b = 0; b < EN_BINS; ++b) {
                    const double d = xv - (b + 0.5) / EN_BINS, z = d * inv_s;
                    const double k = exp(-0.5 * z * z) * norm;
                    if (k > 0.0) {          // an underflowed kernel value must not meet an overflowed d^2 / s^3
                        v[b] += k;
                        v[EN_BINS + b] += k * (d * d * inv_s3 - inv_s);
                    }
                }
            }
        }
        block_sum<EN_HT>(v, lds, slabs + ((size_t)blockIdx.x * 3 + c) * EN_HT);
    }
}

// one workgroup: threads 0..2 finish one channel each, thread 0 adds the three entropies in channel order
__global__ __launch_bounds__(64) void entropy_finish_kernel(int n, int nslabs, const double* __restrict__ sums, const double* __restrict__ squares,
                                                             const double* __restrict__ ht, double* __restrict__ params, float* __restrict__ value) {
    __shared__ double ec[3];
    const int c = threadIdx.x;
    if (c < 3) {
        const double m = slab_sum3(sums, nslabs, c) / (double)n;
        const double s = slab_sum3(squares, nslabs, c) / (double)(n - 1);
        double h[EN_BINS], T[EN_BINS];
        for (int b = 0; b < EN_BINS; ++b) {
            double a = 0.0, t = 0.0;
            for (int g = 0; g < nslabs; ++g) {
                const double* p = ht + ((size_t)g * 3 + c) * EN_HT;
                a += p[b];
                t += p[EN_BINS + b];
            }
            h[b] = a; T[b] = t;
        }
        double S = 0.0;
        for (int b = 0; b < EN_BINS; ++b) S += h[b];
        double* P = params + c * EN_PARAMS;
        const bool valid = width_ok(s) && S > 1e-6 && S <= 1.0e300;
        double E = 0.0, G = 0.0;
        if (valid) {
            double q[EN_BINS], qh = 0.0;
            for (int b = 0; b < EN_BINS; ++b) {
                const double p = h[b] / S + 1e-6, lp = log(p);
                E -= p * lp;
                q[b] = -(lp + 1.0);
                qh += q[b] * h[b];
            }
            qh /= S;
            for (int b = 0; b < EN_BINS; ++b) {
                const double g = (q[b] - qh) / S;
                P[4 + b] = g;
                G += g * T[b];
            }
        } else {
            for (int b = 0; b < EN_BINS; ++b) P[4 + b] = 0.0;
        }
        P[0] = valid ? 1.0 : 0.0;
        P[1] = m;
        P[2] = s;
        P[3] = valid ? G * 2.0 / (double)(n - 1) : 0.0;
        ec[c] = E;
    }
    __syncthreads();
    if (threadIdx.x == 0) *value = (float)((ec[0] + ec[1]) + ec[2]);
}

__global__ __launch_bounds__(EN_T) void entropy_grad_kernel(const float* __restrict__ x, int n, const double* __restrict__ params, const float* __restrict__ d_value,
                                                             float* __restrict__ d_x) {
    const float up = d_value ? *d_value : 1.f;
    for (long long j = (long long)blockIdx.x * EN_T + threadIdx.x; j < 3ll * n; j += (long long)gridDim.x * EN_T) {
        const int c = (int)(j % 3);
        const double* P = params + c * EN_PARAMS;
        float out = 0.f;                      // a degenerate channel: exactly zero, whatever the upstream factor
        if (P[0] != 0.0) {
            const double m = P[1], s = P[2], inv_s = 1.0 / s, norm = (1.0 / EN_BINS) / (s * 2.5066282746310002);
            const double xv = (double)x[j];
            double a = 0.0;
#pragma unroll
            for (int b = 0; b < EN_BINS; ++b) {
                const double d = xv - (b + 0.5) / EN_BINS, z = d * inv_s;
                const double k = exp(-0.5 * z * z) * norm;
                if (k > 0.0) a -= P[4 + b] * k * d;
            }
            out = (float)(a * inv_s * inv_s + P[3] * (xv - m)) * up;      // the last operation: an fp32 product with the upstream scalar
        }
        d_x[j] = out;
    }
}

}  // namespace

int entropy_grid(int n) {
    const int g = (n + EN_ROWS - 1) / EN_ROWS;
    return g < 1 ? 1 : (g < ENTROPY_MAX_GRID ? g : ENTROPY_MAX_GRID);
}

size_t entropy_scratch_doubles(int n) { return (size_t)entropy_grid(n) * (3 + 3 + 3 * EN_HT) + 3 * EN_PARAMS; }

void launch_gaussian_entropy(const float* x, int n, const float* d_value, float* value, float* d_x, double* scratch, hipStream_t s) {
    const int grid = entropy_grid(n);
    double* sums = scratch;
    double* squares = sums + (size_t)grid * 3;
    double* ht = squares + (size_t)grid * 3;
    double* params = ht + (size_t)grid * 3 * EN_HT;
    hipLaunchKernelGGL(entropy_sums_kernel, dim3(grid), dim3(EN_T), 0, s, x, n, sums);
    hipLaunchKernelGGL(entropy_squares_kernel, dim3(grid), dim3(EN_T), 0, s, x, n, (const double*)sums, squares);
    hipLaunchKernelGGL(entropy_hist_kernel, dim3(grid), dim3(EN_T), 0, s, x, n, (const double*)squares, ht);
    hipLaunchKernelGGL(entropy_finish_kernel, dim3(1), dim3(64), 0, s, n, grid, (const double*)sums, (const double*)squares, (const double*)ht, params, value);
    if (d_x) {
        const long long work = (3ll * n + EN_T - 1) / EN_T;
        const int ggrid = (int)(work < 1024 ? work : 1024);
        hipLaunchKernelGGL(entropy_grad_kernel, dim3(ggrid), dim3(EN_T), 0, s, x, n, (const double*)params, d_value, d_x);
    }
}

// MSE, PSNR and SSIM of one image pair: the reference's evaluator on the device.
//
//   reference: Evaluator.evaluate / psnr_metric / ssim_metric      lib/evaluators/base_evaluator.py:26-48, 71-104
//              skimage.metrics.structural_similarity(pred, gt, channel_axis=-1, data_range=1) at its defaults
//
// The two images are pred / gt (P x 3 fp32): either all H*W pixels, or a ray list with the flat pixel index of every ray; a pixel no ray
// covers has bg in both images (:79-85).  The assembled image is never built: fetch(r, c) reads either layout, the ray list through an
// inverse index (pixel -> ray, -1: background) the call builds in scratch.
//
// SSIM, per channel and per 7 x 7 window that lies inside the rectangle (the image, or with crop_to_mask the bounding rectangle of the
// nonzero mask pixels, :32-39), NP = 49:
//     ux, uy, uxx, uyy, uxy = window means of x, y, x^2, y^2, xy;   vx = NP / (NP - 1) (uxx - ux^2), vy, vxy likewise
//     S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),   C1 = (0.01 R)^2, C2 = (0.03 R)^2
// and the value is the mean of S over the (h - 6)(w - 6) windows and the 3 channels: skimage's uniform_filter + crop of 3 border pixels
// keeps exactly the windows that do not touch the border, so its reflect padding never reaches the result.
//
// Arithmetic: the inputs are fp32, everything after them is double.  The moments of a window are taken of x - xc, y - yc (xc, yc: the
// window's centre pixel; the differences of two fp32 values are exact in double): the variances do not depend on the shift, and
// uxx - ux^2 no longer cancels the seven digits it does on a smooth image.  vx, vy and vxy come out of ONE function, and the four
// factors of S are formed without contraction, so identical images give numerator == denominator bit for bit and S == 1.
//
// Launches (grids depend on H, W alone):
//     prep     inverse index := -1, rectangle := the image (or, for crop_to_mask, the empty rectangle)
//     scatter  inverse index of the ray list                                      [ray list only]
//     pixels   per 2048 pixels in pixel order: the sum of (x - y)^2 -> one partial; the mask's rectangle by integer min / max atomics
//     ssim     per 32 x 32 tile of windows, anchored at the RECTANGLE's corner: x, y with the 6 extra rows and columns in LDS -> one partial
//     finish   partials added in index order (ssim: every tile row in order, then the rows in order) -> out[0..4)
// No float atomics.  Tiles beyond the rectangle write an exact 0, so cropping to a mask and handing in the cropped arrays add the same
// numbers in the same order; the pixel sums run in pixel order, so the order of the rays does not matter.
#include "ra_kernels.hpp"
#include "ra_fetch.hpp"      // Images, fetch, pair_prep_kernel, pair_scatter_kernel
#include <algorithm>
#include <climits>

namespace {

constexpr int MT_T = 256;                     // threads per workgroup
constexpr int MT_TILE = 32;                   // windows per tile side
constexpr int MT_WIN = 7;
constexpr int MT_LD = MT_TILE + MT_WIN - 1;   // pixels per tile side: 38
constexpr int MT_NP = MT_WIN * MT_WIN;
constexpr int MT_PIX = 2048;                  // pixels per workgroup of the pixel pass

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the workgroup's sum (fixed tree: lanes by butterfly, then the four waves in order); valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* lds) {
    const int tid = threadIdx.x;
    const double w = wave_sum(v);
    if ((tid & 63) == 0) lds[tid >> 6] = w;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__global__ __launch_bounds__(MT_T) void metrics_pixel_kernel(Images im, int HW, const unsigned char* __restrict__ mask, int* __restrict__ rect,
                                                              double* __restrict__ partial) {
    __shared__ double lds[4];
    double v = 0.0;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    const int base = blockIdx.x * MT_PIX;
    for (int j = threadIdx.x; j < MT_PIX; j += MT_T) {
        const int p = base + j;
        if (p >= HW) break;
        const int r = p / im.W, c = p - r * im.W;
        float x[3], y[3];
        fetch(im, r, c, x, y);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { const double d = (double)x[ch] - (double)y[ch]; v = fma(d, d, v); }
        if (mask && mask[p]) { x0 = min(x0, c); y0 = min(y0, r); x1 = max(x1, c); y1 = max(y1, r); }
    }
    const double s = block_sum(v, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
    if (mask) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            x0 = min(x0, __shfl_xor(x0, o)); y0 = min(y0, __shfl_xor(y0, o));
            x1 = max(x1, __shfl_xor(x1, o)); y1 = max(y1, __shfl_xor(y1, o));
        }
        if ((threadIdx.x & 63) == 0 && x1 >= 0) {
            atomicMin(rect + 0, x0); atomicMin(rect + 1, y0);
            atomicMax(rect + 2, x1); atomicMax(rect + 3, y1);
        }
    }
}

// NP / (NP - 1) (mean(ab) - mean(a) mean(b)): the one expression of vx, vy and vxy
__device__ __forceinline__ double sample_cov(double sab, double ma, double mb) {
#pragma clang fp contract(off)
    return ((double)MT_NP / (MT_NP - 1)) * (sab * (1.0 / MT_NP) - ma * mb);
}

__device__ __forceinline__ double ssim_of(double ux, double uy, double vx, double vy, double vxy, double c1, double c2) {
#pragma clang fp contract(off)
    const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2;
    const double b1 = (ux * ux + uy * uy) + c1, b2 = (vx + vy) + c2;
    return (a1 * a2) / (b1 * b2);
}

__global__ __launch_bounds__(MT_T) void metrics_ssim_kernel(Images im, const int* __restrict__ rect, double c1, double c2, double* __restrict__ partial) {
    __shared__ float X[3][MT_LD * MT_LD], Y[3][MT_LD * MT_LD];
    __shared__ double lds[4];
    const int tile = blockIdx.y * gridDim.x + blockIdx.x;
    const int x0 = rect[0], y0 = rect[1], x1 = rect[2], y1 = rect[3];
    // the rectangle holds no window (empty mask: x0 = INT_MAX, x1 = -1), or this tile starts behind the last one: an exact 0
    const long long r0l = (long long)y0 + (long long)blockIdx.y * MT_TILE, c0l = (long long)x0 + (long long)blockIdx.x * MT_TILE;
    if (r0l + (MT_WIN - 1) > y1 || c0l + (MT_WIN - 1) > x1) {
        if (threadIdx.x == 0) partial[tile] = 0.0;
        return;
    }
    const int r0 = (int)r0l, c0 = (int)c0l;
    for (int i = threadIdx.x; i < MT_LD * MT_LD; i += MT_T) {
        const int r = r0 + i / MT_LD, c = c0 + i % MT_LD;
        float x[3] = {0.f, 0.f, 0.f}, y[3] = {0.f, 0.f, 0.f};       // beyond the rectangle: read by no counted window
        if (r <= y1 && c <= x1) fetch(im, r, c, x, y);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { X[ch][i] = x[ch]; Y[ch][i] = y[ch]; }
    }
    __syncthreads();
    const int lx = threadIdx.x & (MT_TILE - 1), ly0 = threadIdx.x / MT_TILE;
    double acc = 0.0;
#pragma unroll 1
    for (int ly = ly0; ly < MT_TILE; ly += MT_T / MT_TILE) {
        if (r0 + ly + (MT_WIN - 1) > y1 || c0 + lx + (MT_WIN - 1) > x1) continue;
#pragma unroll 1
        for (int ch = 0; ch < 3; ++ch) {
            const float* xs = &X[ch][ly * MT_LD + lx];
            const float* ys = &Y[ch][ly * MT_LD + lx];
            const double xc = (double)xs[3 * MT_LD + 3], yc = (double)ys[3 * MT_LD + 3];
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
            for (int dy = 0; dy < MT_WIN; ++dy) {
#pragma unroll
                for (int dx = 0; dx < MT_WIN; ++dx) {
                    const double a = (double)xs[dy * MT_LD + dx] - xc, b = (double)ys[dy * MT_LD + dx] - yc;
                    sx += a;
                    sy += b;
                    sxx = fma(a, a, sxx);
                    syy = fma(b, b, syy);
                    sxy = fma(a, b, sxy);
                }
            }
            const double mx = sx * (1.0 / MT_NP), my = sy * (1.0 / MT_NP);
            acc += ssim_of(xc + mx, yc + my, sample_cov(sxx, mx, mx), sample_cov(syy, my, my), sample_cov(sxy, mx, my), c1, c2);
        }
    }
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) partial[tile] = s;
}

// one workgroup.  mse: MT_T contiguous runs of partials, each in order, then the runs in order.  ssim: every tile row in order, then the rows.
__global__ __launch_bounds__(MT_T) void metrics_finish_kernel(const double* __restrict__ pmse, int n_mse, const double* __restrict__ pssim, int ntx, int nty,
                                                               double* __restrict__ rows, const int* __restrict__ rect, double mse_count,
                                                               double* __restrict__ out) {
    __shared__ double run[MT_T];
    const int per = (n_mse + MT_T - 1) / MT_T;
    double a = 0.0;
    for (int g = threadIdx.x * per; g < n_mse && g < (threadIdx.x + 1) * per; ++g) a += pmse[g];
    run[threadIdx.x] = a;
    for (int ty = threadIdx.x; ty < nty; ty += MT_T) {
        double b = 0.0;
        for (int tx = 0; tx < ntx; ++tx) b += pssim[ty * ntx + tx];
        rows[ty] = b;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sq = 0.0;
    for (int t = 0; t < MT_T; ++t) sq += run[t];
    const double mse = sq / mse_count;
    out[0] = mse;
    out[1] = mse == 0.0 ? (double)INFINITY : -10.0 * log10(mse);
    const long long w = (long long)rect[2] - rect[0] + 1, h = (long long)rect[3] - rect[1] + 1;
    const long long n = (w >= MT_WIN && h >= MT_WIN) ? (w - (MT_WIN - 1)) * (h - (MT_WIN - 1)) : 0;
    double ss = 0.0;
    for (int ty = 0; ty < nty; ++ty) ss += rows[ty];
    out[2] = n > 0 ? ss / (3.0 * (double)n) : (double)NAN;      // narrower or lower than the window: skimage raises
    out[3] = (double)n;
}

inline size_t align_up(size_t v) { return (v + 31) & ~(size_t)31; }
inline int mse_grid(long long hw) { return (int)((hw + MT_PIX - 1) / MT_PIX); }
inline int tiles(int n) { return (n + MT_TILE - 1) / MT_TILE; }

}  // namespace

size_t metrics_scratch_bytes(int H, int W, bool ray_list) {
    const long long hw = (long long)H * W;
    return 32 + align_up(sizeof(double) * ((size_t)mse_grid(hw) + (size_t)tiles(W) * tiles(H) + tiles(H))) + (ray_list ? sizeof(int) * (size_t)hw : 0);
}

void launch_image_metrics(const MetricsIO& io, hipStream_t s) {
    const int HW = io.H * io.W, n_mse = mse_grid(HW), ntx = tiles(io.W), nty = tiles(io.H);
    const bool ray_list = io.pix != nullptr;
    char* base = (char*)io.scratch;
    int* rect = (int*)base;
    double* pmse = (double*)(base + 32);
    double* pssim = pmse + n_mse;
    double* rows = pssim + (size_t)ntx * nty;
    int* inv = ray_list ? (int*)(base + 32 + align_up(sizeof(double) * ((size_t)n_mse + (size_t)ntx * nty + nty))) : nullptr;
    const Images im{io.pred, io.gt, inv, io.bg, io.W};
    const int fill_grid = ray_list ? std::min(1024, (HW + FETCH_T - 1) / FETCH_T) : 1;
    hipLaunchKernelGGL(pair_prep_kernel, dim3(fill_grid), dim3(FETCH_T), 0, s, inv, ray_list ? HW : 0, rect, io.H, io.W, io.crop_to_mask);
    if (ray_list && io.P > 0)
        hipLaunchKernelGGL(pair_scatter_kernel, dim3(std::min(1024, (io.P + FETCH_T - 1) / FETCH_T)), dim3(FETCH_T), 0, s, io.pix, io.P, HW, inv);
    hipLaunchKernelGGL(metrics_pixel_kernel, dim3(n_mse), dim3(MT_T), 0, s, im, HW, io.crop_to_mask ? io.mask : nullptr, rect, pmse);
    const double c1 = (0.01 * (double)io.data_range) * (0.01 * (double)io.data_range), c2 = (0.03 * (double)io.data_range) * (0.03 * (double)io.data_range);
    hipLaunchKernelGGL(metrics_ssim_kernel, dim3(ntx, nty), dim3(MT_T), 0, s, im, (const int*)rect, c1, c2, pssim);
    const double mse_count = 3.0 * (double)(io.mse_over_rays ? io.P : HW);
    hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(MT_T), 0, s, (const double*)pmse, n_mse, (const double*)pssim, ntx, nty, rows,
                       (const int*)rect, mse_count, io.out);
}

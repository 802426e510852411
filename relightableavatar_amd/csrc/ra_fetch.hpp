// The one reader of an image pair in either layout, shared by the evaluator's kernels (ra_metrics.hip, ra_lpips.hip).
//
// pred / gt are P x 3 fp32: all H*W pixels, or a ray list read through an inverse index (pixel -> ray, -1: no ray, the pixel holds bg in
// both images; lib/evaluators/base_evaluator.py:79-85).  The assembled image is never built for its own sake.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>

namespace {

struct Images {
    const float *pred, *gt;
    const int* inv;       // pixel -> ray (-1: no ray), or nullptr: the maps are full images
    float bg;
    int W;
};

// channel values of pixel (r, c) of the two assembled images
__device__ __forceinline__ void fetch(const Images& im, int r, int c, float (&x)[3], float (&y)[3]) {
    long long k = (long long)r * im.W + c;
    if (im.inv) k = im.inv[k];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        x[ch] = k < 0 ? im.bg : im.pred[3 * k + ch];
        y[ch] = k < 0 ? im.bg : im.gt[3 * k + ch];
    }
}

constexpr int FETCH_T = 256;      // threads per workgroup of the two kernels below

// inverse index := -1, rectangle := the image (or, for crop_to_mask, the empty rectangle)
__global__ __launch_bounds__(FETCH_T) void pair_prep_kernel(int* __restrict__ inv, int n_inv, int* __restrict__ rect, int H, int W, int crop) {
    for (int i = blockIdx.x * FETCH_T + threadIdx.x; i < n_inv; i += gridDim.x * FETCH_T) inv[i] = -1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        rect[0] = crop ? INT_MAX : 0;
        rect[1] = crop ? INT_MAX : 0;
        rect[2] = crop ? -1 : W - 1;
        rect[3] = crop ? -1 : H - 1;
    }
}

__global__ __launch_bounds__(FETCH_T) void pair_scatter_kernel(const long long* __restrict__ pix, int P, int HW, int* __restrict__ inv) {
    for (int i = blockIdx.x * FETCH_T + threadIdx.x; i < P; i += gridDim.x * FETCH_T) {
        const long long p = pix[i];
        if ((unsigned long long)p < (unsigned long long)HW) inv[p] = i;      // a pixel outside the image: the ray is dropped
    }
}

}  // namespace

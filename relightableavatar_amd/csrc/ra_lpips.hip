// LPIPS (AlexNet, version 0.1, linear layers on, spatial = False) of one image pair: the fourth metric of the reference's evaluator.
//
//   reference: lpips.LPIPS(verbose=False)(pred, gt) on images in [0, 1] WITHOUT normalize=True      lib/evaluators/base_evaluator.py:19-24, 50-69
//
//   scaling   x = (x - shift) / scale per channel (a division)
//   features  conv 11/4/2 3->64, pool 3/2, conv 5/1/2 64->192, pool 3/2, conv 3/1/1 192->384, 384->256, 256->256; a tap after every ReLU
//   per tap   n = f / (sqrt(sum_c f^2) + 1e-10) for both images, r = mean over positions of sum_c lin[c] (n0 - n1)^2
//   value     r0 + r1 + r2 + r3 + r4
//
// Activations are NHWC and the two images are batched: stage s is one dense (2 * npix_s) x C_s matrix, image 1 behind image 0, so a row
// is one pixel's channel vector (contiguous for the gather of the next convolution and for the channel norm).  The buffers are compact in
// the CROPPED size (h, w), which only the device knows: the assembly kernel writes the cropped, scaled planes at the origin and (h, w) into
// dims[]; every later kernel derives its sizes from there and leaves beyond them.  Every grid is a function of (H, W) alone.
//
// The convolutions are implicit GEMMs on v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulate; every K-sum is one fixed, k-ordered
// blocked sum inside one workgroup — chains of 32 products, added in groups of 8 stages, the groups added in order; no split-K):
// M = output pixels of both images, N = output channels, K = (ky, kx, ci) (ra_lpips_pack.hpp).  A workgroup of 4 waves owns a
// LPIPS_BM x LPIPS_BN = 128 x 64 tile, a wave 64 x 32 of it (two accumulators that share the B operand).  Per K stage of 32 the A tile is
// gathered from the activation planes into LDS (zeros for the padding and beyond K), the B tile is one contiguous copy of the packed
// weights; the next stage's global loads are issued before the MFMAs of the current one.  Bias + ReLU in the epilogue.
//
// Everything after the fp32 features is double; sums are fixed trees (lanes by butterfly, waves and partials in index order): no float
// atomics, two identical calls are bit-identical, (a, b) and (b, a) agree bit for bit ((n0 - n1)^2 is symmetric), identical images give
// exact zeros, and crop_to_mask gives the bits of a call on the cropped arrays (same rows, same tiles, same order).
#include "ra_kernels.hpp"
#include "ra_fetch.hpp"
#include "ra_lpips_pack.hpp"
#include <algorithm>
#include <cmath>

namespace {

constexpr int LP_T = 256;                      // threads per workgroup
constexpr int LP_LDA = LPIPS_BM + 4;           // LDS row strides (floats): k-major tiles, rows 16-byte aligned
constexpr int LP_LDB = LPIPS_BN + 4;
constexpr int LP_GROUP = 8;                    // K stages per group of the blocked summation
constexpr int LP_POS = 16;                     // positions per workgroup of the tap reduction (4 per wave)
constexpr int LP_MAX_GRID = 4096;              // workgroups of the grid-stride kernels

typedef float f32x16 __attribute__((ext_vector_type(16)));

// side lengths of stage `stage` for the cropped image (h, w): 0 input, 1 conv1, 2 pool1 (= conv2), 3 pool2 (= conv3..5); false: no output
__host__ __device__ __forceinline__ bool stage_size(int h, int w, int stage, int& sh, int& sw) {
    if (h < LPIPS_MIN_SIDE || w < LPIPS_MIN_SIDE) return false;
    sh = h; sw = w;
    if (stage >= 1) { sh = lpips_conv1_side(sh); sw = lpips_conv1_side(sw); }
    if (stage >= 2) { sh = lpips_pool_side(sh); sw = lpips_pool_side(sw); }
    if (stage >= 3) { sh = lpips_pool_side(sh); sw = lpips_pool_side(sw); }
    return true;
}
constexpr int TAP_STAGE[LPIPS_TAPS] = {1, 2, 3, 3, 3};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the bounding rectangle of the mask's nonzero pixels (cv2.boundingRect) by integer min / max atomics
__global__ __launch_bounds__(LP_T) void lpips_rect_kernel(const unsigned char* __restrict__ mask, int HW, int W, int* __restrict__ rect) {
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    for (int p = blockIdx.x * LP_T + threadIdx.x; p < HW; p += gridDim.x * LP_T) {
        if (!mask[p]) continue;
        const int r = p / W, c = p - r * W;
        x0 = min(x0, c); y0 = min(y0, r); x1 = max(x1, c); y1 = max(y1, r);
    }
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

// the cropped, scaled planes of both images at the origin: plane[(img * h * w + r * w + c) * 3 + ch]; dims := (h, w) ((0, 0): empty mask)
__global__ __launch_bounds__(LP_T) void lpips_assemble_kernel(Images im, const int* __restrict__ rect, const float* __restrict__ shift,
                                                               const float* __restrict__ scale, float* __restrict__ plane, int* __restrict__ dims) {
    const int x0 = rect[0], y0 = rect[1];
    const int w = rect[2] >= x0 ? rect[2] - x0 + 1 : 0, h = rect[3] >= y0 ? rect[3] - y0 + 1 : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { dims[0] = h; dims[1] = w; }
    if (h < LPIPS_MIN_SIDE || w < LPIPS_MIN_SIDE) return;      // nothing downstream reads the planes
    const int n = h * w;
    const int i = blockIdx.x * LP_T + threadIdx.x;
    if (i >= n) return;
    const int r = i / w, c = i - r * w;
    float x[3], y[3];
    fetch(im, y0 + r, x0 + c, x, y);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        plane[(size_t)i * 3 + ch] = (x[ch] - shift[ch]) / scale[ch];
        plane[((size_t)n + i) * 3 + ch] = (y[ch] - shift[ch]) / scale[ch];
    }
}

// ---- convolution + bias + ReLU: in (2 * ih * iw) x CIN -> out (2 * oh * ow) x cout --------------------------------------------------
template <int CIN, int KS, int STRIDE, int PAD>
__global__ __launch_bounds__(LP_T) void lpips_conv_kernel(const float* __restrict__ in, const float* __restrict__ wp, const float* __restrict__ bias,
                                                           float* __restrict__ out, const int* __restrict__ dims, int in_stage, int cout) {
    constexpr int K = CIN * KS * KS;
    constexpr int KT = (K + LPIPS_BK - 1) / LPIPS_BK;
    constexpr bool VEC = CIN % LPIPS_BK == 0;          // a K stage lies inside one filter tap: 32 contiguous channels of one input pixel
    __shared__ __attribute__((aligned(16))) float As[LPIPS_BK * LP_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[LPIPS_BK * LP_LDB];
    int ih, iw;
    if (!stage_size(dims[0], dims[1], in_stage, ih, iw)) return;
    const int oh = (ih + 2 * PAD - KS) / STRIDE + 1, ow = (iw + 2 * PAD - KS) / STRIDE + 1;
    const int npix = oh * ow, M = 2 * npix;
    const int m0 = blockIdx.x * LPIPS_BM;
    if (m0 >= M) return;                               // the grid covers the uncropped image
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    // this thread's part of the A gather.  VEC: 4 rows (tid / 8 + 32 i), one float4 of k (tid % 8) each; else: 1 row (tid % 128), 16 k
    constexpr int NROW = VEC ? 4 : 1;
    int iy0[NROW], ix0[NROW];
    size_t base[NROW];
#pragma unroll
    for (int i = 0; i < NROW; ++i) {
        const int m = m0 + (VEC ? (tid >> 3) + 32 * i : (tid & 127));
        const int img = m >= npix ? 1 : 0, p = m - img * npix;
        const int oy = p / ow, ox = p - oy * ow;
        iy0[i] = m < M ? oy * STRIDE - PAD : -(1 << 20);                // a row beyond M: every tap misses, zeros
        ix0[i] = ox * STRIDE - PAD;
        base[i] = (size_t)img * ih * iw;
    }
    const float* wtile = wp + (size_t)blockIdx.y * KT * (LPIPS_BK * LPIPS_BN);

    float4 av[VEC ? 4 : 1];
    float as[VEC ? 1 : 16];
    float4 bv0, bv1;
    auto load_stage = [&](int kt) {
        const int k0 = kt * LPIPS_BK;
        if constexpr (VEC) {
            const int tap = k0 / CIN, c0 = k0 - tap * CIN, ky = tap / KS, kx = tap - ky * KS;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int iy = iy0[i] + ky, ix = ix0[i] + kx;
                av[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if ((unsigned)iy < (unsigned)ih && (unsigned)ix < (unsigned)iw)
                    av[i] = *reinterpret_cast<const float4*>(in + (base[0 + i] + (size_t)iy * iw + ix) * CIN + c0 + 4 * (tid & 7));
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k = k0 + (tid >> 7) * 16 + j;
                const int tap = k / CIN, ci = k - tap * CIN, ky = tap / KS, kx = tap - ky * KS;
                const int iy = iy0[0] + ky, ix = ix0[0] + kx;
                as[j] = 0.f;
                if (k < K && (unsigned)iy < (unsigned)ih && (unsigned)ix < (unsigned)iw) as[j] = in[(base[0] + (size_t)iy * iw + ix) * CIN + ci];
            }
        }
        const float4* wsrc = reinterpret_cast<const float4*>(wtile + (size_t)kt * (LPIPS_BK * LPIPS_BN));
        bv0 = wsrc[tid];
        bv1 = wsrc[tid + LP_T];
    };
    auto store_stage = [&]() {
        if constexpr (VEC) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = (tid >> 3) + 32 * i, k = 4 * (tid & 7);
                As[(k + 0) * LP_LDA + row] = av[i].x;
                As[(k + 1) * LP_LDA + row] = av[i].y;
                As[(k + 2) * LP_LDA + row] = av[i].z;
                As[(k + 3) * LP_LDA + row] = av[i].w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) As[((tid >> 7) * 16 + j) * LP_LDA + (tid & 127)] = as[j];
        }
        // float4 q of the [32][64] tile: row q / 16, columns 4 (q % 16) ..
        *reinterpret_cast<float4*>(&Bs[(tid >> 4) * LP_LDB + 4 * (tid & 15)]) = bv0;
        *reinterpret_cast<float4*>(&Bs[((tid + LP_T) >> 4) * LP_LDB + 4 * (tid & 15)]) = bv1;
    };

    // K is summed in fixed blocks, not as one chain of up to 3456 terms: a stage's 32 products (an MFMA chain), LP_GROUP stages, the groups —
    // every level in index order.  Against the single chain this cuts the rounding error of a deep layer several times at no MFMA more.
    f32x16 acc0, acc1, mid0, mid1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; mid0[r] = 0.f; mid1[r] = 0.f; }
    const int wm = (wv & 1) * 64, wn = (wv >> 1) * 32;
    const int la = wm + (lane & 31), lb = wn + (lane & 31), lk = lane >> 5;      // the MFMA's operand map: A[i = lane & 31][k = lane >> 5]

    load_stage(0);
#pragma unroll 1
    for (int kt = 0; kt < KT; ++kt) {
        store_stage();
        __syncthreads();
        if (kt + 1 < KT) load_stage(kt + 1);
        f32x16 p0, p1;                                  // this stage's 32 products: one MFMA chain from zero
#pragma unroll
        for (int r = 0; r < 16; ++r) { p0[r] = 0.f; p1[r] = 0.f; }
#pragma unroll
        for (int kk = 0; kk < LPIPS_BK / 2; ++kk) {
            const int k = 2 * kk + lk;
            const float b = Bs[k * LP_LDB + lb];
            p0 = __builtin_amdgcn_mfma_f32_32x32x2f32(As[k * LP_LDA + la], b, p0, 0, 0, 0);
            p1 = __builtin_amdgcn_mfma_f32_32x32x2f32(As[k * LP_LDA + la + 32], b, p1, 0, 0, 0);
        }
        mid0 += p0;
        mid1 += p1;
        if ((kt + 1) % LP_GROUP == 0 || kt + 1 == KT) {       // a group of stages is complete (uniform: kt is)
            acc0 += mid0;
            acc1 += mid1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { mid0[r] = 0.f; mid1[r] = 0.f; }
        }
        __syncthreads();
    }

    // C/D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int n = blockIdx.y * LPIPS_BN + lb;
    const float bn = bias[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * lk;
        const int ma = m0 + wm + row, mb = ma + 32;
        if (ma < M) out[(size_t)ma * cout + n] = fmaxf(acc0[r] + bn, 0.f);
        if (mb < M) out[(size_t)mb * cout + n] = fmaxf(acc1[r] + bn, 0.f);
    }
}

// 3 x 3 / stride 2 max pool, no padding, floor: in (2 * ih * iw) x C -> out (2 * oh * ow) x C
__global__ __launch_bounds__(LP_T) void lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out, const int* __restrict__ dims, int in_stage, int C) {
    int ih, iw;
    if (!stage_size(dims[0], dims[1], in_stage, ih, iw)) return;
    const int oh = lpips_pool_side(ih), ow = lpips_pool_side(iw);
    const long long total = 2ll * oh * ow * C;
    for (long long e = (long long)blockIdx.x * LP_T + threadIdx.x; e < total; e += (long long)gridDim.x * LP_T) {
        const int c = (int)(e % C);
        const int m = (int)(e / C);
        const int img = m >= oh * ow ? 1 : 0, p = m - img * oh * ow;
        const int oy = p / ow, ox = p - oy * ow;
        const float* src = in + (((size_t)img * ih + 2 * oy) * iw + 2 * ox) * C + c;
        float v = src[0];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) v = fmaxf(v, src[((size_t)dy * iw + dx) * C]);
        out[e] = v;
    }
}

// one tap: per position both channel norms and sum_c lin[c] (n0 - n1)^2, one double partial per workgroup of LP_POS positions
__global__ __launch_bounds__(LP_T) void lpips_tap_kernel(const float* __restrict__ act, const float* __restrict__ lin, const int* __restrict__ dims,
                                                          int stage, int C, double* __restrict__ partial) {
    __shared__ double lds[4];
    int sh, sw;
    if (!stage_size(dims[0], dims[1], stage, sh, sw)) return;
    const int npix = sh * sw;
    if (blockIdx.x * LP_POS >= npix) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double acc = 0.0;
#pragma unroll 1
    for (int i = 0; i < LP_POS / 4; ++i) {
        const int p = blockIdx.x * LP_POS + wv * (LP_POS / 4) + i;
        if (p >= npix) break;                                           // wave-uniform
        const float* f0 = act + (size_t)p * C;
        const float* f1 = act + ((size_t)npix + p) * C;
        double s0 = 0.0, s1 = 0.0;
        for (int c = lane; c < C; c += 64) {
            const double a = (double)f0[c], b = (double)f1[c];
            s0 = fma(a, a, s0);
            s1 = fma(b, b, s1);
        }
        const double d0 = sqrt(wave_sum(s0)) + 1e-10, d1 = sqrt(wave_sum(s1)) + 1e-10;
        double v = 0.0;
        for (int c = lane; c < C; c += 64) {
            const double t = (double)f0[c] / d0 - (double)f1[c] / d1;
            v = fma((double)lin[c], t * t, v);
        }
        acc += wave_sum(v);
    }
    if (lane == 0) lds[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

struct TapPartials { const double* p[LPIPS_TAPS]; };

// one workgroup: per tap LP_T contiguous runs of partials, each in order, then the runs in order; the mean; out[0] = the sum of the taps
__global__ __launch_bounds__(LP_T) void lpips_finish_kernel(TapPartials tp, const int* __restrict__ dims, int force_nan, double* __restrict__ out) {
    __shared__ double run[LP_T];
    __shared__ double r[LPIPS_TAPS];
    int sh, sw;
    if (force_nan || !stage_size(dims[0], dims[1], 0, sh, sw)) {        // below 31 in a dimension (an empty mask too): torch raises
        if (threadIdx.x < 1 + LPIPS_TAPS) out[threadIdx.x] = (double)NAN;
        return;
    }
    for (int k = 0; k < LPIPS_TAPS; ++k) {
        stage_size(dims[0], dims[1], TAP_STAGE[k], sh, sw);
        const int npix = sh * sw, n = (npix + LP_POS - 1) / LP_POS, per = (n + LP_T - 1) / LP_T;
        double a = 0.0;
        for (int g = threadIdx.x * per; g < n && g < (threadIdx.x + 1) * per; ++g) a += tp.p[k][g];
        run[threadIdx.x] = a;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int t = 0; t < LP_T; ++t) s += run[t];
            r[k] = s / (double)npix;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (((r[0] + r[1]) + r[2]) + r[3]) + r[4];
        for (int k = 0; k < LPIPS_TAPS; ++k) out[1 + k] = r[k];
    }
}

// image 0's rows of one stage, (npix x C) -> (C, h, w)
__global__ __launch_bounds__(LP_T) void lpips_chw_kernel(const float* __restrict__ act, int npix, int C, float* __restrict__ out) {
    const long long total = (long long)npix * C;
    for (long long e = (long long)blockIdx.x * LP_T + threadIdx.x; e < total; e += (long long)gridDim.x * LP_T) {
        const int p = (int)(e / C), c = (int)(e % C);
        out[(size_t)c * npix + p] = act[e];
    }
}

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }
inline int grid_for(long long n) { return (int)std::max(1ll, std::min((long long)LP_MAX_GRID, (n + LP_T - 1) / LP_T)); }

// the scratch of an H x W call: every offset depends on (H, W, ray_list) alone
struct Layout {
    size_t rect, dims, inv, plane, conv[LPIPS_TAPS], pool[2], partial[LPIPS_TAPS], total;
    int npix[4];              // positions per image of the four stages, uncropped
    int tap_grid[LPIPS_TAPS];
};
Layout layout_of(int H, int W, bool ray_list) {
    Layout L{};
    for (int s = 0; s < 4; ++s) {
        int sh = 0, sw = 0;
        L.npix[s] = stage_size(H, W, s, sh, sw) ? sh * sw : 0;
    }
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
    L.rect = take(4 * sizeof(int));
    L.dims = take(2 * sizeof(int));
    L.inv = take(ray_list ? sizeof(int) * (size_t)H * W : 0);
    L.plane = take(sizeof(float) * 2 * (size_t)L.npix[0] * 3);
    for (int k = 0; k < LPIPS_TAPS; ++k) L.conv[k] = take(sizeof(float) * 2 * (size_t)L.npix[TAP_STAGE[k]] * LPIPS_LAYERS[k].cout);
    for (int k = 0; k < 2; ++k) L.pool[k] = take(sizeof(float) * 2 * (size_t)L.npix[2 + k] * LPIPS_LAYERS[k].cout);
    for (int k = 0; k < LPIPS_TAPS; ++k) {
        L.tap_grid[k] = std::max(1, (L.npix[TAP_STAGE[k]] + LP_POS - 1) / LP_POS);
        L.partial[k] = take(sizeof(double) * (size_t)L.tap_grid[k]);
    }
    L.total = o;
    return L;
}

template <int CIN, int KS, int STRIDE, int PAD>
void launch_conv(int layer, const LpipsIO& io, const Layout& L, const float* in, int in_stage, float* out, hipStream_t s) {
    const LpipsLayer& l = LPIPS_LAYERS[layer];
    static_assert(CIN > 0, "");
    const int m_max = 2 * L.npix[TAP_STAGE[layer]];
    hipLaunchKernelGGL((lpips_conv_kernel<CIN, KS, STRIDE, PAD>), dim3((m_max + LPIPS_BM - 1) / LPIPS_BM, l.cout / LPIPS_BN), dim3(LP_T), 0, s,
                       in, io.arena + io.off.conv[layer], io.arena + io.off.bias[layer], out, (const int*)((char*)io.scratch + L.dims), in_stage, l.cout);
}

// assembly + the convolutions up to and including tap `last`
void launch_features(const LpipsIO& io, const Layout& L, int last, hipStream_t s) {
    char* base = (char*)io.scratch;
    const int HW = io.H * io.W;
    const bool ray_list = io.pix != nullptr;
    int* rect = (int*)(base + L.rect);
    int* dims = (int*)(base + L.dims);
    int* inv = ray_list ? (int*)(base + L.inv) : nullptr;
    float* plane = (float*)(base + L.plane);
    float* conv[LPIPS_TAPS];
    for (int k = 0; k < LPIPS_TAPS; ++k) conv[k] = (float*)(base + L.conv[k]);
    float* pool[2] = {(float*)(base + L.pool[0]), (float*)(base + L.pool[1])};
    const Images im{io.pred, io.gt, inv, io.bg, io.W};
    hipLaunchKernelGGL(pair_prep_kernel, dim3(ray_list ? std::min(1024, (HW + FETCH_T - 1) / FETCH_T) : 1), dim3(FETCH_T), 0, s, inv, ray_list ? HW : 0,
                       rect, io.H, io.W, io.crop_to_mask);
    if (ray_list && io.P > 0)
        hipLaunchKernelGGL(pair_scatter_kernel, dim3(std::min(1024, (io.P + FETCH_T - 1) / FETCH_T)), dim3(FETCH_T), 0, s, io.pix, io.P, HW, inv);
    if (io.crop_to_mask) hipLaunchKernelGGL(lpips_rect_kernel, dim3(grid_for(HW)), dim3(LP_T), 0, s, io.mask, HW, io.W, rect);
    hipLaunchKernelGGL(lpips_assemble_kernel, dim3((HW + LP_T - 1) / LP_T), dim3(LP_T), 0, s, im, (const int*)rect, io.arena + io.off.shift,
                       io.arena + io.off.scale, plane, dims);
    launch_conv<3, 11, 4, 2>(0, io, L, plane, 0, conv[0], s);
    if (last < 1) return;
    hipLaunchKernelGGL(lpips_pool_kernel, dim3(grid_for(2ll * L.npix[2] * 64)), dim3(LP_T), 0, s, (const float*)conv[0], pool[0], (const int*)dims, 1, 64);
    launch_conv<64, 5, 1, 2>(1, io, L, pool[0], 2, conv[1], s);
    if (last < 2) return;
    hipLaunchKernelGGL(lpips_pool_kernel, dim3(grid_for(2ll * L.npix[3] * 192)), dim3(LP_T), 0, s, (const float*)conv[1], pool[1], (const int*)dims, 2, 192);
    launch_conv<192, 3, 1, 1>(2, io, L, pool[1], 3, conv[2], s);
    if (last < 3) return;
    launch_conv<384, 3, 1, 1>(3, io, L, conv[2], 3, conv[3], s);
    if (last < 4) return;
    launch_conv<256, 3, 1, 1>(4, io, L, conv[3], 3, conv[4], s);
}

}  // namespace

size_t lpips_scratch_bytes(int H, int W, bool ray_list) { return layout_of(H, W, ray_list).total; }

void launch_lpips(const LpipsIO& io, hipStream_t s) {
    const Layout L = layout_of(io.H, io.W, io.pix != nullptr);
    char* base = (char*)io.scratch;
    TapPartials tp{};
    for (int k = 0; k < LPIPS_TAPS; ++k) tp.p[k] = (const double*)(base + L.partial[k]);
    const int* dims = (const int*)(base + L.dims);
    if (io.H < LPIPS_MIN_SIDE || io.W < LPIPS_MIN_SIDE) {               // no rectangle of this image reaches 31 x 31
        hipLaunchKernelGGL(lpips_finish_kernel, dim3(1), dim3(LP_T), 0, s, tp, dims, 1, io.out);
        return;
    }
    launch_features(io, L, LPIPS_TAPS - 1, s);
    for (int k = 0; k < LPIPS_TAPS; ++k)
        hipLaunchKernelGGL(lpips_tap_kernel, dim3(L.tap_grid[k]), dim3(LP_T), 0, s, (const float*)(base + L.conv[k]), io.arena + io.off.lin[k], dims,
                           TAP_STAGE[k], LPIPS_LAYERS[k].cout, (double*)(base + L.partial[k]));
    hipLaunchKernelGGL(lpips_finish_kernel, dim3(1), dim3(LP_T), 0, s, tp, dims, 0, io.out);
}

void launch_lpips_features(const LpipsIO& io, int tap, float* out, hipStream_t s) {
    const Layout L = layout_of(io.H, io.W, false);
    launch_features(io, L, tap, s);
    const int npix = L.npix[TAP_STAGE[tap]], C = LPIPS_LAYERS[tap].cout;
    hipLaunchKernelGGL(lpips_chw_kernel, dim3(grid_for((long long)npix * C)), dim3(LP_T), 0, s, (const float*)((char*)io.scratch + L.conv[tap]), npix, C, out);
}

void lpips_feature_shape(int H, int W, int tap, int* C, int* h, int* w) {
    *C = LPIPS_LAYERS[tap].cout;
    *h = *w = 0;
    stage_size(H, W, TAP_STAGE[tap], *h, *w);
}

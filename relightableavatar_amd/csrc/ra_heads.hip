// The two material heads of the relighting stage on cached surface features, forward and weight gradient (gfx950).
//
//   reference: albedo_network / roughness_network   lib/networks/relight/relight_network.py:45-47,91-104
//              MLP                                   lib/utils/net_utils.py:1242-1273 (256 -> 128 -> 128 -> {3, 1}, Softplus(beta = 100),
//                                                    output slope * sigmoid + bias)
//              what is trained                       lib/train/trainers/relight_trainer.py:113-118 (geometry frozen: the heads and the probe)
//
// Parameters are ONE flat fp32 vector theta in torch's own layout (include/relightableavatar.h, ra_heads_param_count); d_theta has the
// same layout.  Width 128 and depth 2 are compiled in.
//
// Operands are IEEE half with fp32 accumulation (v_mfma_f32_16x16x32_f16), WHATEVER ra_config.mlp_f16 says: the weight gradient in bf16
// operands is 7-13 x noisier than in f16, and nothing here is shared with the render kernels' streams.
// Arithmetic, per linear layer (the emulation of tests/test_oracle_heads_grad.py):
//   forward   y = q(x) q(W)^T + b                         q: round to f16; b, the activation and its derivative in fp32
//   backward  qd = q(s delta) / s,  dX = qd q(W),  dW = qd^T q(x),  db = sum delta (fp32, not rounded)
// s is a power of two found on the device per call and per head: 2^(4 - floor(log2 max |d_out|)), so the largest incoming gradient lands
// in [16, 32) whatever its scale — an MSE over a frame hands in gradients of 1e-6, whose f16 deltas would underflow.  Everything that acts
// on a delta is linear; slabs are multiplied by 1 / s (exact) in fp32 when they are written.  A delta beyond the f16 range saturates.
//
// Kernels (64-point tiles, 4 waves):
//   heads_pack_kernel   theta -> f16 images of the weights (W0, W1, W1^T, W2 padded to 4 rows, per head)
//   heads_kernel<0>     forward: feat -> LDS (f16) -> layer 0, 1 (MFMA; a wave owns 32 of the 128 columns for all 64 points) -> head (VALU)
//   heads_kernel<1>     the same forward with sigma' = sigmoid(100 z) kept in registers (the accumulator layout of a layer is the layout of
//                       its delta), then delta3 -> delta2 (VALU, K <= 3) -> delta1 (MFMA against W1^T); bias gradients, dW2.  Activations
//                       and scaled deltas go to a tape TRANSPOSED ([feature][point of the tile]: the accumulator holds four consecutive
//                       points of one feature per lane, an 8-byte store), which is the operand layout of
//   heads_dw_kernel     dW0 = delta1^T x0, dW1 = delta2^T h1: the contraction runs over the points, so both MFMA operands are 16-byte
//                       loads along the tape's point axis.  Grid (G, head, 3): two 64-row halves of dW0 and dW1.
//   heads_slab_sum      d_theta[i] = sum over the G partial slabs in slab order.
//
// Reproducibility: workgroup b of G = min(tiles, HEADS_MAX_GRID) takes tiles b, b + G, ... in order and owns slab b; no float atomics (the
// only atomic is an integer max for s).  The grid depends on n alone.  The two heads share nothing but the feature tape: a head whose
// incoming gradient is NULL is not launched, its slice of d_theta is zeroed, and the other head's slice does not change by a bit.
#include "ra_kernels.hpp"

namespace {

typedef _Float16 hf;
typedef __attribute__((ext_vector_type(8))) _Float16 hf8;
typedef __attribute__((ext_vector_type(4))) _Float16 hf4;

constexpr int TILE = 64, TPB = 256, W = 128, FIN = 256;
constexpr int XS = FIN + 8, HS = W + 8;                    // LDS row strides (halves)
// f16 weight images, halves per head
constexpr int P_W0 = 0, P_W1 = W * FIN, P_W1T = P_W1 + W * W, P_W2 = P_W1T + W * W, P_HEAD = P_W2 + 4 * W;
// theta offsets inside a head (floats)
constexpr int T_W0 = 0, T_B0 = W * FIN, T_W1 = T_B0 + W, T_B1 = T_W1 + W * W, T_W2 = T_B1 + W;
__host__ __device__ constexpr int head_nout(int hd) { return hd == 0 ? 3 : 1; }
__host__ __device__ constexpr int head_base(int hd) { return hd == 0 ? 0 : T_W2 + 3 * W + 3; }
__host__ __device__ constexpr int head_size(int hd) { return T_W2 + head_nout(hd) * (W + 1); }
static_assert(head_base(1) + head_size(1) == HEADS_PARAMS, "theta layout");
// tape of one tile (halves): x0^T, then per head h1^T, h2^T, delta1^T, delta2^T, each [feature][64 points]
constexpr int TP_X = 0, TP_HEAD0 = FIN * TILE, TP_H1 = 0, TP_H2 = W * TILE, TP_D1 = 2 * W * TILE, TP_D2 = 3 * W * TILE, TP_PER_HEAD = 4 * W * TILE;
constexpr int TP_TILE = TP_HEAD0 + 2 * TP_PER_HEAD;
static_assert((size_t)TP_TILE * sizeof(hf) == HEADS_TAPE_BYTES_PER_TILE, "tape size");

__device__ __forceinline__ f32x4 mfma16(const hf8& a, const hf8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ hf to_half_sat(float x) { return (hf)fminf(fmaxf(x, -65504.f), 65504.f); }

// 2^k with k = 4 - floor(log2 m) for the call's largest |gradient| m (bits of a non-negative float); 1 for m = 0 or non-finite
__device__ __forceinline__ int scale_exp(unsigned bits) {
    const int e = (int)(bits >> 23) & 255;
    if (bits == 0u || e == 255) return 0;
    const int k = 4 - (e - 127);
    return k < -120 ? -120 : (k > 120 ? 120 : k);
}

__global__ __launch_bounds__(256) void heads_pack_kernel(const float* __restrict__ theta, hf* __restrict__ w16) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * P_HEAD) return;
    const int hd = i / P_HEAD, o = i % P_HEAD;
    const float* th = theta + head_base(hd);
    float v;
    if (o < P_W1) v = th[T_W0 + o];
    else if (o < P_W1T) v = th[T_W1 + (o - P_W1)];
    else if (o < P_W2) { const int q = o - P_W1T, j = q / W, k = q % W; v = th[T_W1 + k * W + j]; }      // W1T[j][k] = W1[k][j]
    else { const int q = o - P_W2, r = q / W; v = r < head_nout(hd) ? th[T_W2 + q] : 0.f; }
    w16[i] = (hf)v;
}

__global__ __launch_bounds__(256) void heads_absmax_kernel(const float* __restrict__ g, size_t n, unsigned* __restrict__ out) {
    unsigned m = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned b = __builtin_bit_cast(unsigned, g[i]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)m, o); m = t > m ? t : m; }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);      // integer max: order-independent
}

struct HeadsArgs {
    const float* theta; const hf* w16; const float* feat; int n;       // the launch's points
    float *albedo, *rough;                                              // forward outputs (nullable)
    const float *d_albedo, *d_rough;                                    // backward: incoming gradients (NULL: head not launched)
    const unsigned* amax;                                               // backward: [2] bits of max |d_albedo|, max |d_rough| of the CALL
    hf* tape; float* slabs; int accumulate;                             // slabs: G x HEADS_PARAMS; accumulate: add to what an earlier chunk wrote
    int head0, x_writer;                                                // first head of the grid's y axis; the head that writes x0^T
    float slope[2], bias[2];
};

// z (fp32 accumulators of a 128-wide layer, bias added here) -> softplus100 -> f16 image [point][column] in LDS (+ transposed tape);
// returns sigma' in place of z when BWD
template <bool BWD>
__device__ __forceinline__ void layer_epilogue(f32x4 (&acc)[4][2], const float* __restrict__ bias, hf* __restrict__ img, hf* __restrict__ tapeT,
                                               int wv, int lane) {
    const int c16 = lane & 15, q = lane >> 4;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = (2 * wv + j) * 16 + c16;
        const float b = bias[col];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            hf4 hv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z = acc[mt][j][r] + b;
                const float t = 100.f * z;
                const float e = expf(-fabsf(t));
                const float sp = (fmaxf(t, 0.f) + log1pf(e)) * 0.01f;          // softplus(beta = 100), as torch: log1p(exp(beta z)) / beta
                hv[r] = (hf)sp;
                img[(mt * 16 + 4 * q + r) * HS + col] = hv[r];
                if (BWD) acc[mt][j][r] = t >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);      // sigmoid(beta z)
            }
            if (BWD) *reinterpret_cast<hf4*>(tapeT + col * TILE + mt * 16 + 4 * q) = hv;
        }
    }
}

template <bool BWD>
__global__ __launch_bounds__(TPB) void heads_kernel(HeadsArgs a) {
    __shared__ __attribute__((aligned(16))) hf sX[TILE * XS];        // layer 0's input; afterwards h2 and the head's deltas live here
    __shared__ __attribute__((aligned(16))) hf sH1[TILE * HS];       // h1; afterwards q(s delta2)
    hf* sH2 = sX;
    float* sD3 = reinterpret_cast<float*>(sX + TILE * HS);           // [64][4] s delta3 (fp32)
    float* sQ3 = sD3 + TILE * 4;                                     // [64][4] q(s delta3)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c16 = lane & 15, q = lane >> 4;
    const int hd = a.head0 + blockIdx.y, nout = head_nout(hd);
    const float* th = a.theta + head_base(hd);
    const hf* wh = a.w16 + (size_t)hd * P_HEAD;
    const int ntiles = (a.n + TILE - 1) / TILE;
    float s = 1.f, inv_s = 1.f;
    if (BWD) { const int k = scale_exp(a.amax[hd]); s = ldexpf(1.f, k); inv_s = ldexpf(1.f, -k); }
    const float* dout = hd == 0 ? a.d_albedo : a.d_rough;
    float* yout = hd == 0 ? a.albedo : a.rough;
    const float slope = a.slope[hd], obias = a.bias[hd];
    float b0acc[2] = {0.f, 0.f}, b1acc[2] = {0.f, 0.f}, w2acc[2] = {0.f, 0.f}, b2acc = 0.f;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int p0 = tile * TILE;
        hf* tp = BWD ? a.tape + (size_t)tile * TP_TILE : nullptr;
        hf* tph = BWD ? tp + TP_HEAD0 + (size_t)hd * TP_PER_HEAD : nullptr;
        // ---- features: thread t owns column t (of 256) of the tile's 64 rows
#pragma unroll 2
        for (int i = 0; i < TILE; i += 4) {
            hf4 hv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = p0 + i + r;
                hv[r] = (hf)(p < a.n ? a.feat[(size_t)p * FIN + tid] : 0.f);
                sX[(i + r) * XS + tid] = hv[r];
            }
            if (BWD && hd == a.x_writer) *reinterpret_cast<hf4*>(tp + TP_X + tid * TILE + i) = hv;
        }
        __syncthreads();
        // ---- layer 0: D[point][column] = X (A, LDS rows) x W0^T (B: rows of W0)
        f32x4 z1[4][2], z2[4][2];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int j = 0; j < 2; ++j) z1[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int ks = 0; ks < FIN / 32; ++ks) {
            hf8 bf[2], af[4];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const hf8*>(wh + P_W0 + ((2 * wv + j) * 16 + c16) * FIN + ks * 32 + 8 * q);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) af[mt] = *reinterpret_cast<const hf8*>(sX + (mt * 16 + c16) * XS + ks * 32 + 8 * q);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int j = 0; j < 2; ++j) z1[mt][j] = mfma16(af[mt], bf[j], z1[mt][j]);
        }
        layer_epilogue<BWD>(z1, th + T_B0, sH1, BWD ? tph + TP_H1 : nullptr, wv, lane);       // z1 := sigma'(z1) when BWD
        __syncthreads();                                                                       // sH1 complete; sX dead
        // ---- layer 1
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int j = 0; j < 2; ++j) z2[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int ks = 0; ks < W / 32; ++ks) {
            hf8 bf[2], af[4];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const hf8*>(wh + P_W1 + ((2 * wv + j) * 16 + c16) * W + ks * 32 + 8 * q);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) af[mt] = *reinterpret_cast<const hf8*>(sH1 + (mt * 16 + c16) * HS + ks * 32 + 8 * q);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int j = 0; j < 2; ++j) z2[mt][j] = mfma16(af[mt], bf[j], z2[mt][j]);
        }
        layer_epilogue<BWD>(z2, th + T_B1, sH2, BWD ? tph + TP_H2 : nullptr, wv, lane);
        __syncthreads();                                                                       // sH2 complete; sH1 dead
        // ---- head: thread (point, output)
        {
            const int pt = tid >> 2, o = tid & 3, p = p0 + pt;
            float sd = 0.f;
            if (o < nout) {
                float z = th[T_W2 + nout * W + o];
                const hf* hrow = sH2 + pt * HS;
                const hf* wrow = wh + P_W2 + o * W;
#pragma unroll 8
                for (int j = 0; j < W; ++j) z = __builtin_fmaf((float)hrow[j], (float)wrow[j], z);
                const float e = expf(-fabsf(z));
                const float sg = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
                if (p < a.n && yout) yout[(size_t)p * nout + o] = slope * sg + obias;
                if (BWD && p < a.n) sd = s * dout[(size_t)p * nout + o] * slope * (sg * (1.f - sg));
            }
            if (BWD) { sD3[tid] = sd; sQ3[tid] = (float)to_half_sat(sd); }
        }
        if (BWD) {
            __syncthreads();
            // ---- dW2[o][j] (thread: o = tid >> 7 and o + 2, j = tid & 127), db2
            {
                const int j = tid & 127, o = tid >> 7;
                float w0 = 0.f, w1 = 0.f;
#pragma unroll 4
                for (int pt = 0; pt < TILE; ++pt) {
                    const float h = (float)sH2[pt * HS + j];
                    w0 = __builtin_fmaf(sQ3[pt * 4 + o], h, w0);
                    w1 = __builtin_fmaf(sQ3[pt * 4 + o + 2], h, w1);
                }
                w2acc[0] += w0; w2acc[1] += w1;
                if (tid < 4) {
                    float t = 0.f;
#pragma unroll 4
                    for (int pt = 0; pt < TILE; ++pt) t += sD3[pt * 4 + tid];
                    b2acc += t;
                }
            }
            // ---- delta2 = (q(s delta3) q(W2)) sigma'(z2), in layer 1's accumulator layout
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = (2 * wv + j) * 16 + c16;
                float w2c[3] = {(float)wh[P_W2 + col], (float)wh[P_W2 + W + col], (float)wh[P_W2 + 2 * W + col]};
                float bsum = 0.f;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    hf4 hv;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int pt = mt * 16 + 4 * q + r;
                        float u = sQ3[pt * 4] * w2c[0];
                        if (nout > 1) { u = __builtin_fmaf(sQ3[pt * 4 + 1], w2c[1], u); u = __builtin_fmaf(sQ3[pt * 4 + 2], w2c[2], u); }
                        const float d = u * z2[mt][j][r];
                        bsum += d;
                        hv[r] = to_half_sat(d);
                        sH1[pt * HS + col] = hv[r];
                    }
                    *reinterpret_cast<hf4*>(tph + TP_D2 + col * TILE + mt * 16 + 4 * q) = hv;
                }
                bsum += __shfl_xor(bsum, 16);
                bsum += __shfl_xor(bsum, 32);
                b1acc[j] += bsum;
            }
            __syncthreads();                                                                   // q(s delta2) image complete
            // ---- delta1 = (q(s delta2) q(W1)) sigma'(z1): A = delta2 rows, B[k = i][n = j] = W1[i][j] = rows of W1^T
            f32x4 u1[4][2];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int j = 0; j < 2; ++j) u1[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
            for (int ks = 0; ks < W / 32; ++ks) {
                hf8 bf[2], af[4];
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const hf8*>(wh + P_W1T + ((2 * wv + j) * 16 + c16) * W + ks * 32 + 8 * q);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) af[mt] = *reinterpret_cast<const hf8*>(sH1 + (mt * 16 + c16) * HS + ks * 32 + 8 * q);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int j = 0; j < 2; ++j) u1[mt][j] = mfma16(af[mt], bf[j], u1[mt][j]);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = (2 * wv + j) * 16 + c16;
                float bsum = 0.f;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    hf4 hv;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float d = u1[mt][j][r] * z1[mt][j][r];
                        bsum += d;
                        hv[r] = to_half_sat(d);
                    }
                    *reinterpret_cast<hf4*>(tph + TP_D1 + col * TILE + mt * 16 + 4 * q) = hv;
                }
                bsum += __shfl_xor(bsum, 16);
                bsum += __shfl_xor(bsum, 32);
                b0acc[j] += bsum;
            }
        }
        __syncthreads();                                                                       // the LDS images are free for the next tile
    }
    if (BWD) {      // this workgroup's slab: bias gradients and the last layer, unscaled
        float* slab = a.slabs + (size_t)blockIdx.x * HEADS_PARAMS + head_base(hd);
        auto put = [&](int i, float v) { slab[i] = a.accumulate ? slab[i] + v * inv_s : v * inv_s; };
        if (q == 0) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = (2 * wv + j) * 16 + c16;
                put(T_B0 + col, b0acc[j]);
                put(T_B1 + col, b1acc[j]);
            }
        }
        const int j = tid & 127, o = tid >> 7;
        if (o < nout) put(T_W2 + o * W + j, w2acc[0]);
        if (o + 2 < nout) put(T_W2 + (o + 2) * W + j, w2acc[1]);
        if (tid < nout) put(T_W2 + nout * W + tid, b2acc);
    }
}

// dW = delta^T x over the points of the workgroup's tiles.  part 0, 1: rows 64 part .. + 63 of dW0 (delta1^T x0: 64 x 256, a wave owns
// 64 columns); part 2: dW1 (delta2^T h1: 128 x 128, a wave owns 32 columns).  Both operands are 16-byte loads along the tape's point axis.
struct DwArgs { const hf* tape; int ntiles; const unsigned* amax; float* slabs; int accumulate; int head0; };

template <int MT, int NT>
__device__ __forceinline__ void dw_part(const DwArgs& a, const hf* __restrict__ AT0, const hf* __restrict__ BT0, int row0, int col0, int ncols,
                                        float* __restrict__ out, float inv_s, int lane) {
    const int c16 = lane & 15, q = lane >> 4;
    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const hf* AT = AT0 + (size_t)tile * TP_TILE;
        const hf* BT = BT0 + (size_t)tile * TP_TILE;
#pragma unroll
        for (int ks = 0; ks < TILE / 32; ++ks) {
            hf8 af[MT], bf[NT];
#pragma unroll
            for (int m = 0; m < MT; ++m) af[m] = *reinterpret_cast<const hf8*>(AT + (row0 + m * 16 + c16) * TILE + ks * 32 + 8 * q);
#pragma unroll
            for (int n = 0; n < NT; ++n) bf[n] = *reinterpret_cast<const hf8*>(BT + (col0 + n * 16 + c16) * TILE + ks * 32 + 8 * q);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[m][n] = mfma16(af[m], bf[n], acc[m][n]);
        }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float* o = out + (size_t)(row0 + m * 16 + 4 * q + r) * ncols + col0 + n * 16 + c16;
                const float v = acc[m][n][r] * inv_s;
                *o = a.accumulate ? *o + v : v;
            }
}

__global__ __launch_bounds__(TPB) void heads_dw_kernel(DwArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int hd = a.head0 + blockIdx.y, part = blockIdx.z;
    const float inv_s = ldexpf(1.f, -scale_exp(a.amax[hd]));
    const hf* th = a.tape + TP_HEAD0 + (size_t)hd * TP_PER_HEAD;
    float* slab = a.slabs + (size_t)blockIdx.x * HEADS_PARAMS + head_base(hd);
    if (part < 2) dw_part<4, 4>(a, th + TP_D1, a.tape + TP_X, 64 * part, 64 * wv, FIN, slab + T_W0, inv_s, lane);
    else dw_part<8, 2>(a, th + TP_D2, th + TP_H1, 0, 32 * wv, W, slab + T_W1, inv_s, lane);
}

// out[i] = sum over the G slabs, in slab order (four interleaved partial sums, combined in a fixed order)
__global__ __launch_bounds__(256) void heads_slab_sum_kernel(const float* __restrict__ slabs, int G, int i0, int n, float* __restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int i = i0 + k;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int b = 0;
    for (; b + 4 <= G; b += 4) {
        a0 += slabs[(size_t)b * HEADS_PARAMS + i];
        a1 += slabs[(size_t)(b + 1) * HEADS_PARAMS + i];
        a2 += slabs[(size_t)(b + 2) * HEADS_PARAMS + i];
        a3 += slabs[(size_t)(b + 3) * HEADS_PARAMS + i];
    }
    for (; b < G; ++b) a0 += slabs[(size_t)b * HEADS_PARAMS + i];
    out[i] = (a0 + a1) + (a2 + a3);
}

void fill_cfg(HeadsArgs& k, const ra_config& cfg) {
    k.slope[0] = cfg.albedo_slope; k.bias[0] = cfg.albedo_bias;
    k.slope[1] = cfg.roughness_slope; k.bias[1] = cfg.roughness_bias;
}

}  // namespace

int heads_grid(int n) {
    const int tiles = (n + TILE - 1) / TILE;
    return tiles < HEADS_MAX_GRID ? tiles : HEADS_MAX_GRID;
}

void launch_heads_forward(const HeadsIO& io, const ra_config& cfg, hipStream_t s) {
    if (io.n <= 0) return;
    hipLaunchKernelGGL(heads_pack_kernel, dim3((2 * P_HEAD + 255) / 256), dim3(256), 0, s, io.theta, reinterpret_cast<hf*>(io.w16));
    HeadsArgs k{};
    k.theta = io.theta; k.w16 = reinterpret_cast<const hf*>(io.w16); k.feat = io.feat; k.n = io.n;
    k.albedo = io.albedo; k.rough = io.rough;
    fill_cfg(k, cfg);
    const int tiles = (io.n + TILE - 1) / TILE;
    const int h0 = io.albedo ? 0 : 1, nh = (io.albedo ? 1 : 0) + (io.rough ? 1 : 0);
    if (nh == 0) return;
    k.head0 = h0;
    hipLaunchKernelGGL(heads_kernel<false>, dim3(tiles < 2048 ? tiles : 2048, nh), dim3(TPB), 0, s, k);
}

void launch_heads_backward(const HeadsIO& io, const ra_config& cfg, hipStream_t s) {
    if (io.n <= 0) return;
    const int G = heads_grid(io.n);
    const int h0 = io.d_albedo ? 0 : 1, nh = (io.d_albedo ? 1 : 0) + (io.d_rough ? 1 : 0);
    for (int hd = 0; hd < 2; ++hd) {
        const bool on = hd == 0 ? io.d_albedo != nullptr : io.d_rough != nullptr;
        if (!on) (void)hipMemsetAsync(io.d_theta + head_base(hd), 0, (size_t)head_size(hd) * sizeof(float), s);
    }
    if (nh == 0) return;
    hipLaunchKernelGGL(heads_pack_kernel, dim3((2 * P_HEAD + 255) / 256), dim3(256), 0, s, io.theta, reinterpret_cast<hf*>(io.w16));
    (void)hipMemsetAsync(io.amax, 0, 2 * sizeof(unsigned), s);
    if (io.d_albedo) hipLaunchKernelGGL(heads_absmax_kernel, dim3(64), dim3(256), 0, s, io.d_albedo, (size_t)io.n * 3, io.amax);
    if (io.d_rough) hipLaunchKernelGGL(heads_absmax_kernel, dim3(64), dim3(256), 0, s, io.d_rough, (size_t)io.n, io.amax + 1);
    for (int c0 = 0; c0 < io.n; c0 += HEADS_CHUNK) {       // the tape holds HEADS_CHUNK points; the slabs carry on from chunk to chunk
        const int nc = io.n - c0 < HEADS_CHUNK ? io.n - c0 : HEADS_CHUNK;
        HeadsArgs k{};
        k.theta = io.theta; k.w16 = reinterpret_cast<const hf*>(io.w16); k.feat = io.feat + (size_t)c0 * FIN; k.n = nc;
        k.d_albedo = io.d_albedo ? io.d_albedo + (size_t)c0 * 3 : nullptr;
        k.d_rough = io.d_rough ? io.d_rough + c0 : nullptr;
        k.amax = io.amax; k.tape = reinterpret_cast<hf*>(io.tape); k.slabs = io.slabs; k.accumulate = c0 > 0;
        k.head0 = h0; k.x_writer = h0;
        fill_cfg(k, cfg);
        hipLaunchKernelGGL(heads_kernel<true>, dim3(G, nh), dim3(TPB), 0, s, k);
        DwArgs d{};
        d.tape = k.tape; d.ntiles = (nc + TILE - 1) / TILE; d.amax = io.amax; d.slabs = io.slabs; d.accumulate = k.accumulate; d.head0 = h0;
        hipLaunchKernelGGL(heads_dw_kernel, dim3(G, nh, 3), dim3(TPB), 0, s, d);
    }
    for (int hd = h0; hd < h0 + nh; ++hd)
        hipLaunchKernelGGL(heads_slab_sum_kernel, dim3((head_size(hd) + 255) / 256), dim3(256), 0, s, io.slabs, G, head_base(hd), head_size(hd), io.d_theta);
}

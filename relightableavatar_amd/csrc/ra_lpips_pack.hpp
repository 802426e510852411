// LPIPS (AlexNet): the five convolutions' shapes and the host packer of their weights.  Plain C++ (no HIP): also compiled on its own by
// tests/native/lpips_pack_main.cpp under the host sanitizers.
//
// A convolution runs as an implicit GEMM (ra_lpips.hip): out[m][n] = sum_k A[m][k] B[k][n] with m = an output pixel of either image,
// n = an output channel and k = (ky * ks + kx) * Cin + ci — the channels of one filter tap are contiguous, like the NHWC activations
// the A operand is gathered from.  K is padded with zeros to a multiple of LPIPS_BK (conv1: 363 -> 384).
// Packed order = the order the kernel reads: per block column of LPIPS_BN output channels, per K tile of LPIPS_BK, a dense
// [LPIPS_BK][LPIPS_BN] tile (one contiguous 8 KB copy into LDS per workgroup and K step).
#pragma once
#include <cstddef>

struct LpipsLayer { int cin, cout, ks, stride, pad; };
constexpr int LPIPS_TAPS = 5;
constexpr LpipsLayer LPIPS_LAYERS[LPIPS_TAPS] = {{3, 64, 11, 4, 2}, {64, 192, 5, 1, 2}, {192, 384, 3, 1, 1}, {384, 256, 3, 1, 1}, {256, 256, 3, 1, 1}};
constexpr int LPIPS_BM = 128;     // output pixels per workgroup tile
constexpr int LPIPS_BN = 64;      // output channels per workgroup tile (divides every Cout)
constexpr int LPIPS_BK = 32;      // K per LDS stage (divides Cin of conv2..5: a stage never straddles two filter taps there)
constexpr int LPIPS_MIN_SIDE = 31;    // the smallest image side for which every stage has an output

constexpr int lpips_k(const LpipsLayer& l) { return l.cin * l.ks * l.ks; }
constexpr int lpips_kpad(const LpipsLayer& l) { return (lpips_k(l) + LPIPS_BK - 1) / LPIPS_BK * LPIPS_BK; }
constexpr size_t lpips_packed_count(const LpipsLayer& l) { return (size_t)lpips_kpad(l) * l.cout; }

// sizes of the stages for an input side n >= LPIPS_MIN_SIDE: conv1 (k 11, stride 4, pad 2), the two 3 / 2 pools (no pad, floor)
constexpr int lpips_conv1_side(int n) { return (n + 2 * 2 - 11) / 4 + 1; }
constexpr int lpips_pool_side(int n) { return (n - 3) / 2 + 1; }

inline size_t lpips_packed_index(const LpipsLayer& l, int n, int k) {
    const int kt = lpips_kpad(l) / LPIPS_BK;
    return (((size_t)(n / LPIPS_BN) * kt + k / LPIPS_BK) * LPIPS_BK + k % LPIPS_BK) * LPIPS_BN + n % LPIPS_BN;
}

// w: (Cout, Cin, ks, ks) as torch stores it -> packed: lpips_packed_count(l) floats
inline void lpips_pack_conv(const LpipsLayer& l, const float* w, float* packed) {
    const size_t total = lpips_packed_count(l);
    for (size_t i = 0; i < total; ++i) packed[i] = 0.f;
    for (int n = 0; n < l.cout; ++n)
        for (int ci = 0; ci < l.cin; ++ci)
            for (int ky = 0; ky < l.ks; ++ky)
                for (int kx = 0; kx < l.ks; ++kx)
                    packed[lpips_packed_index(l, n, (ky * l.ks + kx) * l.cin + ci)] = w[(((size_t)n * l.cin + ci) * l.ks + ky) * l.ks + kx];
}

inline void lpips_unpack_conv(const LpipsLayer& l, const float* packed, float* w) {
    for (int n = 0; n < l.cout; ++n)
        for (int ci = 0; ci < l.cin; ++ci)
            for (int ky = 0; ky < l.ks; ++ky)
                for (int kx = 0; kx < l.ks; ++kx)
                    w[(((size_t)n * l.cin + ci) * l.ks + ky) * l.ks + kx] = packed[lpips_packed_index(l, n, (ky * l.ks + kx) * l.cin + ci)];
}

// the device arena: the five packed convolutions, then bias[5], lin[5], shift[3], scale[3]; every part starts on a multiple of 64 floats
struct LpipsArena {
    size_t conv[LPIPS_TAPS], bias[LPIPS_TAPS], lin[LPIPS_TAPS], shift, scale, total;
};
inline LpipsArena lpips_arena() {
    LpipsArena a{};
    size_t o = 0;
    auto take = [&o](size_t n) { const size_t at = o; o += (n + 63) / 64 * 64; return at; };
    for (int k = 0; k < LPIPS_TAPS; ++k) a.conv[k] = take(lpips_packed_count(LPIPS_LAYERS[k]));
    for (int k = 0; k < LPIPS_TAPS; ++k) a.bias[k] = take(LPIPS_LAYERS[k].cout);
    for (int k = 0; k < LPIPS_TAPS; ++k) a.lin[k] = take(LPIPS_LAYERS[k].cout);
    a.shift = take(3);
    a.scale = take(3);
    a.total = o;
    return a;
}

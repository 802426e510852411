// Stand-alone check of the LPIPS weight packer (relightableavatar_amd/csrc/ra_lpips_pack.hpp), meant to be built with the host sanitizers:
//     c++ -std=c++17 -fsanitize=address,undefined -I relightableavatar_amd/csrc tests/native/lpips_pack_main.cpp -o lpips_pack_main
// For each of the five convolutions: pack -> unpack gives the weights back bit for bit, every weight lands in exactly one slot, every
// other slot (the K padding of conv1) is zero, and the arena's parts do not overlap.  Buffers are sized exactly, so an index one past
// either array is an AddressSanitizer report.
#include "ra_lpips_pack.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

int main() {
    int bad = 0;
    for (int k = 0; k < LPIPS_TAPS; ++k) {
        const LpipsLayer& l = LPIPS_LAYERS[k];
        const size_t n = (size_t)l.cout * lpips_k(l), np = lpips_packed_count(l);
        std::vector<float> w(n), packed(np, -1.f), back(n, -2.f);
        uint32_t s = 12345u + (uint32_t)k;
        for (size_t i = 0; i < n; ++i) {                      // nonzero, asymmetric values
            s = s * 1664525u + 1013904223u;
            w[i] = 1.f + (float)(s >> 8) * (1.f / 16777216.f) + (float)(i % 7);
        }
        lpips_pack_conv(l, w.data(), packed.data());
        lpips_unpack_conv(l, packed.data(), back.data());
        if (std::memcmp(w.data(), back.data(), n * sizeof(float)) != 0) { std::printf("layer %d: round trip differs\n", k); ++bad; }
        size_t nonzero = 0;
        for (size_t i = 0; i < np; ++i) nonzero += packed[i] != 0.f;
        if (nonzero != n) { std::printf("layer %d: %zu nonzero slots, %zu weights\n", k, nonzero, n); ++bad; }
        // the padding rows are the k beyond K of every block column
        for (int c = 0; c < l.cout; ++c)
            for (int kk = lpips_k(l); kk < lpips_kpad(l); ++kk)
                if (packed[lpips_packed_index(l, c, kk)] != 0.f) { std::printf("layer %d: padding slot (%d, %d) not zero\n", k, c, kk); ++bad; }
        if (lpips_kpad(l) % LPIPS_BK || l.cout % LPIPS_BN || lpips_kpad(l) - lpips_k(l) >= LPIPS_BK) { std::printf("layer %d: bad tiling\n", k); ++bad; }
        std::printf("layer %d: Cout %d Cin %d k %d: K %d -> %d, %zu packed floats\n", k, l.cout, l.cin, l.ks, lpips_k(l), lpips_kpad(l), np);
    }
    const LpipsArena a = lpips_arena();
    size_t end = 0;
    for (int k = 0; k < LPIPS_TAPS; ++k) { if (a.conv[k] < end || a.conv[k] % 64) ++bad; end = a.conv[k] + lpips_packed_count(LPIPS_LAYERS[k]); }
    for (int k = 0; k < LPIPS_TAPS; ++k) { if (a.bias[k] < end || a.bias[k] % 64) ++bad; end = a.bias[k] + LPIPS_LAYERS[k].cout; }
    for (int k = 0; k < LPIPS_TAPS; ++k) { if (a.lin[k] < end || a.lin[k] % 64) ++bad; end = a.lin[k] + LPIPS_LAYERS[k].cout; }
    if (a.shift < end || a.scale < a.shift + 3 || a.total < a.scale + 3) ++bad;
    if (bad) { std::printf("FAILED: %d\n", bad); return 1; }
    std::printf("round trip ok: %d layers, arena %zu floats\n", LPIPS_TAPS, a.total);
    return 0;
}

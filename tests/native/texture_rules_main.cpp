// A stand-alone CPU program around csrc/ra_texture_rules.hpp (built with -fsanitize=address,undefined by tests/test_oracle_texture.py).
// It reads one case from the file named on its command line — whitespace-separated tokens, every float as the hexadecimal bits of its
// fp32 value:
//     Bt TH TW C B H W filter boundary max_mip_level, tex (Bt TH TW C), uv (B H W 2), uv_da (B H W 4), dout (B H W C)
// builds the mip chain with texture_levels / texture_mean, and prints, for the test to compare bit for bit with the float32 restatement
// (tests/texture_ref.py):
//     levels <n> <h w offset> ...
//     log2 <x> <texture_log2(x)>                  for eight fixed arguments
//     px <b> <pixel> <ok> <l0> <two> <f> [<idx0..3> <w0..3> per level read] out <C values> duv <2 values>      every pixel; nearest prints
//                                                 its one texel in place of the taps
//     done <pixels>
#include "ra_texture_rules.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static unsigned bits(float x) { unsigned u; std::memcpy(&u, &x, 4); return u; }
static bool read_floats(std::FILE* f, std::vector<float>& v) {
    for (float& x : v) {
        unsigned u;
        if (std::fscanf(f, "%x", &u) != 1) return false;
        std::memcpy(&x, &u, 4);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: texture_rules_main <case file>\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int Bt, TH, TW, C, B, H, W, filter, boundary, mm;
    if (std::fscanf(f, "%d %d %d %d %d %d %d %d %d %d", &Bt, &TH, &TW, &C, &B, &H, &W, &filter, &boundary, &mm) != 10 || Bt < 1 || TH < 1 || TW < 1 || C < 1 ||
        C > TEX_MAX_CHANNELS || B < 1 || H < 1 || W < 1 || (Bt != 1 && Bt != B) || filter < TEX_NEAREST || filter > TEX_TRILINEAR || boundary < TEX_WRAP ||
        boundary > TEX_CLAMP || mm < 0 || TH > 4096 || TW > 4096) {
        std::printf("bad header\n");
        return 2;
    }
    const size_t HW = (size_t)H * W;
    std::vector<float> tex((size_t)Bt * TH * TW * C), uv(B * HW * 2), da(B * HW * 4), dout(B * HW * C);
    if (!read_floats(f, tex) || !read_floats(f, uv) || !read_floats(f, da) || !read_floats(f, dout)) { std::printf("short case file\n"); return 2; }
    std::fclose(f);

    TexLevels L;
    texture_levels(TH, TW, filter == TEX_TRILINEAR ? mm : 0, L);
    std::printf("levels %d", L.n);
    for (int l = 0; l < L.n; ++l) std::printf(" %d %d %lld", L.h[l], L.w[l], L.off[l]);
    std::printf("\n");
    const size_t total = (size_t)L.off[L.n];
    std::vector<float> chain((size_t)Bt * total * C);
    for (int bt = 0; bt < Bt; ++bt) {
        float* base = chain.data() + bt * total * C;
        std::memcpy(base, tex.data() + (size_t)bt * TH * TW * C, (size_t)TH * TW * C * sizeof(float));
        for (int l = 1; l < L.n; ++l) {
            const float* s = base + L.off[l - 1] * C;
            float* d = base + L.off[l] * C;
            const int sw = L.w[l - 1];
            for (int y = 0; y < L.h[l]; ++y)
                for (int x = 0; x < L.w[l]; ++x)
                    for (int c = 0; c < C; ++c) {
                        const size_t r0 = (size_t)(2 * y) * sw + 2 * x, r1 = r0 + sw;
                        d[((size_t)y * L.w[l] + x) * C + c] = texture_mean(s[r0 * C + c], s[(r0 + 1) * C + c], s[r1 * C + c], s[(r1 + 1) * C + c]);
                    }
        }
    }
    const float probes[8] = {1.0f, 1.41421354f, 1.41421366f, 2.0f, 3.0f, 1.17549435e-38f, 65536.5f, 3.0e38f};
    for (float x : probes) std::printf("log2 %08x %08x\n", bits(x), bits(texture_log2(x)));

    size_t n = 0;
    std::vector<float> out(C);
    for (int b = 0; b < B; ++b)
        for (size_t q = 0; q < HW; ++q, ++n) {
            const size_t i = b * HW + q;
            TexPixel p;
            texture_pixel(uv[2 * i], uv[2 * i + 1], da.data() + 4 * i, L, filter, boundary, p);
            std::printf("px %d %zu %d %d %d %08x", b, q, p.ok, p.l0, p.two, bits(p.f));
            const float* base = chain.data() + (Bt == 1 ? 0 : b) * total * C;
            float duv[2] = {0.0f, 0.0f};
            for (int c = 0; c < C; ++c) out[c] = 0.0f;
            if (p.ok && filter == TEX_NEAREST) {
                std::printf(" %d", p.t[0].idx[0]);
                for (int c = 0; c < C; ++c) out[c] = base[(size_t)p.t[0].idx[0] * C + c];
            } else if (p.ok) {
                for (int k = 0; k <= p.two; ++k) {
                    for (int t = 0; t < 4; ++t) std::printf(" %d", p.t[k].idx[t]);
                    for (int t = 0; t < 4; ++t) std::printf(" %08x", bits(p.t[k].w[t]));
                }
                const int l1 = p.two ? p.l0 + 1 : p.l0;
                const float *a = base + L.off[p.l0] * C, *bb = base + L.off[l1] * C;
                for (int c = 0; c < C; ++c) out[c] = texture_value(p, a + c, bb + c, C);
                texture_duv(p, a, bb, dout.data() + i * C, C, L.w[p.l0], L.h[p.l0], L.w[l1], L.h[l1], duv);
            }
            std::printf(" out");
            for (int c = 0; c < C; ++c) std::printf(" %08x", bits(out[c]));
            std::printf(" duv %08x %08x\n", bits(duv[0]), bits(duv[1]));
        }
    std::printf("done %zu\n", n);
    return 0;
}

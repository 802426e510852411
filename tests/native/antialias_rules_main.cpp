// A stand-alone CPU program around csrc/ra_antialias_rules.hpp (built with -fsanitize=address,undefined by
// tests/test_oracle_antialias.py).  It reads one case from the file named on its command line — whitespace-separated tokens, every
// float as the hexadecimal bits of its fp32 value:
//     B V F H W C, pos (B V 4), faces (F 3), face map (B H W, decimal), zw (B H W), color (B H W C), dout (B H W C)
// builds the twin array of the faces as ra_topo_create defines it, and prints, for the test to compare bit for bit with the float32
// restatement (tests/antialias_ref.py):
//     flags <n>                                           faces on which antialias_face_flags differs from raster_setup's flags (must be 0)
//     pair <b> <slot> <own> <k> <he> <alpha> <c0> <c1> <c2> <cross> <dc0> <dc1> <dc2> <da0..2> <db0..2>      every active pair, ascending
//     out <b> <pixel> <c> <value>                         every value of the forward that differs from its input colour
//     done <active pairs> <changed values>
#include "ra_antialias_rules.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

static unsigned bits(float x) { unsigned u; std::memcpy(&u, &x, 4); return u; }
static bool read_float(std::FILE* f, float* x) {
    unsigned u;
    if (std::fscanf(f, "%x", &u) != 1) return false;
    std::memcpy(x, &u, 4);
    return true;
}
static bool read_floats(std::FILE* f, std::vector<float>& v) {
    for (float& x : v) if (!read_float(f, &x)) return false;
    return true;
}
static bool read_ints(std::FILE* f, std::vector<int>& v) {
    for (int& x : v) if (std::fscanf(f, "%d", &x) != 1) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: antialias_rules_main <case file>\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int B, V, F, H, W, C;
    if (std::fscanf(f, "%d %d %d %d %d %d", &B, &V, &F, &H, &W, &C) != 6 || B < 0 || V < 0 || F < 0 || H < 0 || W < 0 || C < 1) { std::printf("bad header\n"); return 2; }
    const size_t HW = (size_t)H * W;
    std::vector<float> pos((size_t)B * V * 4), zw(B * HW), color(B * HW * C), dout(B * HW * C);
    std::vector<int> faces((size_t)F * 3), face(B * HW);
    if (!read_floats(f, pos) || !read_ints(f, faces) || !read_ints(f, face) || !read_floats(f, zw) || !read_floats(f, color) || !read_floats(f, dout)) {
        std::printf("short case file\n");
        return 2;
    }
    std::fclose(f);
    for (int x : faces) if (x < 0 || x >= V) { std::printf("face index outside [0, V)\n"); return 2; }

    // half-edge 3 f + k leaves corner k towards corner (k + 1) % 3; twin: the other half-edge of an edge with exactly two, else -count
    std::map<std::pair<int, int>, std::vector<int>> edges;
    for (int h = 0; h < 3 * F; ++h) {
        const int a = faces[h], b = faces[3 * (h / 3) + (h % 3 + 1) % 3];
        edges[{a < b ? a : b, a < b ? b : a}].push_back(h);
    }
    std::vector<int> twin((size_t)3 * F + 1, -1);
    for (const auto& e : edges) {
        if (e.second.size() == 2) { twin[e.second[0]] = e.second[1]; twin[e.second[1]] = e.second[0]; }
        else for (int h : e.second) twin[h] = -(int)e.second.size();
    }

    int flag_mismatches = 0;
    for (int b = 0; b < B; ++b)
        for (int g = 0; g < F; ++g) {
            const int* i = &faces[3 * g];
            const float* p = &pos[(size_t)4 * b * V];
            RasterFace r;
            raster_setup(p + 4 * i[0], p + 4 * i[1], p + 4 * i[2], i[0], i[1], i[2], H, W, r);
            flag_mismatches += antialias_face_flags(p + 4 * i[0], p + 4 * i[1], p + 4 * i[2], i[0], i[1], i[2]) != r.flags;
        }
    std::printf("flags %d\n", flag_mismatches);

    long long n_active = 0, n_changed = 0;
    for (int b = 0; b < B; ++b) {
        const int* fm = face.data() + b * HW;
        const float *z = zw.data() + b * HW, *p = pos.data() + (size_t)4 * b * V;
        const float *col = color.data() + b * HW * C, *go = dout.data() + b * HW * C;
        for (long long slot = 0; slot < 2 * (long long)HW; ++slot) {
            const long long q = slot >> 1;
            const int vertical = (int)(slot & 1), y = (int)(q / W), x = (int)(q - (long long)y * W);
            if (vertical ? y + 1 >= H : x + 1 >= W) continue;
            AaPair pr;
            antialias_pair(fm, z, p, faces.data(), twin.data(), F, H, W, x, y, vertical, pr);
            if (!pr.active) continue;
            ++n_active;
            const long long first = q, second = vertical ? q + W : q + 1;
            const long long tp = antialias_target(pr) ? second : first, sp = antialias_target(pr) ? first : second;
            float g = 0.0f;
            for (int c = 0; c < C; ++c) {
                const float diff = col[sp * C + c] - col[tp * C + c];
                const float prod = go[tp * C + c] * diff;
                g = g + prod;
            }
            if (pr.alpha < 0.0f) g = -g;
            float dc[3], da[3], db[3];
            antialias_dc(pr, vertical, vertical ? H : W, g, dc);
            const int ff = pr.he / 3, cc = pr.he - 3 * ff, tail = faces[pr.he], head = faces[3 * ff + (cc + 1) % 3];
            antialias_ends(p + 4 * (tail < head ? tail : head), p + 4 * (tail < head ? head : tail), dc, da, db);
            std::printf("pair %d %lld %d %d %d %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x\n", b, slot, pr.own, pr.k, pr.he, bits(pr.alpha),
                        bits(pr.c[0]), bits(pr.c[1]), bits(pr.c[2]), bits(pr.cross), bits(dc[0]), bits(dc[1]), bits(dc[2]), bits(da[0]), bits(da[1]), bits(da[2]),
                        bits(db[0]), bits(db[1]), bits(db[2]));
        }
        // the forward: every pixel gathers its pairs in the order left, right, up, down
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const long long pix = (long long)y * W + x;
                float w[4];
                long long other[4];
                bool use[4];
                for (int k = 0; k < 4; ++k) {
                    const int vertical = k >> 1, me = (k & 1) ? 0 : 1, fx = k == 0 ? x - 1 : x, fy = k == 2 ? y - 1 : y;
                    use[k] = false;
                    if (!(k == 0 ? x > 0 : k == 1 ? x + 1 < W : k == 2 ? y > 0 : y + 1 < H)) continue;
                    AaPair pr;
                    antialias_pair(fm, z, p, faces.data(), twin.data(), F, H, W, fx, fy, vertical, pr);
                    if (!pr.active || antialias_target(pr) != me) continue;
                    const long long first = (long long)fy * W + fx, second = vertical ? first + W : first + 1;
                    use[k] = true; w[k] = antialias_weight(pr); other[k] = me ? first : second;
                }
                for (int c = 0; c < C; ++c) {
                    const float mine = col[pix * C + c];
                    float acc = mine;
                    for (int k = 0; k < 4; ++k) if (use[k]) acc = antialias_blend(acc, w[k], col[other[k] * C + c], mine);
                    if (bits(acc) != bits(mine)) { std::printf("out %d %lld %d %08x\n", b, pix, c, bits(acc)); ++n_changed; }
                }
            }
    }
    std::printf("done %lld %lld\n", n_active, n_changed);
    return 0;
}

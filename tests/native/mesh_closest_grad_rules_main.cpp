// A stand-alone CPU program around csrc/ra_mesh_grad_rules.hpp (built with -fsanitize=address,undefined by
// tests/test_oracle_mesh_closest_grad.py).  It reads one case from the file named on its command line — whitespace-separated tokens,
// every float as the hexadecimal bits of its fp32 value:
//     F V n C has_g identity, faces (F 3 ints), face (n ints), pts (n 3), closest (n 3), bary (n 3), g (n, when has_g), ga (n C)
// runs the header's functions row by row, sorts the slots' keys as the device does (vertex, 3 i + k), sums every run as a wave does —
// lane l adds terms l, l + 64, ... from +0, the lanes meet in the xor tree 32, 16, .., 1 — and prints, for the test to compare bit for
// bit with the float32 restatement (tests/mesh_closest_grad_ref.py):
//     live <n>                    the live rows it counted
//     dpts <bits> ...             n 3 values (when has_g)
//     dverts <bits> ...           V 3 values (when has_g)
//     dattr <bits> ...            V C values
//     identity <worst>            when `identity`: the largest | dpts + sum_k dv_k | / (2^-23 |dpts|) over the finite live rows, which
//                                 it also asserts to be at most 8 (three product roundings, two additions, |sum bary - 1| <= 4 x 2^-23)
#include "ra_mesh_grad_rules.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

typedef unsigned long long u64;

static unsigned bits(float x) { unsigned u; std::memcpy(&u, &x, 4); return u; }
static bool read_floats(std::FILE* f, std::vector<float>& v) {
    for (float& x : v) {
        unsigned u;
        if (std::fscanf(f, "%x", &u) != 1) return false;
        std::memcpy(&x, &u, 4);
    }
    return true;
}
static bool read_ints(std::FILE* f, std::vector<int>& v) {
    for (int& x : v) if (std::fscanf(f, "%d", &x) != 1) return false;
    return true;
}
static void print(const char* name, const std::vector<float>& v) {
    std::printf("%s", name);
    for (float x : v) std::printf(" %08x", bits(x));
    std::printf("\n");
}

// what lane 0 of a wave holds: terms[first .. first + count) of `stride` floats each, channel c
static float wave_sum(const std::vector<float>& terms, size_t first, size_t count, int stride, int c) {
    float lane[64];
    for (int l = 0; l < 64; ++l) {
        float acc = 0.0f;
        for (size_t t = l; t < count; t += 64) acc = acc + terms[(first + t) * stride + c];
        lane[l] = acc;
    }
    for (int w = 32; w > 0; w >>= 1) {
        float next[64];
        for (int l = 0; l < 64; ++l) next[l] = lane[l] + lane[l ^ w];
        std::memcpy(lane, next, sizeof lane);
    }
    return lane[0];
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: mesh_closest_grad_rules_main <case file>\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int F, V, n, C, has_g, identity;
    if (std::fscanf(f, "%d %d %d %d %d %d", &F, &V, &n, &C, &has_g, &identity) != 6 || F < 1 || V < 1 || n < 0 || C < 0 || C > MESHG_MAX_C) {
        std::printf("bad header\n");
        return 2;
    }
    std::vector<int> faces((size_t)F * 3), face(n);
    std::vector<float> pts((size_t)n * 3), closest((size_t)n * 3), bary((size_t)n * 3), g(has_g ? n : 0), ga((size_t)n * C);
    if (!read_ints(f, faces) || !read_ints(f, face) || !read_floats(f, pts) || !read_floats(f, closest) || !read_floats(f, bary) || !read_floats(f, g) ||
        !read_floats(f, ga)) {
        std::printf("short case file\n");
        return 2;
    }
    std::fclose(f);

    // the row pass: dpts and the keys; a dead row gets the largest key
    const u64 slots = 3ull * (u64)n, inert = (u64)V * slots;
    std::vector<float> dpts((size_t)n * 3, 0.0f);
    std::vector<u64> keys((size_t)n * 3);
    int n_live = 0;
    double worst = 0.0;
    for (int i = 0; i < n; ++i) {
        int idx[3];
        const bool live = mesh_grad_live(face[i], faces.data(), F, V, idx);
        n_live += live;
        if (live && has_g) {
            mesh_grad_dpts(&pts[3 * (size_t)i], &closest[3 * (size_t)i], g[i], &dpts[3 * (size_t)i]);
            if (identity)
                for (int c = 0; c < 3; ++c) {
                    const float d = dpts[3 * (size_t)i + c];
                    float s = mesh_grad_vert_term(bary[3 * (size_t)i], d);
                    for (int k = 1; k < 3; ++k) s = s + mesh_grad_vert_term(bary[3 * (size_t)i + k], d);
                    s = d + s;
                    if (std::isfinite(d) && d != 0.0f) worst = std::max(worst, std::fabs((double)s) / (std::ldexp(1.0, -23) * std::fabs((double)d)));
                    else if (std::isfinite(d) && s != 0.0f) worst = INFINITY;
                }
        }
        for (int k = 0; k < 3; ++k) keys[3 * (size_t)i + k] = live ? (u64)idx[k] * slots + (u64)(3 * (size_t)i + k) : inert;
    }
    std::printf("live %d\n", n_live);
    std::stable_sort(keys.begin(), keys.end());

    // the run pass: the payload of every sorted slot is recomputed from its row, then every run is summed as a wave sums it
    std::vector<float> tv(keys.size() * 3, 0.0f), ta(keys.size() * (size_t)(C > 0 ? C : 1), 0.0f);
    for (size_t s = 0; s < keys.size() && keys[s] < inert; ++s) {
        const u64 slot = keys[s] % slots;
        const size_t i = (size_t)(slot / 3);
        const float b = bary[slot];
        if (has_g) {
            float d[3];
            mesh_grad_dpts(&pts[3 * i], &closest[3 * i], g[i], d);
            for (int c = 0; c < 3; ++c) tv[s * 3 + c] = mesh_grad_vert_term(b, d[c]);
        }
        for (int c = 0; c < C; ++c) ta[s * C + c] = mesh_grad_attr_term(b, ga[i * C + c]);
    }
    std::vector<float> dverts((size_t)V * 3, 0.0f), dattr((size_t)V * C, 0.0f);
    for (size_t lo = 0; lo < keys.size() && keys[lo] < inert;) {
        const u64 vert = keys[lo] / slots;
        size_t hi = lo;
        while (hi < keys.size() && keys[hi] / slots == vert) ++hi;
        if (has_g) for (int c = 0; c < 3; ++c) dverts[vert * 3 + c] = wave_sum(tv, lo, hi - lo, 3, c);
        for (int c = 0; c < C; ++c) dattr[vert * C + c] = wave_sum(ta, lo, hi - lo, C, c);
        lo = hi;
    }
    if (has_g) { print("dpts", dpts); print("dverts", dverts); }
    print("dattr", dattr);
    if (identity) {
        std::printf("identity %.3f\n", worst);
        if (!(worst <= 8.0)) { std::printf("identity violated\n"); return 1; }
    }
    return 0;
}

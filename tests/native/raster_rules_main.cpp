// A stand-alone CPU program around csrc/ra_raster_rules.hpp (built plain and with -fsanitize=address,undefined by
// tests/test_oracle_raster.py).  On seeded random and lattice-aligned meshes it asserts
//   - the complementarity lemma: for every edge shared by two faces with opposite orientation and every sample point, both faces
//     evaluate the same bits of E; with equal sigma exactly one edge clause holds, with opposite sigma both or neither;
//   - coverage: the lattice-aligned grid (vertices exactly on pixel centres, varying w) owns n x n pixels exactly once;
//   - the depth rule's order independence: folding a pixel's samples with raster_closer in ascending, descending and shuffled face
//     order gives the same face and the same bits of (u, v, zw), duplicated faces (equal zw) included.
#include "ra_raster_rules.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double rnd() {          // uniform [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

struct Mesh { std::vector<float> pos; std::vector<int> faces; };
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

// an n x n quad grid over the pixels first .. first + n; jitter == 0: vertices exactly on pixel centres.  fold: every third row of
// vertices is pulled back over its neighbour, which makes back-facing faces and silhouette edges
static Mesh grid(int n, int first, int H, int W, double jitter, bool fold, bool flip_diagonals) {
    Mesh m;
    for (int j = 0; j <= n; ++j)
        for (int i = 0; i <= n; ++i) {
            const float w = jitter == 0.0 ? 1.0f + 0.25f * (float)((3 * i + 5 * j) % 4) : (float)(0.5 + 1.5 * rnd());
            double x = (2.0 * (first + i) + 1.0) / W - 1.0, y = (2.0 * (first + (fold && j % 3 == 2 ? j - 1.6 : j)) + 1.0) / H - 1.0;
            x += jitter * (rnd() - 0.5) * 2.0 / W; y += jitter * (rnd() - 0.5) * 2.0 / H;
            const float fx = (float)x, fy = (float)y;
            m.pos.insert(m.pos.end(), {fx * w, fy * w, 0.125f * w * (float)((i + 2 * j) % 3 - 1), w});
        }
    auto id = [n](int i, int j) { return j * (n + 1) + i; };
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            const int a = id(i, j), b = id(i + 1, j), c = id(i, j + 1), d = id(i + 1, j + 1);
            if (flip_diagonals && (i + j) % 2) m.faces.insert(m.faces.end(), {a, b, d, a, d, c});
            else m.faces.insert(m.faces.end(), {a, b, c, b, d, c});
        }
    return m;
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

struct Totals { long long edges = 0, samples = 0, silhouettes = 0, pixels = 0; };

static int check_mesh(const Mesh& m, int H, int W, int expect_once, bool lemma, Totals& t) {
    const int F = (int)m.faces.size() / 3;
    std::vector<RasterFace> rec(F);
    for (int f = 0; f < F; ++f) {
        const int* i = &m.faces[3 * f];
        raster_setup(&m.pos[4 * i[0]], &m.pos[4 * i[1]], &m.pos[4 * i[2]], i[0], i[1], i[2], H, W, rec[f]);
    }
    // edge k of a face is opposite corner k: it runs from corner k + 1 to corner k + 2
    std::map<std::pair<int, int>, std::vector<std::pair<int, int>>> edges;
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < 3; ++k) {
            const int a = m.faces[3 * f + (k + 1) % 3], b = m.faces[3 * f + (k + 2) % 3];
            edges[{std::min(a, b), std::max(a, b)}].push_back({f, k});
        }
    for (const auto& e : edges) {
        if (!lemma || e.second.size() != 2) continue;
        const int fa = e.second[0].first, ka = e.second[0].second, fb = e.second[1].first, kb = e.second[1].second;
        const RasterFace &A = rec[fa], &B = rec[fb];
        if (!(A.flags & RASTER_VALID) || !(B.flags & RASTER_VALID)) continue;
        const bool na = (A.flags & (1 << ka)) != 0, nb = (B.flags & (1 << kb)) != 0;
        CHECK(na != nb, "faces %d and %d run their shared edge the same way: the grid is not consistently oriented", fa, fb);
        const bool back_a = (A.flags & RASTER_BACK) != 0, back_b = (B.flags & RASTER_BACK) != 0;
        ++t.edges;
        t.silhouettes += back_a != back_b;
        for (int iy = 0; iy < H; ++iy)
            for (int ix = 0; ix < W; ++ix) {
                const float px = raster_centre(ix, W), py = raster_centre(iy, H);
                const float Ea = raster_edge_at(A.c + 3 * ka, px, py), Eb = raster_edge_at(B.c + 3 * kb, px, py);
                CHECK(same_bits(Ea, Eb), "edge (%d, %d): faces %d and %d see different bits at pixel (%d, %d)", e.first.first, e.first.second, fa, fb, ix, iy);
                if (Ea != Ea) continue;
                const bool ca = raster_edge_clause(Ea, na == back_a), cb = raster_edge_clause(Eb, nb == back_b);
                if (back_a == back_b) CHECK(ca != cb, "edge (%d, %d) at pixel (%d, %d): clauses %d %d are not complementary", e.first.first, e.first.second, ix, iy, ca, cb);
                else CHECK(ca == cb, "silhouette edge (%d, %d) at pixel (%d, %d): clauses %d %d differ", e.first.first, e.first.second, ix, iy, ca, cb);
                ++t.samples;
            }
    }
    // coverage, and the depth rule in three orders
    std::vector<int> order(F);
    int once = 0;
    for (int iy = 0; iy < H; ++iy)
        for (int ix = 0; ix < W; ++ix) {
            const float px = raster_centre(ix, W), py = raster_centre(iy, H);
            int cover = 0, best_f[3] = {-1, -1, -1};
            RasterSample best[3] = {};
            for (int pass = 0; pass < 3; ++pass) {
                for (int f = 0; f < F; ++f) order[f] = pass == 1 ? F - 1 - f : f;
                if (pass == 2) for (int f = F - 1; f > 0; --f) std::swap(order[f], order[(int)(rnd() * (f + 1))]);
                for (int q = 0; q < F; ++q) {
                    RasterSample s;
                    if (!raster_sample(rec[order[q]], ix, iy, px, py, s)) continue;
                    cover += pass == 0;
                    if (raster_closer(s.zw, order[q], best[pass].zw, best_f[pass])) { best[pass] = s; best_f[pass] = order[q]; }
                }
                CHECK(best_f[pass] == best_f[0] && (best_f[0] < 0 || (same_bits(best[pass].u, best[0].u) && same_bits(best[pass].v, best[0].v) &&
                      same_bits(best[pass].zw, best[0].zw))), "pixel (%d, %d): order %d picks face %d, ascending order face %d", ix, iy, pass, best_f[pass], best_f[0]);
            }
            if (expect_once >= 0) CHECK(cover <= 1, "pixel (%d, %d) is owned by %d faces of the lattice grid", ix, iy, cover);
            once += cover == 1;
            ++t.pixels;
        }
    if (expect_once >= 0) CHECK(once == expect_once, "the lattice grid owns %d pixels once, expected %d", once, expect_once);
    return 0;
}

int main() {
    Totals t;
    for (int flip = 0; flip < 2; ++flip) {
        if (check_mesh(grid(8, 4, 16, 16, 0.0, false, flip != 0), 16, 16, 64, true, t)) return 1;
        if (check_mesh(grid(5, 1, 9, 7, 0.0, false, flip != 0), 9, 7, -1, true, t)) return 1;        // runs over the image's edge
    }
    for (int trial = 0; trial < 12; ++trial) {
        const int H = 17 + 3 * trial, W = 40 - 2 * trial;
        Mesh m = grid(6 + trial % 3, 2, H, W, 0.9, trial % 2 == 1, trial % 4 >= 2);
        if (trial % 3 == 0) {           // every face twice: equal zw, the face index decides
            const std::vector<int> f = m.faces;
            m.faces.insert(m.faces.end(), f.begin(), f.end());
            if (check_mesh(m, H, W, -1, false, t)) return 1;        // no edge has two faces any more: only the depth rule is checked
        } else if (check_mesh(m, H, W, -1, true, t)) return 1;
    }
    CHECK(t.silhouettes > 0 && t.edges > t.silhouettes, "the meshes hold no silhouette edge or nothing else");
    std::printf("raster rules ok: %lld shared edges (%lld silhouettes), %lld edge samples, %lld pixels in three orders\n", t.edges, t.silhouettes, t.samples,
                t.pixels);
    return 0;
}

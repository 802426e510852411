// Stand-alone check of csrc/ra_topo_rules.hpp on the CPU (built with -fsanitize=address,undefined -ffp-contract=off by
// tests/test_oracle_topology.py): the half-edge keys, the twin rule and the Taubin step that ra_topo.hip inlines, run the way the
// kernels run them, against the numpy restatement's values (tests/topology_ref.py), which arrive in a small binary file:
//   int32 F, V, E, C, iters; float alpha; faces[3F]; edge[3F]; twin[3F]; nbr_start[V+1]; nbr[2E]; values[V*C] f32; expected[V*C] f32;
//   then the Loop step: int32 n_max; table[2 (n_max+1)] f32; out_start[V+1]; out_he[3F]; ehe_start[E+1]; ehe[3F];
//   loop_expected[(V+E)*C] f32; child twin[12F]; child edge[12F]; child vert[12F]
#include "ra_topo_rules.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

template <typename T> static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: topo_rules_main cases.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    int n_cases = 0, bad = 0;
    for (;;) {
        int hdr[5];
        if (fread(hdr, sizeof(int), 5, f) != 5) break;
        const int F = hdr[0], V = hdr[1], E = hdr[2], C = hdr[3], iters = hdr[4];
        float alpha;
        std::vector<int> faces, edge, twin, nbr_start, nbr;
        std::vector<float> values, expected;
        if (fread(&alpha, sizeof(float), 1, f) != 1 || !read_vec(f, faces, (size_t)3 * F) || !read_vec(f, edge, (size_t)3 * F) || !read_vec(f, twin, (size_t)3 * F) ||
            !read_vec(f, nbr_start, (size_t)V + 1) || !read_vec(f, nbr, (size_t)2 * E) || !read_vec(f, values, (size_t)V * C) ||
            !read_vec(f, expected, (size_t)V * C)) { fprintf(stderr, "truncated case %d\n", n_cases); return 2; }
        const int n = 3 * F;
        // the build: keys, a stable sort, runs of equal keys
        std::vector<uint64_t> keys(n);
        for (int h = 0; h < n; ++h) keys[h] = topo_edge_key(faces[h], faces[topo_next(h)]);
        std::vector<int> order(n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return keys[a] < keys[b]; });
        std::vector<int> start;
        for (int i = 0; i < n; ++i) if (i == 0 || keys[order[i]] != keys[order[i - 1]]) start.push_back(i);
        if ((int)start.size() != E) { printf("case %d: E %d, expected %d\n", n_cases, (int)start.size(), E); ++bad; }
        start.push_back(n);
        for (int e = 0; e + 1 < (int)start.size(); ++e) {
            const int s = start[e], count = start[e + 1] - s;
            for (int i = s; i < s + count; ++i) {
                const int h = order[i], p = topo_twin_pos(i, s, count), tw = p >= 0 ? order[p] : -count;
                if (edge[h] != e || twin[h] != tw) { printf("case %d: half-edge %d: edge %d twin %d, expected %d %d\n", n_cases, h, e, tw, edge[h], twin[h]); ++bad; }
                if (topo_key_min(keys[h]) > topo_key_max(keys[h]) || topo_prev(topo_next(h)) != h || topo_next(h) / 3 != h / 3) { printf("case %d: key or ring of %d\n", n_cases, h); ++bad; }
            }
        }
        // smoothing: 2 x iters Jacobi passes between two buffers
        std::vector<float> a = values, b(values.size());
        for (int pass = 0; pass < 2 * iters; ++pass) {
            const float c = taubin_coeff(alpha, pass & 1);
            for (int v = 0; v < V; ++v)
                for (int ch = 0; ch < C; ++ch) {
                    float s = 0.0f;
                    for (int k = nbr_start[v]; k < nbr_start[v + 1]; ++k) s = s + a[(size_t)nbr[k] * C + ch];
                    b[(size_t)v * C + ch] = taubin_step(a[(size_t)v * C + ch], s, taubin_inv(nbr_start[v + 1] - nbr_start[v]), c);
                }
            a.swap(b);
        }
        if (std::memcmp(a.data(), expected.data(), a.size() * sizeof(float)) != 0) { printf("case %d: the smoothed rows differ from the restatement\n", n_cases); ++bad; }
        // one Loop step: the table, the positions in ascending half-edge order, the child's index arithmetic
        int n_max = 0;
        std::vector<float> table, loop_expected;
        std::vector<int> out_start, out_he, ehe_start, ehe, ctwin, cedge, cvert;
        if (fread(&n_max, sizeof(int), 1, f) != 1 || !read_vec(f, table, (size_t)2 * (n_max + 1)) || !read_vec(f, out_start, (size_t)V + 1) || !read_vec(f, out_he, (size_t)n) ||
            !read_vec(f, ehe_start, (size_t)E + 1) || !read_vec(f, ehe, (size_t)n) || !read_vec(f, loop_expected, (size_t)(V + E) * C) || !read_vec(f, ctwin, (size_t)4 * n) ||
            !read_vec(f, cedge, (size_t)4 * n) || !read_vec(f, cvert, (size_t)4 * n)) { fprintf(stderr, "truncated Loop part of case %d\n", n_cases); return 2; }
        for (int k = 1; k <= n_max; ++k) {
            float w, b;
            loop_weights(k, &w, &b);
            const float got[2] = {w, b};
            for (int j = 0; j < 2; ++j) {
                const float want = table[2 * k + j];
                if (!(std::nextafterf(want, -1e30f) <= got[j] && got[j] <= std::nextafterf(want, 1e30f))) { printf("case %d: weight %d of n = %d: %.9g, expected %.9g\n", n_cases, j, k, got[j], want); ++bad; }
            }
        }
        std::vector<float> sub((size_t)(V + E) * C);
        auto X = [&](int v, int ch) { return values[(size_t)v * C + ch]; };
        for (int ch = 0; ch < C; ++ch) {
            for (int v = 0; v < V; ++v) {
                const int s = out_start[v], e = out_start[v + 1];
                bool open = false;
                for (int k = s; k < e; ++k) open = open || twin[out_he[k]] < 0;
                float acc = 0.0f;
                for (int k = s; k < e; ++k) {
                    const int h = out_he[k];
                    const float x = X(faces[h], ch), xn = X(faces[topo_next(h)], ch);
                    float c = open ? 0.0f : loop_vert_inner(x, xn, table[2 * (e - s)], table[2 * (e - s) + 1]);
                    if (twin[h] < 0) c = c + loop_vert_open(x, xn);
                    const int tp = twin[topo_prev(h)];
                    if (tp >= 0 && twin[topo_prev(tp)] < 0) c = c + loop_vert_open(X(faces[tp], ch), X(faces[topo_prev(tp)], ch));
                    acc = acc + c;
                }
                sub[(size_t)v * C + ch] = acc;
            }
            for (int e = 0; e < E; ++e) {
                float acc = 0.0f;
                for (int k = ehe_start[e]; k < ehe_start[e + 1]; ++k) {
                    const int h = ehe[k];
                    const float x = X(faces[h], ch);
                    acc = acc + (twin[h] >= 0 ? loop_edge_inner(x, X(faces[topo_prev(h)], ch)) : loop_edge_open(x, X(faces[topo_next(h)], ch), -twin[h]));
                }
                sub[(size_t)(V + e) * C + ch] = acc;
            }
        }
        if (std::memcmp(sub.data(), loop_expected.data(), sub.size() * sizeof(float)) != 0) { printf("case %d: the subdivided rows differ from the restatement\n", n_cases); ++bad; }
        for (int h = 0; h < n; ++h) {
            const int pv = topo_prev(h), tw = twin[h], tp = twin[pv];
            const int i0 = 3 * h, i1 = 3 * h + 1, i2 = 3 * h + 2, i3 = 3 * n + h;
            const bool ok = ctwin[i0] == child_twin0(tw) && ctwin[i1] == i3 && ctwin[i2] == child_twin2(tp) && ctwin[i3] == i1 &&
                            cedge[i0] == child_edge0(edge[h], h, tw) && cedge[i1] == 2 * E + h && cedge[i2] == child_edge2(edge[pv], pv, tp) && cedge[i3] == 2 * E + h &&
                            cvert[i0] == faces[h] && cvert[i1] == V + edge[h] && cvert[i2] == V + edge[pv] && cvert[i3] == V + edge[pv];
            if (!ok) { printf("case %d: the children of half-edge %d\n", n_cases, h); ++bad; }
        }
        ++n_cases;
    }
    fclose(f);
    if (bad || n_cases == 0) { printf("topo rules FAILED: %d mismatches in %d cases\n", bad, n_cases); return 1; }
    printf("topo rules ok: %d cases\n", n_cases);
    return 0;
}

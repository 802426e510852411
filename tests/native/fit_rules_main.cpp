// Stand-alone check of csrc/ra_fit_rules.hpp on the CPU (built with -fsanitize=address,undefined -ffp-contract=off by
// tests/test_oracle_icp.py): the operator row, the normals, the ICP row rules and the AdamUniform step that ra_fit.hip inlines, run the
// way the kernels run them, against the numpy restatement's values (tests/fit_ref.py), which arrive in a small binary file.  Per case:
//   int32 V, F, C, NN, n, NA, steps; float lambda, dist_th, angle_th, lr, b1, b2;
//   nbr_start[V+1]; nbr[NN]; faces[3F]; out_start[V+1]; out_he[3F];
//   x[V*C]; want_apply[V*C];  verts[3V]; want_fn[3F]; want_area[F]; want_vn[3V]                                           (f32)
//   p[3n]; closest[3n]; d2[n] (f32); face[n] (int32); n0[3n]; n1[3F] (f32); want_keep[n] (bytes); count (f64); want_grad[3n] (f32)
//   param[NA]; grads[steps*NA]; want_param[NA]; want_g1[NA]; want_g2 (f32)
#include "ra_fit_rules.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

template <typename T> static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T> static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: fit_rules_main cases.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    int n_cases = 0, bad = 0;
    for (;;) {
        int hdr[7];
        if (fread(hdr, sizeof(int), 7, f) != 7) break;
        const int V = hdr[0], F = hdr[1], C = hdr[2], NN = hdr[3], n = hdr[4], NA = hdr[5], steps = hdr[6];
        float par[6];
        std::vector<int> nbr_start, nbr, faces, out_start, out_he, face;
        std::vector<float> x, want_apply, verts, want_fn, want_area, want_vn, p, closest, d2, n0, n1, want_grad, param, grads, want_param, want_g1;
        std::vector<unsigned char> want_keep;
        double count = 0.0;
        float want_g2 = 0.0f;
        if (fread(par, sizeof(float), 6, f) != 6 || !read_vec(f, nbr_start, (size_t)V + 1) || !read_vec(f, nbr, (size_t)NN) || !read_vec(f, faces, (size_t)3 * F) ||
            !read_vec(f, out_start, (size_t)V + 1) || !read_vec(f, out_he, (size_t)3 * F) || !read_vec(f, x, (size_t)V * C) || !read_vec(f, want_apply, (size_t)V * C) ||
            !read_vec(f, verts, (size_t)3 * V) || !read_vec(f, want_fn, (size_t)3 * F) || !read_vec(f, want_area, (size_t)F) || !read_vec(f, want_vn, (size_t)3 * V) ||
            !read_vec(f, p, (size_t)3 * n) || !read_vec(f, closest, (size_t)3 * n) || !read_vec(f, d2, (size_t)n) || !read_vec(f, face, (size_t)n) ||
            !read_vec(f, n0, (size_t)3 * n) || !read_vec(f, n1, (size_t)3 * F) || !read_vec(f, want_keep, (size_t)n) || fread(&count, sizeof(double), 1, f) != 1 ||
            !read_vec(f, want_grad, (size_t)3 * n) || !read_vec(f, param, (size_t)NA) || !read_vec(f, grads, (size_t)steps * NA) || !read_vec(f, want_param, (size_t)NA) ||
            !read_vec(f, want_g1, (size_t)NA) || fread(&want_g2, sizeof(float), 1, f) != 1) { fprintf(stderr, "truncated case %d\n", n_cases); return 2; }
        const double lambda = (double)par[0];
        // the operator: one (vertex, channel) at a time, neighbours ascending, the vertex itself skipped
        std::vector<float> got(x.size());
        for (int v = 0; v < V; ++v)
            for (int ch = 0; ch < C; ++ch) {
                double s = 0.0;
                int deg = 0;
                for (int k = nbr_start[v]; k < nbr_start[v + 1]; ++k) {
                    if (nbr[k] == v) continue;
                    ++deg;
                    s = s + (double)x[(size_t)nbr[k] * C + ch];
                }
                got[(size_t)v * C + ch] = (float)fit_diffuse((double)x[(size_t)v * C + ch], s, deg, lambda);
            }
        if (!same(got, want_apply)) { printf("case %d: M x differs from the restatement\n", n_cases); ++bad; }
        // normals
        std::vector<float> fn((size_t)3 * F), area((size_t)F), vn((size_t)3 * V);
        auto raw = [&](int t, double* nn) { fit_face_normal_raw(&verts[3 * faces[3 * t]], &verts[3 * faces[3 * t + 1]], &verts[3 * faces[3 * t + 2]], nn); };
        for (int t = 0; t < F; ++t) {
            double nn[3];
            raw(t, nn);
            fit_face_normal(nn, &fn[3 * t]);
            area[t] = fit_face_area(&verts[3 * faces[3 * t]], &verts[3 * faces[3 * t + 1]], &verts[3 * faces[3 * t + 2]]);
        }
        for (int v = 0; v < V; ++v) {
            double sum[3] = {0.0, 0.0, 0.0};
            for (int k = out_start[v]; k < out_start[v + 1]; ++k) {
                double nn[3];
                raw(out_he[k] / 3, nn);
                for (int i = 0; i < 3; ++i) sum[i] = sum[i] + nn[i];
            }
            fit_vert_normal(sum, &vn[3 * v]);
        }
        if (!same(fn, want_fn) || !same(area, want_area) || !same(vn, want_vn)) { printf("case %d: normals or areas differ from the restatement\n", n_cases); ++bad; }
        // ICP rows
        std::vector<float> grad((size_t)3 * n, 0.0f);
        for (int i = 0; i < n; ++i) {
            const bool keep = face[i] >= 0 && face[i] < F && fit_icp_keep(d2[i], par[1], &n1[3 * face[i]], &n0[3 * i], par[2]);
            if (keep != (want_keep[i] != 0)) { printf("case %d: row %d kept %d\n", n_cases, i, (int)keep); ++bad; }
            if (keep && count > 0.0)
                for (int k = 0; k < 3; ++k) grad[3 * i + k] = fit_icp_grad((double)p[3 * i + k] - (double)closest[3 * i + k], count);
        }
        if (!same(grad, want_grad)) { printf("case %d: the ICP gradient differs from the restatement\n", n_cases); ++bad; }
        // AdamUniform
        std::vector<float> g1((size_t)NA, 0.0f);
        float g2 = 0.0f;
        for (int t = 1; t <= steps; ++t) {
            const float* g = &grads[(size_t)(t - 1) * NA];
            double m = 0.0;
            for (int i = 0; i < NA; ++i) m = std::fabs((double)g[i]) > m ? std::fabs((double)g[i]) : m;
            g2 = fit_adam_moment(g2, m * m, (double)par[5]);
            const double c1 = 1.0 - fit_pow((double)par[4], t), c2 = 1.0 - fit_pow((double)par[5], t);
            for (int i = 0; i < NA; ++i) {
                g1[i] = fit_adam_moment(g1[i], (double)g[i], (double)par[4]);
                param[i] = fit_adam_param(param[i], g1[i], g2, (double)par[3], c1, c2);
            }
        }
        if (!same(param, want_param) || !same(g1, want_g1) || std::memcmp(&g2, &want_g2, sizeof(float)) != 0) { printf("case %d: AdamUniform differs from the restatement\n", n_cases); ++bad; }
        ++n_cases;
    }
    fclose(f);
    if (bad || n_cases == 0) { printf("fit rules FAILED: %d mismatches in %d cases\n", bad, n_cases); return 1; }
    printf("fit rules ok: %d cases\n", n_cases);
    return 0;
}

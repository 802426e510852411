// Stand-alone check of csrc/ra_cloth_rules.hpp on the CPU (built plain and with -fsanitize=address,undefined -ffp-contract=off by
// tests/test_oracle_physx.py): every per-element rule that ra_cloth.hip inlines, instantiated in float — the kernels' arithmetic — and
// in double, on cases that arrive in a small binary file (the fixture's, written by the test), on the build rules of every face of
// those cases, and on four constructed elements (a flat hinge, a folded hinge, a rigidly
// rotated face, a face scaled by 2).  Per case of the file:
//   int32 V, F, H, B; float thickness, mu, lambda, bending; double tol_es, tol_eb, tol_gs, tol_gb;
//   faces[3F]; hinge[4H] = (face0, face1, k0, k1) (int32); dm_inv[4F]; area[F]; x[B*V*3] (f32)
// The float results are gathered the way the kernels gather them (face corners in ascending half-edge order, hinge slots in ascending
// (hinge, slot) order is the same set here: the order differs from the device only in rounding) and written to `out`:
//   per case: double e_stretch[B], e_bending[B]; float grad_stretch[B*V*3], grad_bending[B*V*3]
// and the float and double evaluations must agree: |sum32 - sum64| <= tol_e |sum64|, max |g32 - g64| <= tol_g max |g64|.
#include "ra_cloth_rules.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

template <typename T> static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static const double EPS = 1.1920928955078125e-07;
static int bad = 0;
static void expect(bool ok, const char* what, double a = 0, double b = 0) {
    if (!ok) { printf("FAILED: %s (%.9g vs %.9g)\n", what, a, b); ++bad; }
}

template <typename T> struct Eval {
    std::vector<double> es, eb;
    std::vector<T> gs, gb;
};

template <typename T>
static void evaluate(int V, int F, int H, int B, const float* par, const std::vector<int>& faces, const std::vector<int>& hinge, const std::vector<float>& dm_inv,
                     const std::vector<float>& area, const std::vector<float>& x32, Eval<T>& o) {
    std::vector<T> x(x32.begin(), x32.end());
    o.es.assign(B, 0.0); o.eb.assign(B, 0.0);
    o.gs.assign((size_t)B * V * 3, (T)0); o.gb.assign((size_t)B * V * 3, (T)0);
    for (int b = 0; b < B; ++b) {
        const T* xb = x.data() + (size_t)b * V * 3;
        T* gs = o.gs.data() + (size_t)b * V * 3;
        T* gb = o.gb.data() + (size_t)b * V * 3;
        for (int f = 0; f < F; ++f) {
            const int* v = &faces[3 * f];
            const T m[4] = {(T)dm_inv[4 * f], (T)dm_inv[4 * f + 1], (T)dm_inv[4 * f + 2], (T)dm_inv[4 * f + 3]};
            T g[9];
            o.es[b] += (double)cloth_stretch<T>(xb + 3 * v[0], xb + 3 * v[1], xb + 3 * v[2], m, (T)area[f], (T)par[0], (T)par[1], (T)par[2], g);
            for (int k = 0; k < 3; ++k)
                for (int c = 0; c < 3; ++c) gs[3 * v[k] + c] = gs[3 * v[k] + c] + g[3 * k + c];
        }
        for (int h = 0; h < H; ++h) {
            const int f0 = hinge[4 * h], f1 = hinge[4 * h + 1], k0 = hinge[4 * h + 2], k1 = hinge[4 * h + 3];
            const T* a[3] = {xb + 3 * faces[3 * f0], xb + 3 * faces[3 * f0 + 1], xb + 3 * faces[3 * f0 + 2]};
            const T* c[3] = {xb + 3 * faces[3 * f1], xb + 3 * faces[3 * f1 + 1], xb + 3 * faces[3 * f1 + 2]};
            const T asum = (T)(area[f0] + area[f1]);        // a float sum, as the build makes it
            T g[18];
            o.eb[b] += (double)cloth_bending<true, T>(a, c, k0, k1, asum, (T)par[3], g);
            for (int k = 0; k < 3; ++k)
                for (int d = 0; d < 3; ++d) {
                    gb[3 * faces[3 * f0 + k] + d] = gb[3 * faces[3 * f0 + k] + d] + g[3 * k + d];
                    gb[3 * faces[3 * f1 + k] + d] = gb[3 * faces[3 * f1 + k] + d] + g[9 + 3 * k + d];
                }
        }
    }
}

template <typename A, typename Bt> static double grad_err(const std::vector<A>& a, const std::vector<Bt>& b) {
    double worst = 0.0, scale = 0.0;
    for (size_t i = 0; i < a.size(); ++i) {
        const double d = std::fabs((double)a[i] - (double)b[i]), s = std::fabs((double)b[i]);
        worst = d > worst ? d : worst;
        scale = s > scale ? s : scale;
    }
    return scale > 0.0 ? worst / scale : worst;
}

// The build rules (cloth_face_area, cloth_mass_share, cloth_dm_inv) on every face of a case, the corners taken from its first row of
// positions and the material triangle from flattening that face in double: float against double on the same float inputs.  Bounds:
// a cross product or a 2 x 2 determinant of differences is off by a few eps of |u| |v|, and |u| |v| / |u x v| stays below 8 on the test
// meshes (their slimmest triangles, the fan's, have an angle of 0.15 rad) -> 64 eps; a share is two roundings of the same area -> 4 eps.
static void build_rules(int F, const std::vector<int>& faces, const std::vector<float>& x, int n_case) {
    double worst_area = 0.0, worst_share = 0.0, worst_inv = 0.0;
    const float density = 426 * 0.00047f;
    for (int f = 0; f < F; ++f) {
        const float* p[3] = {&x[3 * faces[3 * f]], &x[3 * faces[3 * f + 1]], &x[3 * faces[3 * f + 2]]};
        double pd[3][3];
        for (int k = 0; k < 3; ++k) for (int c = 0; c < 3; ++c) pd[k][c] = (double)p[k][c];
        const float a32 = cloth_face_area<float>(p[0], p[1], p[2]);
        const double a64 = cloth_face_area<double>(pd[0], pd[1], pd[2]);
        worst_area = std::fmax(worst_area, std::fabs(a32 - a64) / a64);
        const float s32 = cloth_mass_share<float>(density, a32);
        const double s64 = cloth_mass_share<double>((double)density, (double)a32);
        worst_share = std::fmax(worst_share, std::fabs(s32 - s64) / s64);
        // corner 2 at the origin, corner 0 on +x
        double u[3], v[3];
        for (int c = 0; c < 3; ++c) { u[c] = pd[0][c] - pd[2][c]; v[c] = pd[1][c] - pd[2][c]; }
        const double lu = std::sqrt(cloth_dot(u, u)), bx = cloth_dot(u, v) / lu, by = std::sqrt(std::fmax(cloth_dot(v, v) - bx * bx, 0.0));
        const float m0[2] = {(float)lu, 0.0f}, m1[2] = {(float)bx, (float)by}, m2[2] = {0.0f, 0.0f};
        const double d0[2] = {m0[0], m0[1]}, d1[2] = {m1[0], m1[1]}, d2[2] = {0.0, 0.0};
        float dm[4], inv[4];
        double dmd[4], invd[4];
        cloth_dm_inv<float>(m0, m1, m2, dm, inv);
        cloth_dm_inv<double>(d0, d1, d2, dmd, invd);
        double scale = 0.0, diff = 0.0;
        for (int k = 0; k < 4; ++k) {
            scale = std::fmax(scale, std::fabs(invd[k]));
            diff = std::fmax(diff, std::fabs(inv[k] - invd[k]));
            expect((double)dm[k] == dmd[k], "Dm: differences of float inputs at the origin are exact", dm[k], dmd[k]);
        }
        worst_inv = std::fmax(worst_inv, diff / scale);
    }
    printf("case %d: build rules, float vs double: area %.2e, mass share %.2e, Dm_inv %.2e\n", n_case, worst_area, worst_share, worst_inv);
    expect(worst_area <= 64 * EPS, "face area, float against double", worst_area, 64 * EPS);
    expect(worst_share <= 4 * EPS, "mass share, float against double", worst_share, 4 * EPS);
    expect(worst_inv <= 64 * EPS, "Dm_inv, float against double", worst_inv, 64 * EPS);
}

static void constructed() {
    const float mu = 23569.0f, lambda = 44392.0f, th = 0.00047f, bend = 3.96e-5f;
    // a flat hinge: two coplanar triangles over the edge (1,0,0) -> (0,1,0): energy and gradient exactly 0
    {
        const float p[4][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {1, 1, 0}};
        const float* a[3] = {p[0], p[1], p[2]};
        const float* b[3] = {p[2], p[1], p[3]};
        float g[18];
        const float e = cloth_bending<true, float>(a, b, 1, 0, 1.0f, bend, g);     // a[1] = (1,0,0) -> b[0] = (0,1,0)
        expect(e == 0.0f, "flat hinge: energy 0", e, 0);
        for (int k = 0; k < 18; ++k) expect(g[k] == 0.0f, "flat hinge: gradient 0", g[k], 0);
    }
    // a hinge folded almost shut (theta = +-(pi - 0.01)): float against double, and theta squared keeps the energy even in the sign
    for (int sign = -1; sign <= 1; sign += 2) {
        const double t = 0.01;       // the second face lies back over the first
        const float q[4][3] = {{0, 0, 0}, {1, 0, 0}, {0.3f, 1, 0}, {0.4f, (float)std::cos(t), (float)(sign * std::sin(t))}};
        const float* a[3] = {q[0], q[1], q[2]};
        const float* b[3] = {q[1], q[0], q[3]};
        double qd[4][3];
        for (int i = 0; i < 4; ++i) for (int c = 0; c < 3; ++c) qd[i][c] = (double)q[i][c];
        const double* ad[3] = {qd[0], qd[1], qd[2]};
        const double* bd[3] = {qd[1], qd[0], qd[3]};
        float g[18];
        double gd[18];
        const float e = cloth_bending<true, float>(a, b, 0, 0, 1.0f, bend, g);      // a[0] = (0,0,0) -> b[0] = (1,0,0)
        const double ed = cloth_bending<true, double>(ad, bd, 0, 0, 1.0, (double)bend, gd);
        expect(ed > 0.4 * bend && std::fabs(e - ed) <= 64 * EPS * ed, "folded hinge: energy", e, ed);
        const std::vector<float> gv(g, g + 18);
        const std::vector<double> gdv(gd, gd + 18);
        const double ge = grad_err(gv, gdv);
        expect(ge <= 256 * EPS, "folded hinge: gradient", ge, 256 * EPS);
    }
    // a rest face, rotated rigidly and translated: the stretch energy stays at its rest value (0 up to the det + eps quirk) to fp32 rounding
    {
        const float m0[2] = {0.7f, 0.0f}, m1[2] = {0.2f, 0.5f}, m2[2] = {0.0f, 0.0f};
        float inv[4];
        cloth_dm_inv<float>(m0, m1, m2, (float*)nullptr, inv);
        const double cz = std::cos(0.7), sz = std::sin(0.7), cx = std::cos(-1.1), sx = std::sin(-1.1);
        float r[3][3];
        const double rest[3][2] = {{0.7, 0.0}, {0.2, 0.5}, {0.0, 0.0}};
        for (int i = 0; i < 3; ++i) {
            const double x = cz * rest[i][0] - sz * rest[i][1], y = sz * rest[i][0] + cz * rest[i][1];
            r[i][0] = (float)(x + 0.3); r[i][1] = (float)(cx * y + 1.0); r[i][2] = (float)(sx * y - 2.0);
        }
        const float flat[3][3] = {{0.7f, 0, 0}, {0.2f, 0.5f, 0}, {0, 0, 0}};
        const float e0 = cloth_stretch<float>(flat[0], flat[1], flat[2], inv, 0.175f, th, mu, lambda, (float*)nullptr);
        const float e1 = cloth_stretch<float>(r[0], r[1], r[2], inv, 0.175f, th, mu, lambda, (float*)nullptr);
        const double bound = 0.175 * th * (2.0 * mu + lambda) * (16 * EPS) * (16 * EPS);      // G off by at most a few eps of C ~ 1 in every entry
        expect(std::fabs((double)e1 - (double)e0) <= bound && e0 <= bound, "rotated face: stretch energy at rest", e1, e0);
    }
    // the same face scaled by 2: F = 2 I, G = 1.5 I, psi = 4.5 mu + 4.5 lambda
    {
        const float m0[2] = {0.7f, 0.0f}, m1[2] = {0.2f, 0.5f}, m2[2] = {0.0f, 0.0f};
        float inv[4];
        cloth_dm_inv<float>(m0, m1, m2, (float*)nullptr, inv);
        const float big[3][3] = {{1.4f, 0, 0}, {0.4f, 1.0f, 0}, {0, 0, 0}};
        float g[9];
        const float e = cloth_stretch<float>(big[0], big[1], big[2], inv, 0.175f, th, mu, lambda, g);
        const double want = 0.175 * (double)th * (4.5 * mu + 4.5 * lambda);
        expect(std::fabs(e - want) <= 32 * EPS * want, "scaled face: stretch energy", e, want);
        for (int c = 0; c < 3; ++c) expect(std::fabs((double)g[c] + g[3 + c] + g[6 + c]) <= 1e-6 * std::fabs((double)g[0]) + 1e-12, "scaled face: gradient sums to 0");
    }
    // inertia: float against double
    {
        const float xn[3] = {0.31f, -0.2f, 0.05f}, xc[3] = {0.3f, -0.21f, 0.04f}, vc[3] = {0.1f, 0.2f, -0.3f}, acc[3] = {0, -9.81f, 0};
        const double xnd[3] = {xn[0], xn[1], xn[2]}, xcd[3] = {xc[0], xc[1], xc[2]}, vcd[3] = {vc[0], vc[1], vc[2]}, accd[3] = {acc[0], acc[1], acc[2]};
        float g[3];
        double gd[3];
        const float dt = 1.0f / 30.0f;
        const float v = cloth_inertia<float>(xn, xc, vc, 0.01f, dt, acc, g);
        const double vd = cloth_inertia<double>(xnd, xcd, vcd, (double)0.01f, (double)dt, accd, gd);
        expect(std::fabs(v - vd) <= 64 * EPS * vd, "dynamic term: value", v, vd);
        for (int c = 0; c < 3; ++c) expect(std::fabs(g[c] - gd[c]) <= 64 * EPS * std::fabs(gd[1]), "dynamic term: gradient", g[c], gd[c]);
        expect(cloth_gravity<float>(9.81f, 0.5f, 2.0f) == 9.81f, "gravity: g mass y");
    }
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: cloth_rules_main cases.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!f || !out) { perror("open"); return 2; }
    int n_cases = 0;
    for (;;) {
        int hdr[4];
        if (fread(hdr, sizeof(int), 4, f) != 4) break;
        const int V = hdr[0], F = hdr[1], H = hdr[2], B = hdr[3];
        float par[4];
        double tol[4];
        std::vector<int> faces, hinge;
        std::vector<float> dm_inv, area, x;
        if (fread(par, sizeof(float), 4, f) != 4 || fread(tol, sizeof(double), 4, f) != 4 || !read_vec(f, faces, (size_t)3 * F) || !read_vec(f, hinge, (size_t)4 * H) ||
            !read_vec(f, dm_inv, (size_t)4 * F) || !read_vec(f, area, (size_t)F) || !read_vec(f, x, (size_t)B * V * 3)) {
            fprintf(stderr, "truncated case %d\n", n_cases);
            return 2;
        }
        Eval<float> a;
        Eval<double> d;
        evaluate<float>(V, F, H, B, par, faces, hinge, dm_inv, area, x, a);
        evaluate<double>(V, F, H, B, par, faces, hinge, dm_inv, area, x, d);
        for (int b = 0; b < B; ++b) {
            expect(std::fabs(a.es[b] - d.es[b]) <= tol[0] * std::fabs(d.es[b]), "stretch energy, float against double", a.es[b], d.es[b]);
            expect(std::fabs(a.eb[b] - d.eb[b]) <= tol[1] * std::fabs(d.eb[b]), "bending energy, float against double", a.eb[b], d.eb[b]);
        }
        const double gs = grad_err(a.gs, d.gs), gb = grad_err(a.gb, d.gb);
        expect(gs <= tol[2], "stretch gradient, float against double", gs, tol[2]);
        expect(gb <= tol[3], "bending gradient, float against double", gb, tol[3]);
        printf("case %d: V %d F %d H %d B %d: float vs double gradient error stretch %.2e bending %.2e\n", n_cases, V, F, H, B, gs, gb);
        build_rules(F, faces, x, n_cases);
        fwrite(a.es.data(), sizeof(double), B, out);
        fwrite(a.eb.data(), sizeof(double), B, out);
        fwrite(a.gs.data(), sizeof(float), a.gs.size(), out);
        fwrite(a.gb.data(), sizeof(float), a.gb.size(), out);
        ++n_cases;
    }
    fclose(f);
    fclose(out);
    constructed();
    if (bad) { printf("cloth rules: %d failures\n", bad); return 1; }
    printf("cloth rules ok: %d cases\n", n_cases);
    return 0;
}

// Stand-alone CPU program around csrc/ra_winding_tri.hpp (the per-pair function the winding kernel of ra_winding.hip inlines): the
// same IEEE fp32 operations on the host.  On seeded (point, triangle) pairs — faces of 1 mm .. 0.3 m at 0, 1 and 100 m from the origin,
// slivers (a vertex collinear with the other two up to fp32 rounding), repeated vertices, points from 1e-4 to 1e3 m away — it checks
//   1. no NaN for a point that is not a vertex of the face, and NaN for one that is;
//   2. |Omega| <= 2 pi (as fp32 rounds it);
//   3. antisymmetry: swapping two vertices negates the value, within twice the bound of 4;
//   4. agreement with a long-double evaluation of the same function — Omega_0 = 2 atan2(|det|, den) on long-double unit vectors,
//      folded with the reference's eps — within
//        tol = 32 U + 32 U (1 + cond) / hypot(det, den),      U = 2^-23,  cond = L1 L2 n_min / (n0 n1 n2),
//      L1, L2 the two longest edges (whatever the vertex order), n_i the distances of p to the vertices, n_min the least.  Where it comes from: every
//      difference of two inputs is one rounding of its own size, so det = (ab x bc) . d_min / (n0 n1 n2) carries about 16 roundings
//      of size cond, den about 16 of size 1, Omega_0 = 2 atan2(|det|, den) moves by 2 (|d det| + |d den|) / hypot(det, den), and the
//      tangent, the root and the arctangent add a few units of U of 2 pi.  hypot -> 0 is p on an edge's line, where the solid angle
//      jumps.  Where the long-double determinant is itself within 16 U cond of zero its SIGN is rounding noise (a sliver, p in the
//      face's plane: the solid angle jumps there), so only |Omega| is compared, and an exact fp32 zero is accepted (det == 0 gives 0).
// Built by tests/test_oracle_winding.py with -fsanitize=address,undefined and -ffp-contract=off.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <initializer_list>

#include "ra_winding_tri.hpp"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double uni() {       // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}
static float range(double lo, double hi) { return (float)(lo + (hi - lo) * uni()); }

struct Exact { long double omega, det, den, cond; };

static Exact exact(const float p[3], const float a[3], const float b[3], const float c[3]) {
    long double d[3][3], n[3], u[3][3];
    for (int k = 0; k < 3; ++k) { d[0][k] = (long double)a[k] - p[k]; d[1][k] = (long double)b[k] - p[k]; d[2][k] = (long double)c[k] - p[k]; }
    for (int i = 0; i < 3; ++i) {
        n[i] = sqrtl(d[i][0] * d[i][0] + d[i][1] * d[i][1] + d[i][2] * d[i][2]);
        for (int k = 0; k < 3; ++k) u[i][k] = d[i][k] / n[i];
    }
    const long double n_min = fminl(n[0], fminl(n[1], n[2]));
    Exact e;
    e.det = u[0][0] * (u[1][1] * u[2][2] - u[1][2] * u[2][1]) - u[0][1] * (u[1][0] * u[2][2] - u[1][2] * u[2][0]) + u[0][2] * (u[1][0] * u[2][1] - u[1][1] * u[2][0]);
    auto dot = [&](int i, int j) { return u[i][0] * u[j][0] + u[i][1] * u[j][1] + u[i][2] * u[j][2]; };
    e.den = 1 + dot(0, 1) + dot(1, 2) + dot(2, 0);
    const long double t = tanl(atan2l(fabsl(e.det), e.den) / 2);            // tan(Omega_0 / 4), Omega_0 / 2 in [0, pi]
    e.omega = e.det == 0 ? 0 : copysignl(4 * atanl(sqrtl(t * t + (long double)WIND_EPS)), e.det);
    long double ab = 0, bc = 0, ca = 0;
    for (int k = 0; k < 3; ++k) {
        ab += ((long double)b[k] - a[k]) * ((long double)b[k] - a[k]); bc += ((long double)c[k] - b[k]) * ((long double)c[k] - b[k]);
        ca += ((long double)a[k] - c[k]) * ((long double)a[k] - c[k]);
    }
    const long double l_min = sqrtl(fminl(ab, fminl(bc, ca)));
    e.cond = (l_min > 0 ? sqrtl(ab) * sqrtl(bc) * sqrtl(ca) / l_min : fmaxl(ab, fmaxl(bc, ca))) * n_min / (n[0] * n[1] * n[2]);
    return e;
}

int main() {
    const double U = std::ldexp(1.0, -23);
    const float TWO_PI = 6.2831855f;
    const int FACES = 6000, POINTS = 24;
    double worst = 0, worst_anti = 0, worst_plain = 0;
    long pairs = 0, noise = 0, on_vertex = 0, degenerate = 0;
    for (int f = 0; f < FACES; ++f) {
        const double off = f % 3 == 0 ? 0.0 : (f % 3 == 1 ? 1.0 : 100.0);
        const float centre[3] = {range(-off, off), range(-off, off), range(-off, off)};
        const double size = std::pow(10.0, -3.0 + 2.5 * uni());
        float a[3], b[3], c[3];
        for (int k = 0; k < 3; ++k) { a[k] = centre[k] + range(-size, size); b[k] = centre[k] + range(-size, size); c[k] = centre[k] + range(-size, size); }
        const int kind = f % 8;
        if (kind == 5) for (int k = 0; k < 3; ++k) c[k] = a[k] + range(-1.5, 2.5) * (b[k] - a[k]);      // collinear to fp32 rounding: a sliver
        if (kind == 6) for (int k = 0; k < 3; ++k) b[k] = a[k];                                          // a repeated vertex
        if (kind == 7) for (int k = 0; k < 3; ++k) b[k] = c[k] = a[k];                                   // a point
        degenerate += kind >= 5;
        for (int i = 0; i < POINTS; ++i) {
            const double reach = std::pow(10.0, -4.0 + 7.0 * (i + uni()) / POINTS);      // 1e-4 .. 1e3 m from the face's centre
            float p[3];
            double dir[3], len = 0;
            for (int k = 0; k < 3; ++k) { dir[k] = 2 * uni() - 1; len += dir[k] * dir[k]; }
            for (int k = 0; k < 3; ++k) p[k] = (float)(centre[k] + reach * dir[k] / std::sqrt(len > 0 ? len : 1));
            if (i == 7) for (int k = 0; k < 3; ++k) p[k] = (f % 2 ? c[k] : a[k]);
            bool hits = false;
            for (const float* v : {a, b, c}) hits = hits || (v[0] == p[0] && v[1] == p[1] && v[2] == p[2]);
            const float w = winding_tri(p, a, b, c);
            ++pairs;
            if (hits) {
                ++on_vertex;
                if (!std::isnan(w)) { std::printf("FAILED face %d point %d: a point on a vertex gives %.9g, not NaN\n", f, i, w); return 1; }
                continue;
            }
            if (std::isnan(w)) { std::printf("FAILED face %d point %d: NaN off every vertex\n", f, i); return 1; }
            if (!(std::fabs(w) <= TWO_PI)) { std::printf("FAILED face %d point %d: |Omega| = %.9g above 2 pi\n", f, i, w); return 1; }
            const Exact e = exact(p, a, b, c);
            const double hyp = (double)hypotl(e.det, e.den);
            const double tol = 32 * U + 32 * U * (1 + (double)e.cond) / hyp;       // hyp == 0: inf, nothing is claimed on an edge's line
            const bool noisy = (double)fabsl(e.det) <= 16 * U * (double)e.cond;
            noise += noisy;
            const float swapped[3] = {winding_tri(p, b, a, c), winding_tri(p, a, c, b), winding_tri(p, c, b, a)};
            for (float s : swapped) {
                if (std::isnan(s)) { std::printf("FAILED face %d point %d: NaN off every vertex (swapped)\n", f, i); return 1; }
                const double anti = noisy ? ((s == 0.f || w == 0.f) ? 0 : std::fabs(std::fabs((double)s) - std::fabs((double)w))) : std::fabs((double)s + (double)w);
                if (anti > 2 * tol) { std::printf("FAILED face %d point %d: not antisymmetric: %.9g vs %.9g (allowed %.3g)\n", f, i, w, s, 2 * tol); return 1; }
                if (std::isfinite(tol)) worst_anti = std::fmax(worst_anti, anti / (2 * tol));
            }
            const double err = noisy ? (w == 0.f ? 0 : std::fabs(std::fabs((double)w) - (double)fabsl(e.omega))) : std::fabs((double)w - (double)e.omega);
            if (err > tol) { std::printf("FAILED face %d point %d: %.9g vs long double %.9Lg, |diff| %.3g > %.3g (cond %.3Lg)\n", f, i, w, e.omega, err, tol, e.cond); return 1; }
            if (std::isfinite(tol)) worst = std::fmax(worst, err / tol);
            worst_plain = std::fmax(worst_plain, err);
        }
    }
    std::printf("%ld pairs (%ld on degenerate faces, %ld on a vertex: NaN, %ld with a determinant whose sign is rounding noise)\n", pairs, degenerate * POINTS, on_vertex, noise);
    std::printf("|Omega - long double| at most %.3f of its bound (largest %.3e); antisymmetry at most %.3f of its bound\n", worst, worst_plain, worst_anti);
    std::printf("winding arithmetic ok\n");
    return 0;
}

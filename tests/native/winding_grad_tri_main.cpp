// Stand-alone CPU program around csrc/ra_winding_grad_tri.hpp (the per-pair function the kernels of ra_winding_grad.hip inline): the
// same IEEE fp32 operations on the host.  On winding_tri_main.cpp's seeded (point, triangle) pairs — faces of 1 mm .. 0.3 m at 0, 1
// and 100 m from the origin, slivers, repeated vertices, points from 1e-4 to 1e3 m away — it checks
//   1. the value: the bits of winding_tri, on every pair (NaN for NaN);
//   2. a point on a vertex gives a NaN gradient; a point off every vertex and off every edge (the computed 1 + cos of each edge
//      positive) gives a finite one; det == 0 gives exactly 0;
//   3. agreement with a long-double evaluation of the same closed form,
//        g = k(T) sum_e (x cross y) (|x| + |y|) / (|x| |y| (|x| |y| + x.y)),   k = (1 + T) sqrt(T) / ((1 + T + eps) sqrt(T + eps)),
//      within   tol = 32 U k S + |g| (4 U + r_k),   U = 2^-23, where
//        S   = sum_e B_e (1 + 1 / (1 + c_e)),  B_e = |x| |y - x| (1 / |x| + 1 / |y|) / (|x| |y| (1 + c_e)): an edge's term bounded
//              without the sine of its cross product.  Every difference of two inputs is one rounding of its own size, so a cross
//              product x cross (y - x) is off by a few U |x| |y - x|, a weight (i_x + i_y) i_x i_y / (1 + c_e) by a few U of itself
//              plus the cosine's few U over (1 + c_e): some 16 roundings per term, 32 U with the sum's;
//        r_k = eps / (T + eps) * (1 + T) / (4 t) * 32 U (1 + cond) / hypot(det, den): k moves with t by dk / k = eps / (T + eps) dt / t,
//              t = tan(Omega_0 / 4) by dt = (1 + T) / 4 dOmega_0, and dOmega_0 is winding_tri_main.cpp's bound of the value (cond as
//              there).  It matters for small and distant faces only (T below eps), where k is far from 1.
//      Where the long-double determinant is within 16 U cond of zero its SIGN is rounding noise, and with it the gradient's: the
//      two are compared up to that sign, and an exact fp32 zero is accepted.  Where the long-double 1 + c_e of an edge is below
//      64 U the point sits on that edge's segment up to rounding and nothing is claimed.
// Built by tests/test_oracle_winding_grad.py with -fsanitize=address,undefined and -ffp-contract=off.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <initializer_list>

#include "ra_winding_grad_tri.hpp"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double uni() {       // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}
static float range(double lo, double hi) { return (float)(lo + (hi - lo) * uni()); }

struct Exact { long double g[3], det, den, cond, k, t, S, e_min; };

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
    e.t = tanl(atan2l(fabsl(e.det), e.den) / 2);            // tan(Omega_0 / 4), Omega_0 / 2 in [0, pi]
    const long double T = e.t * e.t, eps = (long double)WIND_EPS;
    e.k = (1 + T) * e.t / ((1 + T + eps) * sqrtl(T + eps));
    long double sum[3] = {0, 0, 0};
    e.S = 0; e.e_min = 2;
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3;
        const long double* x = d[i]; const long double* y = d[j];
        const long double cr[3] = {x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]};
        const long double one_c = 1 + dot(i, j);
        const long double w = (n[i] + n[j]) / (n[i] * n[j] * (n[i] * n[j] * one_c));
        for (int k = 0; k < 3; ++k) sum[k] += cr[k] * w;
        long double len = 0;
        for (int k = 0; k < 3; ++k) len += (y[k] - x[k]) * (y[k] - x[k]);
        e.S += n[i] * sqrtl(len) * w * (1 + 1 / one_c);
        e.e_min = fminl(e.e_min, one_c);
    }
    for (int k = 0; k < 3; ++k) e.g[k] = e.det == 0 ? 0 : e.k * sum[k];
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
    const int FACES = 6000, POINTS = 24;
    double worst = 0, worst_rel = 0;
    long pairs = 0, noise = 0, on_vertex = 0, degenerate = 0, on_edge = 0, flat = 0, compared = 0;
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
            const WindGrad g = winding_grad_tri(p, a, b, c);
            const float w = winding_tri(p, a, b, c);
            ++pairs;
            if (std::memcmp(&w, &g.omega, 4) != 0 && !(std::isnan(w) && std::isnan(g.omega))) {
                std::printf("FAILED face %d point %d: the value %.9g is not winding_tri's %.9g\n", f, i, g.omega, w); return 1;
            }
            const float gv[3] = {g.gx, g.gy, g.gz};
            if (hits) {
                ++on_vertex;
                if (!(std::isnan(gv[0]) && std::isnan(gv[1]) && std::isnan(gv[2]))) { std::printf("FAILED face %d point %d: a point on a vertex gives a gradient that is not NaN\n", f, i); return 1; }
                continue;
            }
            const Exact e = exact(p, a, b, c);
            if (std::isnan(gv[0]) || std::isnan(gv[1]) || std::isnan(gv[2])) {
                // the rule: the computed 1 + cos of an edge is not positive.  Off the segment (well off, in long double) that is a failure
                if (e.e_min > 64 * U) { std::printf("FAILED face %d point %d: NaN gradient off every vertex and edge (least 1 + cos %.3Lg)\n", f, i, e.e_min); return 1; }
                ++on_edge;
                continue;
            }
            if (!(std::isfinite(gv[0]) && std::isfinite(gv[1]) && std::isfinite(gv[2]))) {
                if (e.e_min > 64 * U) { std::printf("FAILED face %d point %d: infinite gradient off every vertex and edge\n", f, i); return 1; }
                ++on_edge;
                continue;
            }
            if (e.e_min <= 64 * U) { ++on_edge; continue; }
            const bool zero = gv[0] == 0.f && gv[1] == 0.f && gv[2] == 0.f;
            if (w == 0.f) {      // det == 0 as computed: value 0 and gradient 0
                ++flat;
                if (!zero) { std::printf("FAILED face %d point %d: det == 0 with a gradient that is not 0\n", f, i); return 1; }
            }
            const double hyp = (double)hypotl(e.det, e.den);
            const bool noisy = (double)fabsl(e.det) <= 16 * U * (double)e.cond;
            noise += noisy;
            const long double T = e.t * e.t, eps = (long double)WIND_EPS;
            const double r_k = (double)(eps / (T + eps) * (1 + T) / (4 * e.t)) * 32 * U * (1 + (double)e.cond) / hyp;
            double norm = 0, err_plus = 0, err_minus = 0;
            for (int k = 0; k < 3; ++k) {
                norm = std::fmax(norm, (double)fabsl(e.g[k]));
                err_minus = std::fmax(err_minus, std::fabs((double)gv[k] - (double)e.g[k]));
                err_plus = std::fmax(err_plus, std::fabs((double)gv[k] + (double)e.g[k]));
            }
            const double tol = 32 * U * (double)(e.k * e.S) + norm * (4 * U + r_k);
            const double err = noisy ? (zero ? 0 : std::fmin(err_minus, err_plus)) : err_minus;
            if (!(err <= tol)) {      // tol may be inf or NaN on an edge's line (hyp == 0, t == 0): nothing is claimed there
                if (std::isfinite(tol)) {
                    std::printf("FAILED face %d point %d: gradient (%.9g %.9g %.9g) vs long double (%.9Lg %.9Lg %.9Lg), |diff| %.3g > %.3g (cond %.3Lg, k %.3Lg)\n",
                                f, i, gv[0], gv[1], gv[2], e.g[0], e.g[1], e.g[2], err, tol, e.cond, e.k);
                    return 1;
                }
                continue;
            }
            ++compared;
            if (std::isfinite(tol) && tol > 0) worst = std::fmax(worst, err / tol);
            if (norm > 0 && !noisy) worst_rel = std::fmax(worst_rel, err / norm);
        }
    }
    std::printf("%ld pairs (%ld on degenerate faces, %ld on a vertex: NaN, %ld on an edge's segment up to rounding, %ld with det == 0: gradient 0, "
                "%ld with a determinant whose sign is rounding noise), %ld compared\n", pairs, degenerate * POINTS, on_vertex, on_edge, flat, noise, compared);
    std::printf("|gradient - long double| at most %.3f of its bound (largest relative to its own size, off the noisy pairs: %.3e)\n", worst, worst_rel);
    std::printf("winding gradient arithmetic ok\n");
    return 0;
}

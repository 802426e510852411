// Stand-alone CPU program around csrc/ra_mesh_tri.hpp (the arithmetic the query kernel of ra_mesh.hip inlines): the same IEEE fp32
// operations on the host.  It checks, on seeded random leaves built the way mesh_leaves_kernel builds them (32 faces, the box of their
// vertices widened by MESH_BOX_PAD of its largest coordinate):
//   1. the lemma the sweep's exactness rests on — for every point and every face of a leaf,
//        m_box_near(p, box) <= computed d2(p, face) <= m_box_far(p, box),
//      and the computed closest point lies inside the widened box;
//   2. no NaN, barycentrics that sum to 1 within 4 * 2^-23 and are >= -4 * 2^-23, closest = sum bary v within 8 * 2^-23 of the largest
//      coordinate, d2 = |p - closest|^2 within 4 * 2^-23 — also for collinear faces, repeated vertices and slivers;
//   3. against a float64 dense barycentric grid: the computed distance is within the grid's spacing (plus fp32 rounding) of it.
// Built by tests/test_oracle_mesh_distance.py with -fsanitize=address,undefined and -ffp-contract=off.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>

#include "ra_mesh_tri.hpp"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double uni() {       // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}
static float range(double lo, double hi) { return (float)(lo + (hi - lo) * uni()); }

struct Tri { float a[3], b[3], c[3]; };

static int fail(const char* what, int leaf, int face, int point, double x, double y) {
    std::printf("FAILED %s: leaf %d face %d point %d: %.9g vs %.9g\n", what, leaf, face, point, x, y);
    return 1;
}

int main() {
    const double U = std::ldexp(1.0, -23);
    const int LEAVES = 400, FACES = 32, POINTS = 48;
    double worst_q = 0, worst_sum = 0, worst_bary = 0, worst_d2 = 0, worst_slack = 1e30, worst_grid = 0;
    long pairs = 0, degenerate = 0;
    for (int l = 0; l < LEAVES; ++l) {
        // a leaf somewhere in space: offset 0, 1 or 100 m, faces of 1 mm .. 0.3 m
        const double off = l % 3 == 0 ? 0.0 : (l % 3 == 1 ? 1.0 : 100.0);
        const float centre[3] = {range(-off, off), range(-off, off), range(-off, off)};
        const double size = std::pow(10.0, -3.0 + 2.5 * uni());
        std::vector<Tri> tris(FACES);
        for (int f = 0; f < FACES; ++f) {
            Tri& t = tris[f];
            for (int k = 0; k < 3; ++k) {
                t.a[k] = centre[k] + range(-size, size);
                t.b[k] = centre[k] + range(-size, size);
                t.c[k] = centre[k] + range(-size, size);
            }
            const int kind = (l * FACES + f) % 8;
            if (kind == 5) for (int k = 0; k < 3; ++k) t.c[k] = t.a[k] + range(-1.5, 2.5) * (t.b[k] - t.a[k]);     // collinear to fp32 rounding: a sliver
            if (kind == 6) for (int k = 0; k < 3; ++k) (f % 3 == 0 ? t.b[k] : (f % 3 == 1 ? t.c[k] : t.a[k])) = (f % 3 == 2 ? t.b[k] : t.a[k]);      // a repeated vertex
            if (kind == 7 && f % 2) for (int k = 0; k < 3; ++k) t.b[k] = t.c[k] = t.a[k];                          // a point
            degenerate += kind >= 5;
        }
        float box[6] = {3e38f, 3e38f, 3e38f, -3e38f, -3e38f, -3e38f};
        for (const Tri& t : tris)
            for (int k = 0; k < 3; ++k) {
                box[k] = fminf(box[k], fminf(fminf(t.a[k], t.b[k]), t.c[k]));
                box[3 + k] = fmaxf(box[3 + k], fmaxf(fmaxf(t.a[k], t.b[k]), t.c[k]));
            }
        float m = 0.f;
        for (int k = 0; k < 3; ++k) m = fmaxf(m, fmaxf(fabsf(box[k]), fabsf(box[3 + k])));
        const float pad = m * MESH_BOX_PAD;
        for (int k = 0; k < 3; ++k) { box[k] -= pad; box[3 + k] += pad; }
        for (int i = 0; i < POINTS; ++i) {
            // points inside the leaf, just outside it, a leaf away and a kilometre away; every fourth one ON a vertex or an edge midpoint
            const double reach = i % 4 == 0 ? size : (i % 4 == 1 ? 3 * size : (i % 4 == 2 ? 1.0 : 1000.0));
            float p[3] = {centre[0] + range(-reach, reach), centre[1] + range(-reach, reach), centre[2] + range(-reach, reach)};
            if (i % 8 == 4) for (int k = 0; k < 3; ++k) p[k] = tris[i % FACES].b[k];
            if (i % 8 == 0) for (int k = 0; k < 3; ++k) p[k] = 0.5f * (tris[i % FACES].a[k] + tris[i % FACES].c[k]);
            const float near = m_box_near(p, box), far = m_box_far(p, box);
            for (int f = 0; f < FACES; ++f) {
                const Tri& t = tris[f];
                const MeshHit h = mesh_closest_tri(p, t.a, t.b, t.c);
                ++pairs;
                if (!(std::isfinite(h.d2) && std::isfinite(h.x) && std::isfinite(h.y) && std::isfinite(h.z) && std::isfinite(h.u) && std::isfinite(h.v) && std::isfinite(h.w)))
                    return fail("a non-finite output", l, f, i, h.d2, h.u);
                if (!(near <= h.d2)) return fail("box bound above the computed d2", l, f, i, near, h.d2);
                if (!(h.d2 <= far)) return fail("computed d2 above the far-corner bound", l, f, i, h.d2, far);
                const float q[3] = {h.x, h.y, h.z};
                for (int k = 0; k < 3; ++k) {
                    if (!(q[k] >= box[k] && q[k] <= box[3 + k])) return fail("closest point outside the widened box", l, f, i, q[k], box[k]);
                    const double exact_lo = fmin(fmin(t.a[k], t.b[k]), t.c[k]), exact_hi = fmax(fmax(t.a[k], t.b[k]), t.c[k]);
                    const double out = fmax(exact_lo - q[k], q[k] - exact_hi);      // how far it left the triangle's exact box, in units of the pad
                    if (pad > 0 && out > 0) worst_slack = fmin(worst_slack, pad / out);
                }
                if (i % 8 == 4 && f == i % FACES && h.d2 != 0.f) return fail("a point on a vertex with d2 != 0", l, f, i, h.d2, 0);
                // identities in double on the fp32 outputs
                double rebuilt[3], own = 0, coord = 0;
                for (int k = 0; k < 3; ++k) {
                    rebuilt[k] = (double)h.u * t.a[k] + (double)h.v * t.b[k] + (double)h.w * t.c[k];
                    coord = fmax(coord, fmax(fabs(t.a[k]), fmax(fabs(t.b[k]), fabs(t.c[k]))));
                    own += ((double)p[k] - q[k]) * ((double)p[k] - q[k]);
                }
                for (int k = 0; k < 3; ++k) worst_q = fmax(worst_q, fabs(rebuilt[k] - q[k]) / (U * coord));
                worst_sum = fmax(worst_sum, fabs((double)h.u + h.v + h.w - 1) / U);
                worst_bary = fmin(worst_bary, fmin(h.u, fmin(h.v, h.w)) / U);
                if (h.d2 > 0) worst_d2 = fmax(worst_d2, fabs(own - h.d2) / (U * h.d2));
                else if (own != 0) return fail("d2 = 0 off the closest point", l, f, i, own, 0);
                // a dense barycentric grid in double (every 16th pair: it is 300 points per pair)
                if (pairs % 16 == 0) {
                    const int G = 24;
                    double best = 1e300, edge = 0;
                    for (int a = 0; a <= G; ++a)
                        for (int b = 0; a + b <= G; ++b) {
                            const double v = (double)a / G, w = (double)b / G, u = 1 - v - w;
                            double d = 0;
                            for (int k = 0; k < 3; ++k) { const double x = u * t.a[k] + v * t.b[k] + w * t.c[k] - p[k]; d += x * x; }
                            best = fmin(best, d);
                        }
                    for (int k = 0; k < 3; ++k) edge = fmax(edge, fmax(fabs((double)t.b[k] - t.a[k]), fmax(fabs((double)t.c[k] - t.a[k]), fabs((double)t.c[k] - t.b[k]))));
                    const double spacing = std::sqrt(3.0) * edge / G, dist = std::sqrt((double)h.d2), gd = std::sqrt(best);
                    const double fp = 64 * U * (coord + std::sqrt(own));      // fp32 rounding of the computed point and distance
                    if (dist > gd + fp) return fail("computed distance above the grid minimum", l, f, i, dist, gd);
                    if (dist < gd - spacing - fp) return fail("computed distance below the grid minimum by more than the spacing", l, f, i, dist, gd);
                    if (spacing > 0) worst_grid = fmax(worst_grid, (gd - dist) / spacing);
                }
            }
        }
    }
    std::printf("%ld pairs (%ld on degenerate faces): box bound <= d2 <= far bound for all; ", pairs, degenerate * POINTS);
    if (worst_slack > 1e29) std::printf("no closest point left its triangle's exact box\n");
    else std::printf("a closest point left its triangle's exact box by at most 1/%.1f of the pad\n", worst_slack);
    std::printf("|closest - sum bary v| %.2f units (8)  |sum bary - 1| %.2f (4)  min bary %.2f (-4)  |own - d2| %.2f (4)  grid %.2f of a spacing\n",
                worst_q, worst_sum, worst_bary, worst_d2, worst_grid);
    if (worst_q > 8 || worst_sum > 4 || worst_bary < -4 || worst_d2 > 4 || worst_slack < 2) { std::printf("FAILED an identity bound\n"); return 1; }
    std::printf("mesh arithmetic ok\n");
    return 0;
}

// Stand-alone CPU program around csrc/ra_raycast_tri.hpp (the arithmetic the ray-casting kernel of ra_raycast.hip inlines): the same
// IEEE fp32 operations on the host.  On seeded random leaves built the way mesh_leaves_kernel builds them (32 faces, the box of their
// vertices widened by MESH_BOX_PAD of its largest coordinate; 0, 1 and 100 m from the origin; faces of 1 mm to 0.3 m, a share of
// slivers and repeated vertices) and seeded rays (aimed at a face from 3 sizes, 1 m and 1 km away; grazing; in a face's plane; far
// and unrelated; d = 0) it checks:
//   1. part (a) of the lemma: every face's own box (ray_face_box) lies inside its leaf's stored box, component by component;
//   2. THE LEMMA: for every pair raycast_hit accepts, the computed slab test of the leaf box and of a group box (the leaf's box merged
//      with its neighbour's) passes, with entry bounds lo_t(group) <= lo_t(leaf) <= computed t;
//   3. the guard and the slab clause cost no clean hit: against a float64 evaluation of the reference's formula, no pair that float64
//      accepts with margins above the classification margin (tests/raycast_ref.py: min(|u|, |v|, |1 - u - v|, |t|) and |det| / (|d||N|)
//      above 10 x the largest fp32 error measured here on the well-conditioned hits of the pair's class — the leaf's distance from the
//      origin x the ray's reach, since u and v of a 1 mm face seen from 1 km have no fp32 digit to lose —) is rejected — counted
//      separately for the guard and for the clause, both must be 0 — and no such pair's reference predicate flips in fp32.  Faces
//      generated as slivers or with repeated vertices have no clean hits (their N is rounding noise), and neither has a pair whose
//      1e-8 / |det| is above the margin: there the reference's eps has moved its own u, v, t away from the geometry by more than that;
//      those pairs are COUNTED instead — accepted, rejected by the guard, rejected by the slab clause — and the count is printed: it is
//      what clause (3) costs against the reference where the reference's own t has left the face;
//   4. a ray with d = 0 hits nothing, and no accepted pair has a non-finite u, v or t.
// Built by tests/test_oracle_raycast.py with -fsanitize=address,undefined and -ffp-contract=off.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>

#include "ra_raycast_tri.hpp"

static uint64_t g_state;
static double uni() {       // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}
static float range(double lo, double hi) { return (float)(lo + (hi - lo) * uni()); }

struct Tri { float a[3], b[3], c[3]; int kind; };
struct Ref { double u, v, t, cosang, eps_share; bool hit; };

// the reference's formula in float64 on the fp32 inputs
static Ref reference(const float o[3], const float d[3], const Tri& f) {
    double e1[3], e2[3], a0[3], n[3], da0[3];
    for (int k = 0; k < 3; ++k) { e1[k] = (double)f.b[k] - f.a[k]; e2[k] = (double)f.c[k] - f.a[k]; a0[k] = (double)o[k] - f.a[k]; }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1]; n[1] = e1[2] * e2[0] - e1[0] * e2[2]; n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double det = d[0] * n[0] + d[1] * n[1] + d[2] * n[2], invdet = 1.0 / -(det + 1e-8);
    da0[0] = a0[1] * d[2] - a0[2] * d[1]; da0[1] = a0[2] * d[0] - a0[0] * d[2]; da0[2] = a0[0] * d[1] - a0[1] * d[0];
    Ref r;
    r.u = (da0[0] * e2[0] + da0[1] * e2[1] + da0[2] * e2[2]) * invdet;
    r.v = -(da0[0] * e1[0] + da0[1] * e1[1] + da0[2] * e1[2]) * invdet;
    r.t = (a0[0] * n[0] + a0[1] * n[1] + a0[2] * n[2]) * invdet;
    const double dn = std::sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]) * std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    r.cosang = dn > 0 ? std::fabs(det) / dn : 0.0;
    r.eps_share = det != 0 ? std::fabs(1e-8 / det) : 1e300;       // how far the reference's eps moves its own u, v, t, relatively
    r.hit = r.t >= 0 && r.u >= 0 && r.v >= 0 && r.u + r.v <= 1;
    return r;
}

static int fail(const char* what, int leaf, int face, int ray, double x, double y) {
    std::printf("FAILED %s: leaf %d face %d ray %d: %.9g vs %.9g\n", what, leaf, face, ray, x, y);
    return 1;
}

static void leaf_box(const std::vector<Tri>& tris, float box[6]) {
    for (int k = 0; k < 3; ++k) { box[k] = 3e38f; box[3 + k] = -3e38f; }
    for (const Tri& t : tris)
        for (int k = 0; k < 3; ++k) {
            box[k] = fminf(box[k], fminf(fminf(t.a[k], t.b[k]), t.c[k]));
            box[3 + k] = fmaxf(box[3 + k], fmaxf(fmaxf(t.a[k], t.b[k]), t.c[k]));
        }
    float m = 0.f;
    for (int k = 0; k < 3; ++k) m = fmaxf(m, fmaxf(fabsf(box[k]), fabsf(box[3 + k])));
    const float pad = m * MESH_BOX_PAD;
    for (int k = 0; k < 3; ++k) { box[k] -= pad; box[3 + k] += pad; }
}

int main() {
    const int LEAVES = 300, FACES = 32, RAYS = 48, WELL_KINDS = 5;
    const double WELL = 0.1;
    double measured[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, margin[9];       // per class: the leaf's offset (0, 1, 100 m) x the ray's reach (3 sizes, 1 m, 1 km)
    long clean_of[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    long pairs = 0, accepted = 0, ref_hits = 0, clean = 0, guard_lost = 0, clause_lost = 0, flips = 0, guard_rejects = 0, clause_rejects = 0, phantom = 0;
    long eps_hits = 0, eps_guard = 0, eps_clause = 0, eps_kept = 0;      // hits decided but for the reference's eps: what the departure costs
    double tightest = 1e300;
    for (int pass = 0; pass < 2; ++pass) {       // pass 0 measures the fp32 error, pass 1 (the same seed) counts against the margin
        g_state = 0x9e3779b97f4a7c15ull;
        float prev_box[6] = {0, 0, 0, 0, 0, 0};
        for (int l = 0; l < LEAVES; ++l) {
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
                t.kind = (l * FACES + f) % 8;
                if (t.kind == 5) for (int k = 0; k < 3; ++k) t.c[k] = t.a[k] + range(-1.5, 2.5) * (t.b[k] - t.a[k]);     // collinear to fp32 rounding: a sliver
                if (t.kind == 6) for (int k = 0; k < 3; ++k) (f % 3 == 0 ? t.b[k] : (f % 3 == 1 ? t.c[k] : t.a[k])) = (f % 3 == 2 ? t.b[k] : t.a[k]);      // a repeated vertex
                if (t.kind == 7 && f % 2) for (int k = 0; k < 3; ++k) t.b[k] = t.c[k] = t.a[k];                          // a point
            }
            float box[6], group[6];
            leaf_box(tris, box);
            for (int k = 0; k < 3; ++k) { group[k] = l ? fminf(box[k], prev_box[k]) : box[k]; group[3 + k] = l ? fmaxf(box[3 + k], prev_box[3 + k]) : box[3 + k]; }
            for (int k = 0; k < 6; ++k) prev_box[k] = box[k];
            for (const Tri& t : tris) {
                float fb[6];
                ray_face_box(t.a, t.b, t.c, fb);
                for (int k = 0; k < 3; ++k)
                    if (!(box[k] <= fb[k] && fb[3 + k] <= box[3 + k])) return fail("a face box outside its leaf box", l, (int)(&t - tris.data()), -1, fb[k], box[k]);
            }
            for (int i = 0; i < RAYS; ++i) {
                const Tri& aim = tris[i % FACES];
                float o[3], d[3], target[3];
                double b0 = 0.05 + 0.85 * uni(), b1 = 0.05 + (0.9 - b0) * uni();
                for (int k = 0; k < 3; ++k) target[k] = (float)((1 - b0 - b1) * aim.a[k] + b0 * aim.b[k] + b1 * aim.c[k]);
                const int kind = i % 6;
                const double reach = i % 3 == 0 ? 3 * size : (i % 3 == 1 ? 1.0 : 1000.0);
                if (kind <= 2) {                       // aimed at the interior of a face, d of any length
                    for (int k = 0; k < 3; ++k) o[k] = target[k] + range(-reach, reach);
                    const float s = range(0.2, 5.0);
                    for (int k = 0; k < 3; ++k) d[k] = (target[k] - o[k]) * s;
                } else if (kind == 3) {                // grazing: along an edge direction, a hair off the plane
                    for (int k = 0; k < 3; ++k) o[k] = target[k] - (float)reach * (aim.b[k] - aim.a[k]) + range(-1e-4, 1e-4) * (float)size;
                    for (int k = 0; k < 3; ++k) d[k] = target[k] - o[k];
                } else if (kind == 4) {                // in the face's plane, through it
                    for (int k = 0; k < 3; ++k) o[k] = aim.a[k] + 3.f * (aim.a[k] - target[k]);
                    for (int k = 0; k < 3; ++k) d[k] = target[k] - o[k];
                } else {                               // far and unrelated; every fourth of them d = 0
                    for (int k = 0; k < 3; ++k) { o[k] = centre[k] + range(-1000, 1000); d[k] = i % 24 == 5 ? 0.f : range(-1, 1); }
                }
                const int cls = (l % 3) * 3 + i % 3;
                const RayPre pre = ray_prepare(d);
                float lo_l, hi_l, lo_g, hi_g;
                ray_slab(o, pre, box, lo_l, hi_l);
                ray_slab(o, pre, group, lo_g, hi_g);
                const bool zero = d[0] == 0.f && d[1] == 0.f && d[2] == 0.f;
                for (int f = 0; f < FACES; ++f) {
                    const Tri& t = tris[f];
                    const RayTri r = raycast_tri(o, d, t.a, t.b, t.c);
                    const bool ref32 = raycast_ref_hit(r), guard = raycast_guard_ok(d, t.a, t.b, t.c, r.det);
                    const bool hit = raycast_hit(o, d, pre, t.a, t.b, t.c, r);
                    const Ref g = reference(o, d, t);
                    if (pass == 0) {
                        if (g.hit && g.cosang >= WELL && t.kind < WELL_KINDS)
                            measured[cls] = fmax(measured[cls], fmax(fmax(fabs(r.u - g.u), fabs(r.v - g.v)), fabs(r.t - g.t) / fmax(1.0, fabs(g.t))));
                        continue;
                    }
                    ++pairs;
                    ref_hits += ref32;
                    guard_rejects += ref32 && !guard;
                    clause_rejects += ref32 && guard && !hit;
                    if (hit) {
                        ++accepted;
                        if (zero) return fail("a hit of a ray with d = 0", l, f, i, r.t, 0);
                        if (!(std::isfinite(r.u) && std::isfinite(r.v) && std::isfinite(r.t))) return fail("a non-finite accepted pair", l, f, i, r.u, r.t);
                        if (!ray_slab_pass(lo_l, hi_l)) return fail("LEMMA: the leaf's slab test fails for an accepted pair", l, f, i, lo_l, hi_l);
                        if (!ray_slab_pass(lo_g, hi_g)) return fail("LEMMA: the group's slab test fails for an accepted pair", l, f, i, lo_g, hi_g);
                        if (!(lo_l <= r.t)) return fail("LEMMA: the leaf's entry bound above the computed t", l, f, i, lo_l, r.t);
                        if (!(lo_g <= lo_l && hi_g >= hi_l)) return fail("LEMMA: the group's interval inside the leaf's", l, f, i, lo_g, lo_l);
                        if (r.t > 0) tightest = fmin(tightest, (r.t - lo_l) / r.t);
                    }
                    const double m4 = fmin(fmin(fabs(g.u), fabs(g.v)), fmin(fabs(1 - g.u - g.v), fabs(g.t)));
                    const bool decided = m4 > margin[cls] && g.cosang > margin[cls] && g.eps_share <= margin[cls] && t.kind < WELL_KINDS;
                    if (decided && ref32 != g.hit) ++flips;
                    if (decided && g.hit) {
                        ++clean;
                        ++clean_of[cls];
                        guard_lost += !guard;
                        clause_lost += guard && !hit;
                    }
                    // a hit that is decided in every respect but one: the reference's eps has moved its own u, v, t by more than the margin
                    if (m4 > margin[cls] && g.cosang > margin[cls] && g.eps_share > margin[cls] && t.kind < WELL_KINDS && g.hit) {
                        ++eps_hits;
                        eps_guard += !guard;
                        eps_clause += guard && !hit;
                        eps_kept += hit;
                    }
                    phantom += ref32 && !g.hit && !hit;
                }
            }
        }
        if (pass == 0) for (int k = 0; k < 9; ++k) margin[k] = 10 * measured[k];
    }
    std::printf("%ld pairs: %ld pass the reference's test in fp32, %ld accepted (the guard rejects %ld, the slab clause %ld more; %ld of the rejected are no hits in float64)\n",
                pairs, ref_hits, accepted, guard_rejects, clause_rejects, phantom);
    std::printf("the lemma holds for every accepted pair; the tightest leaf entry bound is %.3g of t below t\n", tightest);
    for (int k = 0; k < 9; ++k)
        std::printf("  leaves %s, rays from %s: fp32 error on well-conditioned hits %.3e, margin %.3e, %ld clean hits\n", k / 3 == 0 ? "at the origin" : (k / 3 == 1 ? "1 m off" : "100 m off"),
                    k % 3 == 0 ? "3 sizes" : (k % 3 == 1 ? "1 m" : "1 km"), measured[k], margin[k], clean_of[k]);
    std::printf("%ld clean hits: the guard loses %ld, the clause loses %ld, %ld decided pairs flip in fp32\n", clean, guard_lost, clause_lost, flips);
    std::printf("the cost of the departure: %ld hits that only the reference's eps keeps from being clean (1e-8 / |det| above the margin): %ld accepted, the guard rejects %ld, "
                "the slab clause %ld\n", eps_hits, eps_kept, eps_guard, eps_clause);
    if (eps_kept + eps_guard + eps_clause != eps_hits) { std::printf("FAILED: the eps region does not add up\n"); return 1; }
    if (accepted < 1000 || clean < 1000) { std::printf("FAILED: too few hits to mean anything\n"); return 1; }
    if (guard_lost || clause_lost || flips) { std::printf("FAILED: a clean hit was lost\n"); return 1; }
    std::printf("raycast arithmetic ok\n");
    return 0;
}

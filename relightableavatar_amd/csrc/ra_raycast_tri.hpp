// The per-pair arithmetic of ra_raycast.hip as host + device functions: the reference's moller_trumbore (lib/utils/mesh_utils.py:
// 710-738) for ONE ray and ONE triangle, in named fp32 operations (ra_mesh_tri.hpp's m_mul / m_fma / m_div, contraction off), so
// that a (ray, face) pair has ONE result whatever kernel, loop or launch shape computes it, and a stand-alone CPU program
// (tests/native/raycast_tri_main.cpp) runs the same operations.
//
// raycast_tri, in the reference's order, its eps included:
//     E1 = b - a, E2 = c - a, N = E1 x E2, det = d . N, invdet = 1 / -(det + 1e-8),
//     A0 = o - a, DA0 = A0 x d, u = (DA0 . E2) invdet, v = -(DA0 . E1) invdet, t = (A0 . N) invdet.
// d is not normalised; t is in units of |d|.  Dot products are m_dot (fma(z, fma(x, mul(y)))), cross products fma(a, b, -mul(c, d)).
//
// CONTRACT of a hit (raycast_hit), three clauses:
//   (1) the reference's predicate, two-sided, no culling:  t >= 0, u >= 0, v >= 0, u + v <= 1.
//       It is NOT watertight on shared edges and vertices: the two faces of an edge round u, v independently, so a ray through the
//       edge may be accepted by both, by one or by neither.  The reference's per-triangle test has the same property.
//   (2) the grazing guard, the ONE departure from the reference:  no hit when
//           |det| <= RAY_GUARD * RAY_DET_ROUND * S,     S = sum_k |d_k| (|E1_i E2_j| + |E1_j E2_i|)   (i, j the other two axes).
//       RAY_DET_ROUND * S bounds the rounding of the det computation against the exact det of the fp32 inputs: a component of
//       E1, E2 carries one rounding (relative u = 2^-24), a product of two of them 2u, its mul or fma one more each, so a component
//       of N is off by at most 4u of |E1_i E2_j| + |E1_j E2_i|; the three roundings of m_dot add 3u of sum |d_k N_k|, which is no
//       larger than S.  7u S in all, to first order; 8u = 2^-21 is stated.  At or below that bound the SIGN of det — hence of t, u
//       and v — is not determined by the inputs: the ray may lie in the face's plane, the face may have no area, d may be 0
//       (S = 0: "at or below" rejects it).  There invdet is about +-1e8 and u, v, t are rounding noise, and the reference "hits" a
//       face the ray is nowhere near.  RAY_GUARD = 1 is the narrowest multiple with that meaning; the lemma below holds for any
//       guard, so nothing wider is needed.
//   (3) the slab clause:  the computed t lies in the computed ray interval of the face's OWN widened box,
//           lo_t(face box) <= t <= hi_t(face box)            (ray_slab below, margins included).
//       The face box is the box of a, b, c widened by MESH_BOX_PAD of the face's largest coordinate (ray_face_box): a function of
//       the face alone.  An exact hit point lies in the triangle, so clause (3) only removes pairs whose t is off by more than the
//       slab's relative margin RAY_SLAB_REL = 2^-6: results the guard let through with no correct digit (a det a few times its
//       rounding bound).  The margin is relative because t's error is: a ray from 1 km hits a face with an absolute error of
//       1e-4 in t, far more than any fixed widening of a thin axis-aligned box.
//       What a relative margin REL keeps, derived.  Let B = RAY_DET_ROUND S be the guard's bound and |det| = k B.  The computed det
//       is off by at most B, so 1 / det by a factor within 1 / (1 -+ 1 / k).  The numerator A0 . N is rounded like det, with A0 in
//       the place of d: off by at most 8u sum_k |A0_k| Nabs_k (Nabs the absolute cross product of the guard).  On a hit A0 = -t d +
//       (hit point - a), so |A0_k| <= t |d_k| + e_k with e the face's extent, and the numerator, whose exact value is t det, is off
//       by at most (1 + rho) / k of itself, rho = sum_k e_k Nabs_k / (t S): the face's size over the ray's length to it, small
//       unless the origin sits on the face.  The quotient's own roundings and the slab's (three per bound, 3u relative) are below
//       2^-21.  So t is off by at most about (2 + rho) / k of itself, and clause (3) provably keeps every hit with
//           |det| >= (2 + rho) / REL x B:       REL = 2^-6 -> 128 (1 + rho / 2) rounding bounds, |det| / S >= 2^-14 = 6e-5.
//       That is the choice: a whole number of binary orders above the guard (2^7 bounds) that still costs the sweep nothing it can
//       measure — the price of REL is pruning alone, boxes whose entry is within 1.6 % behind the best hit, 5 cm at 3 m — where
//       REL = 2^-3 would reach down to 16 bounds and open everything within 12 % behind a hit: a whole body's far side.  Between
//       the guard and 128 bounds the bound above is the worst case of every rounding pointing one way; the stand-alone program
//       counts what the clause actually rejects there against float64 (tests/native/raycast_tri_main.cpp).
//       It also removes what the reference's OWN eps has moved that far: its u, v, t are the geometric ones times det / (det + 1e-8),
//       so below |det| = 64e-8 (a face of 6 mm^2, N = 1.2e-5, met by a unit d under 3 degrees) the reference's t has left the face by
//       more than 1.6 % and its u, v have shrunk towards the corner a; such a pair is no hit here.  Part of the same departure.
//
// LEMMA (the sweep's exactness, the counterpart of "bound <= computed d2" in ra_mesh.hip).  If raycast_hit accepts a pair with
// computed t, then for the face's leaf box L and group box G:  ray_slab_pass(L), ray_slab_pass(G), lo_t(G) <= lo_t(L) <= t.
// Proof, by monotonicity alone; no rounding analysis is needed because the face's own computed interval is part of the predicate.
//   (a) Box inclusion in fp32.  ra_mesh.hip stores lo_L = min_faces(min(a, b, c)) - pad_L, pad_L = m_L * MESH_BOX_PAD with m_L the
//       largest |coordinate| of the leaf.  For a face of the leaf min(a, b, c) >= the leaf's min and m_face <= m_L; rounded
//       multiplication by a constant and rounded subtraction are monotone in each operand, so lo_L <= lo_face and likewise
//       hi_L >= hi_face, component by component; G is the min / max of its leaves' boxes.
//   (b) ray_slab is monotone in the box.  Per axis with a finite 1 / d_k: t1 = (lo - o) inv, t2 = (hi - o) inv, near = min, far =
//       max.  A lower lo and a higher hi move t1 and t2 apart (rounded subtraction and multiplication by the same inv are
//       monotone), whatever the sign of inv: near falls or stays, far rises or stays.  Per flat axis (d_k = 0, or so small that
//       1 / d_k overflows): the axis passes iff lo <= o <= hi, which a larger box keeps.  entry = max of the nears, exit = min of
//       the fars, lo_t = entry - REL |entry|, hi_t = exit + REL |exit| by one fma each: x -+ REL |x| increases with x (REL < 1)
//       and fma rounding is monotone.  So lo_t(G) <= lo_t(L) <= lo_t(face) and hi_t(G) >= hi_t(L) >= hi_t(face).  No NaN enters,
//       whether or not the machine flushes subnormals: o, d and the kept faces are finite; on a non-flat axis ray_prepare leaves
//       2^-126 <= |inv| < inf (a subnormal or flushed 1 / d_k, |d_k| > 2^126, is replaced by the smallest normal with its sign — one
//       inv per ray and axis for every box, which is all the monotonicity uses); lo - o may overflow to +-inf, and inf times such an
//       inv keeps its sign.
//   (c) Clause (3) gives lo_t(face) <= t <= hi_t(face) and clause (1) t >= 0, so lo_t(L) <= t <= hi_t(L), hence lo_t(L) <= hi_t(L)
//       and hi_t(L) >= 0: ray_slab_pass(L), with entry bound lo_t(L) <= t; the same for G.                                    qed
// The sweep skips a box when ray_slab_pass fails for every lane, or, in nearest mode, when lo_t > a lane's best t STRICTLY: a face
// with t <= best (a tie included) has lo_t <= t <= best and is never skipped.
#pragma once
#include "ra_mesh_tri.hpp"

constexpr float RAY_EPS = 1e-8f;                 // the reference's eps, added to det
constexpr float RAY_DET_ROUND = 0x1p-21f;        // 8 u: rounding bound of det as a share of S
constexpr float RAY_GUARD = 1.f;                 // the guard's multiple of that bound
constexpr float RAY_SLAB_REL = 0x1p-6f;          // relative margin of the computed slab interval
constexpr float RAY_INF = __builtin_huge_valf();
constexpr float RAY_INV_MIN = 0x1p-126f;         // the smallest normal: the least |1 / d_k| the slab test multiplies by

struct RayTri { float u, v, t, det; };
struct RayPre { float inv[3]; bool flat[3]; };   // per ray: 1 / d_k, and whether axis k is flat

RA_MESH_HD void r_cross(const float a[3], const float b[3], float o[3]) {
    o[0] = m_fma(a[1], b[2], -m_mul(a[2], b[1]));
    o[1] = m_fma(a[2], b[0], -m_mul(a[0], b[2]));
    o[2] = m_fma(a[0], b[1], -m_mul(a[1], b[0]));
}

RA_MESH_HD RayTri raycast_tri(const float o[3], const float d[3], const float a[3], const float b[3], const float c[3]) {
    float e1[3], e2[3], a0[3], n[3], da0[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { e1[k] = b[k] - a[k]; e2[k] = c[k] - a[k]; a0[k] = o[k] - a[k]; }
    r_cross(e1, e2, n);
    RayTri r;
    r.det = m_dot(d[0], d[1], d[2], n[0], n[1], n[2]);
    const float invdet = m_div(1.f, -(r.det + RAY_EPS));
    r_cross(a0, d, da0);
    r.u = m_mul(m_dot(da0[0], da0[1], da0[2], e2[0], e2[1], e2[2]), invdet);
    r.v = m_mul(-m_dot(da0[0], da0[1], da0[2], e1[0], e1[1], e1[2]), invdet);
    r.t = m_mul(m_dot(a0[0], a0[1], a0[2], n[0], n[1], n[2]), invdet);
    return r;
}

// clause (1): the reference's predicate (false for any NaN)
RA_MESH_HD bool raycast_ref_hit(const RayTri& r) { return r.t >= 0.f && r.u >= 0.f && r.v >= 0.f && r.u + r.v <= 1.f; }

// clause (2): true = det is above its rounding bound
RA_MESH_HD bool raycast_guard_ok(const float d[3], const float a[3], const float b[3], const float c[3], float det) {
    float e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { e1[k] = fabsf(b[k] - a[k]); e2[k] = fabsf(c[k] - a[k]); }
    const float nx = m_fma(e1[1], e2[2], m_mul(e1[2], e2[1]));
    const float ny = m_fma(e1[2], e2[0], m_mul(e1[0], e2[2]));
    const float nz = m_fma(e1[0], e2[1], m_mul(e1[1], e2[0]));
    const float s = m_dot(fabsf(d[0]), fabsf(d[1]), fabsf(d[2]), nx, ny, nz);
    return fabsf(det) > m_mul(m_mul(RAY_GUARD, RAY_DET_ROUND), s);
}

RA_MESH_HD RayPre ray_prepare(const float d[3]) {
    RayPre p;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float inv = m_div(1.f, d[k]);
        p.flat[k] = !(fabsf(inv) < RAY_INF);            // d_k = 0, or 1 / d_k overflows
        // |d_k| > 2^126: 1 / d_k is subnormal, or zero where subnormals are flushed.  The smallest normal takes its place, with its sign
        // (a flushed zero keeps it), so that no product below is 0 x inf
        p.inv[k] = copysignf(fmaxf(fabsf(inv), RAY_INV_MIN), inv);
    }
    return p;
}

// the computed ray interval [lo_t, hi_t] of a box (lo.xyz, hi.xyz), margins included; an axis that fails gives lo_t = +inf
RA_MESH_HD void ray_slab(const float o[3], const RayPre& p, const float* bx, float& lo_t, float& hi_t) {
    float entry = -RAY_INF, leave = RAY_INF;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t1 = m_mul(bx[k] - o[k], p.inv[k]), t2 = m_mul(bx[3 + k] - o[k], p.inv[k]);
        const bool inside = bx[k] <= o[k] && o[k] <= bx[3 + k];
        const float near = p.flat[k] ? (inside ? -RAY_INF : RAY_INF) : fminf(t1, t2);
        const float far = p.flat[k] ? (inside ? RAY_INF : -RAY_INF) : fmaxf(t1, t2);
        entry = fmaxf(entry, near);
        leave = fminf(leave, far);
    }
    const bool some = bx[0] <= bx[3];       // the empty box (lo = +inf, hi = -inf) of a leaf or group without faces never passes
    lo_t = some ? m_fma(-RAY_SLAB_REL, fabsf(entry), entry) : RAY_INF;
    hi_t = some ? m_fma(RAY_SLAB_REL, fabsf(leave), leave) : -RAY_INF;
}
RA_MESH_HD bool ray_slab_pass(float lo_t, float hi_t) { return lo_t <= hi_t && hi_t >= 0.f; }      // false for a NaN (inf - inf)

// the face's own widened box: a function of the face alone, inside its leaf's stored box component by component
RA_MESH_HD void ray_face_box(const float a[3], const float b[3], const float c[3], float bx[6]) {
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        bx[k] = fminf(fminf(a[k], b[k]), c[k]);
        bx[3 + k] = fmaxf(fmaxf(a[k], b[k]), c[k]);
        m = fmaxf(m, fmaxf(fabsf(bx[k]), fabsf(bx[3 + k])));
    }
    const float pad = m_mul(m, MESH_BOX_PAD);
#pragma unroll
    for (int k = 0; k < 3; ++k) { bx[k] -= pad; bx[3 + k] += pad; }
}

// clauses (2) and (3), for a pair that passed clause (1)
RA_MESH_HD bool raycast_confirm(const float o[3], const float d[3], const RayPre& p, const float a[3], const float b[3], const float c[3],
                                const RayTri& r) {
    if (!raycast_guard_ok(d, a, b, c, r.det)) return false;
    float bx[6], lo_t, hi_t;
    ray_face_box(a, b, c, bx);
    ray_slab(o, p, bx, lo_t, hi_t);
    return lo_t <= r.t && r.t <= hi_t;
}

RA_MESH_HD bool raycast_hit(const float o[3], const float d[3], const RayPre& p, const float a[3], const float b[3], const float c[3],
                            const RayTri& r) {
    return raycast_ref_hit(r) && raycast_confirm(o, d, p, a, b, c, r);
}

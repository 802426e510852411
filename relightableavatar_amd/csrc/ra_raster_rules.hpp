// The per-face and per-pixel rules of ra_raster.hip as host + device functions, so that a (pixel, face) pair has ONE result whatever
// kernel, loop or launch shape computes it, and a stand-alone CPU program (tests/native/raster_rules_main.cpp) runs the same
// operations.  Every line is one named fp32 operation of one rounding, contraction off.
//
// Homogeneous (clipless) rasterisation of clip-space vertices (x, y, z, w); the vector of a vertex is V = (x, y, w).
//
// Pixel centre (raster_centre).  Pixel (ix, iy) of a W x H image is sampled at p = (px, py, 1), px = (2 ix + 1) / W - 1,
//     py = (2 iy + 1) / H - 1: row 0 is at y = -1.
//
// Edge function (raster_edge, raster_edge_at).  For the two ends A, B of an edge, C = A x B and E(p) = (C.x px + C.y py) + C.z.
//     It is computed PER EDGE IN CANONICAL ORIENTATION, the end with the lower vertex index first, and a face uses s E, s = +1 where
//     the face runs the edge from the lower to the higher index, -1 otherwise.  Negation is exact: the two faces on a shared edge see
//     the same bits of E.  Edge k of a face is the one opposite corner k: e_0 = s_0 E(v1, v2), e_1 = s_1 E(v2, v0), e_2 = s_2 E(v0, v1).
//     With p = sum lambda_i V_i one has e_i = lambda_i det, det = V0 . (V1 x V2).
//
// Face (raster_setup).  det = s_0 ((C0.x x0 + C0.y y0) + C0.z w0), sigma = sign(det).  A face with det == 0, a NaN det or any
//     non-finite coordinate is dropped.  The face's PIXEL BOX is part of the rule: a face with every w > 0 is sampled only at the pixels
//     [raster_lo(min x / w), raster_hi(max x / w)] x [likewise in y], the box of its projected corners widened by one pixel and
//     clamped to the image; a face with any w <= 0 has the whole image.  Because the box belongs to the rule and is a function of the
//     face alone, a kernel that bins faces by it and one that scans every face compute the same bits by construction.  The one-pixel
//     margin is far above the rounding of the box arithmetic (a few ulp of a pixel coordinate below 2^20), so the box never cuts a pixel
//     that lies inside the exact triangle.
//
// Inside test (raster_sample).  With t_k = s_k sigma, a pixel is inside when for all three edges
//         sigma s_k E_k > 0,   or   E_k == 0 and t_k > 0,            that is:   t_k > 0 ? E_k >= 0 : E_k < 0.
//
// LEMMA (complementarity).  Let two faces A, B of one view share an edge with opposite orientation (s_A = -s_B), and let E be the
//     edge's canonical value at a sample point, not NaN.  (i) If sigma_A == sigma_B, exactly one of the two edge clauses holds.
//     (ii) If sigma_A == -sigma_B, both clauses hold or neither does.
// Proof.  Both faces evaluate the same expression on the same operands in the same order: the canonical coefficients depend on the two
//     end vertices alone and the sample point on the pixel alone, so E is one bit pattern for both.  (i) t_A = s_A sigma_A =
//     -s_B sigma_B = -t_B.  Say t_A > 0: A's clause is E >= 0, B's is E < 0.  For a value that is not NaN exactly one of E >= 0, E < 0
//     is true.  (ii) t_A = s_A sigma_A = (-s_B)(-sigma_B) = t_B: the two clauses are the same predicate of the same bits.   QED
//     Consequences.  A consistently oriented mesh has, along an interior edge whose two faces face the same way, no crack and no doubly
//     owned pixel from that edge: a sample on it belongs to the face with t > 0.  On a silhouette, where one face is front- and the
//     other back-facing, both decide the same side, so the pair covers a pixel twice or not at all.  E is NaN only when the
//     coefficients overflow (inf - inf); such a pixel is inside neither face.
//
// Barycentrics.  S = (e_0 + e_1) + e_2, b_i = e_i / S: perspective-correct by construction (b_i = lambda_i / sum lambda).  u = b_0,
//     v = b_1, zw = ((b_0 z_0 + b_1 z_1) + b_2 z_2) / ((b_0 w_0 + b_1 w_1) + b_2 w_2).  A sample is kept only when the interpolated
//     w (the denominator) is > 0 and -1 <= zw <= 1; a NaN fails both.
//
// Depth rule (raster_closer).  Per pixel the lexicographic minimum of (zw, face index), -0 and +0 equal: a strict weak order with no
//     ties between different faces, so the winner does not depend on the order in which faces are seen.
//
// Interpolation (raster_interp).  b_2 = (1 - u) - v, out = (u a_0 + v a_1) + b_2 a_2, as nvdiffrast's interpolate.
//
// Gradients, the face index held fixed.  u = e_0 / S, v = e_1 / S give (raster_bary_grad)
//     g_0 = (du (1 - u) - dv v) / S,  g_1 = (dv (1 - v) - du u) / S,  g_2 = -(du u + dv v) / S       (d loss / d e_k),
// and e_0 = (V1 x V2) . p = V1 . (V2 x p) = V2 . (p x V1) is linear in p, so a face needs only the three sums G_k = sum_pixels g_k p
// (raster_corner_grad):  dV0 = G_1 x V2 + V1 x G_2,  dV1 = G_2 x V0 + V2 x G_0,  dV2 = G_0 x V1 + V0 x G_1,  each (d x, d y, d w);
// z carries no gradient because u, v do not depend on it.  The backward uses the ORIENTED edges directly (no canonical order): its
// S is recomputed through the canonical rule, so that it is the forward's.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define RA_RASTER_HD __host__ __device__ __forceinline__
#else
#define RA_RASTER_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr int RASTER_TILE = 8;              // pixels per tile edge: 64 pixels, one wave
constexpr int RASTER_REC_WORDS = 20;        // a face record: five 16-byte words
enum { RASTER_SIGN0 = 1, RASTER_SIGN1 = 2, RASTER_SIGN2 = 4, RASTER_BACK = 8, RASTER_VALID = 16 };      // bit k: s_k = -1; BACK: sigma = -1

struct RasterFace {
    float c[9];         // the canonical coefficient triple of edge k at c[3 k]
    int flags;
    float z[3], w[3];
    int box[4];         // x0, y0, x1, y1, inclusive; x0 > x1 or y0 > y1: empty
};
struct RasterSample { float u, v, zw, s; };     // s: the sum S (what the backward divides by)

RA_RASTER_HD float raster_centre(int i, int n) {
    const float t = (float)(2 * i + 1);
    const float q = t / (float)n;
    return q - 1.0f;
}

// a, b: clip-space (x, y, z, w) of the edge's ends, the lower vertex index first
RA_RASTER_HD void raster_edge(const float* a, const float* b, float* c) {
    const float p0 = a[1] * b[3], q0 = a[3] * b[1];
    const float p1 = a[3] * b[0], q1 = a[0] * b[3];
    const float p2 = a[0] * b[1], q2 = a[1] * b[0];
    c[0] = p0 - q0; c[1] = p1 - q1; c[2] = p2 - q2;
}
RA_RASTER_HD float raster_edge_at(const float* c, float px, float py) {
    const float a = c[0] * px, b = c[1] * py;
    const float ab = a + b;
    return ab + c[2];
}

RA_RASTER_HD bool raster_finite(float x) { return x - x == 0.0f; }

// the first / last pixel of an axis of n pixels that a face reaching the NDC coordinate `ndc` is sampled at (one pixel of margin)
RA_RASTER_HD int raster_lo(float ndc, int n) {
    const float h = 0.5f * (float)n;
    const float t = ndc * h;
    const float th = t + h;
    const float f = floorf(th - 1.5f);
    if (!(f > 0.0f)) return 0;
    if (f > (float)n) return n;
    return (int)f;
}
RA_RASTER_HD int raster_hi(float ndc, int n) {
    const float h = 0.5f * (float)n;
    const float t = ndc * h;
    const float th = t + h;
    const float f = ceilf(th + 0.5f);
    if (!(f < (float)(n - 1))) return n - 1;
    if (f < -1.0f) return -1;
    return (int)f;
}

// p0, p1, p2: clip-space (x, y, z, w) of the corners; i0, i1, i2 their vertex indices
RA_RASTER_HD void raster_setup(const float* p0, const float* p1, const float* p2, int i0, int i1, int i2, int H, int W, RasterFace& r) {
    int flags = 0;
    if (i1 < i2) raster_edge(p1, p2, r.c); else { raster_edge(p2, p1, r.c); flags |= RASTER_SIGN0; }
    if (i2 < i0) raster_edge(p2, p0, r.c + 3); else { raster_edge(p0, p2, r.c + 3); flags |= RASTER_SIGN1; }
    if (i0 < i1) raster_edge(p0, p1, r.c + 6); else { raster_edge(p1, p0, r.c + 6); flags |= RASTER_SIGN2; }
    const float a = r.c[0] * p0[0], b = r.c[1] * p0[1], c = r.c[2] * p0[3];
    const float ab = a + b;
    const float d0 = ab + c;
    const float det = (flags & RASTER_SIGN0) ? -d0 : d0;
    bool ok = det < 0.0f || det > 0.0f;
    for (int k = 0; k < 4; ++k) ok = ok && raster_finite(p0[k]) && raster_finite(p1[k]) && raster_finite(p2[k]);
    if (det < 0.0f) flags |= RASTER_BACK;
    r.z[0] = p0[2]; r.z[1] = p1[2]; r.z[2] = p2[2];
    r.w[0] = p0[3]; r.w[1] = p1[3]; r.w[2] = p2[3];
    if (!ok) {
        r.flags = 0;
        r.box[0] = r.box[1] = 0; r.box[2] = r.box[3] = -1;
        return;
    }
    r.flags = flags | RASTER_VALID;
    if (p0[3] > 0.0f && p1[3] > 0.0f && p2[3] > 0.0f) {
        const float x0 = p0[0] / p0[3], x1 = p1[0] / p1[3], x2 = p2[0] / p2[3];
        const float y0 = p0[1] / p0[3], y1 = p1[1] / p1[3], y2 = p2[1] / p2[3];
        r.box[0] = raster_lo(fminf(x0, fminf(x1, x2)), W);
        r.box[1] = raster_lo(fminf(y0, fminf(y1, y2)), H);
        r.box[2] = raster_hi(fmaxf(x0, fmaxf(x1, x2)), W);
        r.box[3] = raster_hi(fmaxf(y0, fmaxf(y1, y2)), H);
    } else {
        r.box[0] = 0; r.box[1] = 0; r.box[2] = W - 1; r.box[3] = H - 1;
    }
}

// one edge clause: E the canonical value, t = s sigma > 0 ?
RA_RASTER_HD bool raster_edge_clause(float E, bool t_positive) { return t_positive ? E >= 0.0f : E < 0.0f; }

// the face at pixel (ix, iy), whose centre is (px, py)
RA_RASTER_HD bool raster_sample(const RasterFace& r, int ix, int iy, float px, float py, RasterSample& o) {
    if (!(r.flags & RASTER_VALID)) return false;
    if (ix < r.box[0] || ix > r.box[2] || iy < r.box[1] || iy > r.box[3]) return false;
    const bool back = (r.flags & RASTER_BACK) != 0;
    const float E0 = raster_edge_at(r.c, px, py), E1 = raster_edge_at(r.c + 3, px, py), E2 = raster_edge_at(r.c + 6, px, py);
    const bool n0 = (r.flags & RASTER_SIGN0) != 0, n1 = (r.flags & RASTER_SIGN1) != 0, n2 = (r.flags & RASTER_SIGN2) != 0;
    if (!raster_edge_clause(E0, n0 == back) || !raster_edge_clause(E1, n1 == back) || !raster_edge_clause(E2, n2 == back)) return false;
    const float e0 = n0 ? -E0 : E0, e1 = n1 ? -E1 : E1, e2 = n2 ? -E2 : E2;
    const float e01 = e0 + e1;
    const float S = e01 + e2;
    const float b0 = e0 / S, b1 = e1 / S, b2 = e2 / S;
    const float z0 = b0 * r.z[0], z1 = b1 * r.z[1], z2 = b2 * r.z[2];
    const float w0 = b0 * r.w[0], w1 = b1 * r.w[1], w2 = b2 * r.w[2];
    const float z01 = z0 + z1, w01 = w0 + w1;
    const float zn = z01 + z2, wn = w01 + w2;
    if (!(wn > 0.0f)) return false;
    const float zw = zn / wn;
    if (!(zw >= -1.0f && zw <= 1.0f)) return false;
    o.u = b0; o.v = b1; o.zw = zw; o.s = S;
    return true;
}

// does (zw, f) come before the pixel's best so far (best_f < 0: none)?
RA_RASTER_HD bool raster_closer(float zw, int f, float best_zw, int best_f) {
    return best_f < 0 || zw < best_zw || (zw == best_zw && f < best_f);
}

RA_RASTER_HD float raster_b2(float u, float v) {
    const float t = 1.0f - u;
    return t - v;
}
RA_RASTER_HD float raster_interp(float u, float v, float b2, float a0, float a1, float a2) {
    const float p = u * a0, q = v * a1, r = b2 * a2;
    const float pq = p + q;
    return pq + r;
}

// d loss / d e_k from d loss / d (u, v)
RA_RASTER_HD void raster_bary_grad(float u, float v, float S, float du, float dv, float* g) {
    const float uu = du * u, vv = dv * v;
    const float a = du - uu, b = dv - vv;
    const float n0 = a - vv, n1 = b - uu, n2 = uu + vv;
    g[0] = n0 / S; g[1] = n1 / S; g[2] = -n2 / S;
}

// a x b of (x, y, w) triples
RA_RASTER_HD void raster_cross(const float* a, const float* b, float* o) {
    const float p0 = a[1] * b[2], q0 = a[2] * b[1];
    const float p1 = a[2] * b[0], q1 = a[0] * b[2];
    const float p2 = a[0] * b[1], q2 = a[1] * b[0];
    o[0] = p0 - q0; o[1] = p1 - q1; o[2] = p2 - q2;
}
// G: the three sums G_k (3 each); V0, V1, V2: (x, y, w); out: 9 values, the gradient in (x, y, w) of corner k at out[3 k]
RA_RASTER_HD void raster_corner_grad(const float* G, const float* V0, const float* V1, const float* V2, float* out) {
    float a[3], b[3];
    raster_cross(G + 3, V2, a); raster_cross(V1, G + 6, b);
    for (int k = 0; k < 3; ++k) out[k] = a[k] + b[k];
    raster_cross(G + 6, V0, a); raster_cross(V2, G, b);
    for (int k = 0; k < 3; ++k) out[3 + k] = a[k] + b[k];
    raster_cross(G, V1, a); raster_cross(V0, G + 3, b);
    for (int k = 0; k < 3; ++k) out[6 + k] = a[k] + b[k];
}

// The per-pair rule of ra_antialias.hip as host + device functions, in the style of ra_raster_rules.hpp (which it builds on): a pixel
// pair has ONE result whichever thread, kernel or CPU program (tests/native/antialias_rules_main.cpp) evaluates it.  Every line is one
// named fp32 operation of one rounding, contraction off.  The rule is this project's statement of Laine et al. 2020, section 3.4.
//
// Pair.  Two 4-adjacent pixels of one view, horizontal (x, y)-(x + 1, y) or vertical (x, y)-(x, y + 1), named by its FIRST pixel and
//     its axis, whose face ids f0 != f1 both lie in [-1, F) (-1: empty).  Every other pair is inert.
// Own pixel (antialias_own).  The side that is not empty; with both covered, the side that wins raster_closer(zw, face).  f is the own
//     pixel's face, (px, py) its centre, dir = +1 when the own pixel is the pair's first, else -1.
// Candidate edges (antialias_edge), k = 0, 1, 2 ascending, edge k opposite corner k, ends A, B in canonical order (the lower vertex
//     index first), C = raster_edge(A, B).  It qualifies when
//       A.w > 0 and B.w > 0;
//       it straddles the line through the own centre: horizontal pair qA = A.y - py A.w, qB = B.y - py B.w, (qA < 0) != (qB < 0) and
//           C.x != 0; vertical pair the same with x, px and C.y;
//       its crossing lies between the two centres: horizontal x* = -((C.y py) + C.z) / C.x, d = dir ((x* - px) (0.5 W)); vertical
//           y* = -((C.x px) + C.z) / C.y, d = dir ((y* - py) (0.5 H)); 0 <= d <= 1, a NaN fails;
//       it is a silhouette IN THIS VIEW (antialias_silhouette): the edge does not have exactly two half-edges (twin < 0), or the twin's
//           face is dropped by raster_setup, or t_f == t_g with t = (sign flag of the edge slot == RASTER_BACK flag) of each face — case
//           (ii) of the rasteriser's lemma: the two opposite corners lie on the same side of the edge.
//     The first qualifying k is the pair's edge, alpha = d - 0.5; none: the pair is inert.  The tests are pure, so the order in which
//     they are evaluated (the silhouette test last: it is the dearest) does not change the result.
// Blend (antialias_weight), from the INPUT colours: alpha >= 0: out[other] += alpha (in[own] - in[other]); else out[own] += (-alpha)
//     (in[other] - in[own]).  With `target` the pixel written, `source` the other one and w = |alpha|: out[target] += w (in[source] -
//     in[target]).  A pixel starts from its input and adds the deltas of its pairs in the order left, right, up, down.
// Gradients, the face map and the set of active pairs held fixed.  d out / d in is the transpose of the blend.  d L / d alpha =
//     sign(alpha) sum_c dout[target, c] (in[source, c] - in[target, c]), the channels ascending.  alpha depends on pos through C alone
//     (antialias_dc): horizontal d x* / d C = (-x* / C.x, -py / C.x, -1 / C.x), vertical d y* / d C = (-px / C.y, -y* / C.y, -1 / C.y);
//     with C = A x B in (x, y, w): dA = B x dC, dB = dC x A (antialias_ends, through raster_cross).  z carries no gradient.
//
// Deviations from nvdiffrast, deliberate: no fixed-point snapping of the positions, and only the own pixel's face is searched for
// silhouette edges (as the paper states it).
#pragma once
#include "ra_raster_rules.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

struct AaPair {
    int active;         // 0: inert
    int own;            // 0: the pair's first pixel owns, 1: the second
    int k;              // the edge slot of the own face
    int he;             // its half-edge, 3 f + (k + 1) % 3: it leaves corner k + 1 towards corner k + 2
    float alpha;
    float c[3];         // the canonical coefficient triple
    float cross;        // x* (horizontal) or y* (vertical)
    float px, py;       // the own centre
};

// the flags raster_setup gives the face (its SIGN bits, BACK, VALID; 0 for a dropped face) without the rest of the record
RA_RASTER_HD int antialias_face_flags(const float* p0, const float* p1, const float* p2, int i0, int i1, int i2) {
    int flags = 0;
    float c[3];
    if (i1 < i2) raster_edge(p1, p2, c); else { raster_edge(p2, p1, c); flags |= RASTER_SIGN0; }
    if (!(i2 < i0)) flags |= RASTER_SIGN1;
    if (!(i0 < i1)) flags |= RASTER_SIGN2;
    const float a = c[0] * p0[0], b = c[1] * p0[1], cc = c[2] * p0[3];
    const float ab = a + b;
    const float d0 = ab + cc;
    const float det = (flags & RASTER_SIGN0) ? -d0 : d0;
    bool ok = det < 0.0f || det > 0.0f;
    for (int q = 0; q < 4; ++q) ok = ok && raster_finite(p0[q]) && raster_finite(p1[q]) && raster_finite(p2[q]);
    if (!ok) return 0;
    if (det < 0.0f) flags |= RASTER_BACK;
    return flags | RASTER_VALID;
}

// t of edge slot k: sign flag == BACK flag
RA_RASTER_HD bool antialias_t(int flags, int k) { return (((flags >> k) & 1) != 0) == ((flags & RASTER_BACK) != 0); }

// which pixel of a pair owns it: 0 the first, 1 the second (f0 != f1, at most one of them empty)
RA_RASTER_HD int antialias_own(float zw0, int f0, float zw1, int f1) {
    if (f0 < 0) return 1;
    if (f1 < 0) return 0;
    return raster_closer(zw0, f0, zw1, f1) ? 0 : 1;
}

// one candidate edge without the silhouette test.  a, b: clip-space (x, y, z, w) of the ends, the lower vertex index first; n = W
// (horizontal) or H (vertical).  On success c, *cross and *alpha are set.
RA_RASTER_HD bool antialias_edge(const float* a, const float* b, int vertical, float px, float py, int dir, int n, float* c, float* cross, float* alpha) {
    if (!(a[3] > 0.0f) || !(b[3] > 0.0f)) return false;
    raster_edge(a, b, c);
    const float fix = vertical ? px : py, run = vertical ? py : px;         // the line through the own centre: x = px (vertical pair) or y = py
    const float ca = vertical ? a[0] : a[1], cb = vertical ? b[0] : b[1];
    const float ta = fix * a[3], tb = fix * b[3];
    const float qa = ca - ta, qb = cb - tb;
    if ((qa < 0.0f) == (qb < 0.0f)) return false;
    const float div = vertical ? c[1] : c[0], mul = vertical ? c[0] : c[1];
    if (!(div != 0.0f)) return false;
    const float m = mul * fix;
    const float s = m + c[2];
    const float ns = -s;
    const float x = ns / div;
    const float diff = x - run;
    const float half = 0.5f * (float)n;
    const float sc = diff * half;
    const float d = dir > 0 ? sc : -sc;
    if (!(d >= 0.0f && d <= 1.0f)) return false;
    *cross = x;
    *alpha = d - 0.5f;
    return true;
}

// is edge slot k of face f (flags_f, half-edge he) a silhouette in this view?  pos: the view's V x 4 positions; vert, twin: the topology's
RA_RASTER_HD bool antialias_silhouette(const float* pos, const int* vert, const int* twin, int flags_f, int k, int he) {
    const int tw = twin[he];
    if (tw < 0) return true;
    const int g = tw / 3, j = tw - 3 * g, kg = (j + 2) % 3;          // half-edge 3 g + j leaves corner j: it is edge slot j + 2 of face g
    const int i0 = vert[3 * g], i1 = vert[3 * g + 1], i2 = vert[3 * g + 2];
    const int flags_g = antialias_face_flags(pos + 4ll * i0, pos + 4ll * i1, pos + 4ll * i2, i0, i1, i2);
    if (!(flags_g & RASTER_VALID)) return true;
    return antialias_t(flags_f, k) == antialias_t(flags_g, kg);
}

// The pair whose first pixel is (x, y).  face, zw: the view's H x W maps; pos: the view's V x 4 positions; vert, twin: the topology's 3 F
// arrays (vertex indices checked when it was built).  The caller guarantees that the second pixel exists.
RA_RASTER_HD void antialias_pair(const int* face, const float* zw, const float* pos, const int* vert, const int* twin, int F, int H, int W, int x, int y,
                                 int vertical, AaPair& o) {
    o.active = 0;
    const long long p0 = (long long)y * W + x, p1 = vertical ? p0 + W : p0 + 1;
    const int f0 = face[p0], f1 = face[p1];
    if (f0 == f1 || f0 < -1 || f1 < -1 || f0 >= F || f1 >= F) return;
    const int own = antialias_own(zw[p0], f0, zw[p1], f1);
    const int f = own ? f1 : f0, dir = own ? -1 : 1;
    const int ox = x + (own && !vertical ? 1 : 0), oy = y + (own && vertical ? 1 : 0);
    const float px = raster_centre(ox, W), py = raster_centre(oy, H);
    const int idx[3] = {vert[3 * f], vert[3 * f + 1], vert[3 * f + 2]};
    int flags = -1;
    for (int k = 0; k < 3; ++k) {
        const int ia = idx[(k + 1) % 3], ib = idx[(k + 2) % 3];
        const float *a = pos + 4ll * (ia < ib ? ia : ib), *b = pos + 4ll * (ia < ib ? ib : ia);
        float c[3], cross, alpha;
        if (!antialias_edge(a, b, vertical, px, py, dir, vertical ? H : W, c, &cross, &alpha)) continue;
        if (flags < 0) flags = antialias_face_flags(pos + 4ll * idx[0], pos + 4ll * idx[1], pos + 4ll * idx[2], idx[0], idx[1], idx[2]);
        if (!(flags & RASTER_VALID)) return;            // not a face the rasteriser can have written
        const int he = 3 * f + (k + 1) % 3;
        if (!antialias_silhouette(pos, vert, twin, flags, k, he)) continue;
        o.active = 1; o.own = own; o.k = k; o.he = he; o.alpha = alpha; o.c[0] = c[0]; o.c[1] = c[1]; o.c[2] = c[2]; o.cross = cross; o.px = px; o.py = py;
        return;
    }
}

// the blend of an active pair: is the pair's SECOND pixel the one written, and with which weight
RA_RASTER_HD int antialias_target(const AaPair& p) { return p.alpha >= 0.0f ? 1 - p.own : p.own; }
RA_RASTER_HD float antialias_weight(const AaPair& p) { return p.alpha >= 0.0f ? p.alpha : -p.alpha; }

// one channel of the forward: acc + w (source - target_in)
RA_RASTER_HD float antialias_blend(float acc, float w, float source, float target_in) {
    const float diff = source - target_in;
    const float prod = w * diff;
    return acc + prod;
}

// d L / d C of an active pair from g = d L / d alpha; n = W (horizontal) or H (vertical)
RA_RASTER_HD void antialias_dc(const AaPair& p, int vertical, int n, float g, float* dc) {
    const float gd = p.own ? -g : g;                // dir
    const float half = 0.5f * (float)n;
    const float gx = gd * half;
    const float div = vertical ? p.c[1] : p.c[0];
    const float r = gx / div;
    const float nr = -r;
    const float along = nr * p.cross, fixed = nr * (vertical ? p.px : p.py);
    dc[0] = vertical ? fixed : along;
    dc[1] = vertical ? along : fixed;
    dc[2] = nr;
}

// the gradients (x, y, w) of the canonical ends A, B of an edge from d L / d C: dA = B x dC, dB = dC x A
RA_RASTER_HD void antialias_ends(const float* a, const float* b, const float* dc, float* da, float* db) {
    const float A[3] = {a[0], a[1], a[3]}, B[3] = {b[0], b[1], b[3]};
    raster_cross(B, dc, da);
    raster_cross(dc, A, db);
}

// The rules of the texture path (ra_texture.hip) as host + device functions, in the style of ra_raster_rules.hpp (which it builds on): a
// pixel has ONE result whichever thread, kernel or CPU program (tests/native/texture_rules_main.cpp) evaluates it.  Every line is one
// named fp32 operation of one rounding, contraction off.  The rule is this project's statement of Laine et al. 2020, section 3.3.
//
// Pixel differentials (texture_db).  With e_i = s_i E_i(p), S = (e_0 + e_1) + e_2 and b_i = e_i / S as the forward computes them, e_i
//     is linear in the sample p and d p_x / d X = 2 / W, so d b_i / d X = (2 / W) (c_i.x - b_i ((c_0.x + c_1.x) + c_2.x)) / S with c_i the
//     canonical edge coefficients times s_i (negation is exact); likewise in Y with c.y and 2 / H.  Layout (du/dX, du/dY, dv/dX,
//     dv/dY), u = b_0, v = b_1.  An attribute's differential (texture_attr_da): da/dX = du/dX (a_0 - a_2) + dv/dX (a_1 - a_2).
// Mip chain (texture_levels, texture_mean).  Level l + 1 is the 2 x 2 mean ((a + b) + (c + d)) 0.25 of level l, rows first; it exists
//     while both extents of level l are even and above 1, up to max_mip_level and TEX_MAX_LEVELS - 1.  Lmax is the last level.
// Level of detail (texture_lod).  From uv_da = (du/dX, du/dY, dv/dX, dv/dY): ax = du/dX TW, ay = du/dY TW, bx = dv/dX TH, by = dv/dY TH,
//     A = ax ax + ay ay, Bq = bx bx + by by, Cq = ax bx + ay by, m2 = 0.5 (A + Bq) + sqrt(0.25 (A - Bq)^2 + Cq^2): the squared major
//     axis of the pixel's footprint in level-0 texels.  lod = 0.5 log2(m2) clamped to [0, Lmax]; a NaN m2 or m2 <= 1 gives 0 (log2 <= 0
//     clamps to 0 anyway).  l0 = floor(lod), f = lod - l0; at l0 >= Lmax: l0 = Lmax, f = 0.  sqrt is the correctly rounded one.
// log2 (texture_log2), for normal x > 0.  x = m 2^e with m in [1, 2) from the bits (exact); m > TEX_SQRT2 moves to m / 2, e + 1 (exact),
//     so m lies in [0.7071, 1.4143].  s = (m - 1) / (m + 1), z = s s, p = ((((K9 z + K7) z + K5) z + K3) z + K1), log2(m) = s p with
//     K_j = 2 / (j ln 2) rounded to fp32, and log2(x) = e + s p: the same bits on the host, on the device and in numpy.
// Texel addressing at a level of extents (w, h), row 0 at v = 0.  linear (texture_axis): x = u w - 0.5, x0 = floor(x), fx = x - x0, taps
//     x0 and x0 + 1, gx = 1 - fx; the same in y.  The four weights in the FIXED TAP ORDER (x0, y0), (x1, y0), (x0, y1), (x1, y1) are
//     gx gy, fx gy, gx fy, fx fy, and a channel is ((w0 t0 + w1 t1) + w2 t2) + w3 t3.  nearest: texel floor(u w), floor(v h).
//     Boundary wrap: the index modulo the extent, the mathematical modulo; clamp: clamped to [0, extent - 1].
//     A u or v that is not finite, or so large that |u TW| or |v TH| is not below 2^30, gives an output of 0 and no gradient.
// Trilinear: out = (1 - f) linear(l0) + f linear(l0 + 1); with f == 0 out = linear(l0) and the second level is not read.
// Gradients, FIRST ORDER: the texel cells, the level pair and lod are held fixed; uv_da carries no gradient (nvdiffrast differentiates
//     lod: a stated deviation).  Per level d out_c / d u = w ((t1 - t0) gy + (t3 - t2) fy), d out_c / d v = h ((t2 - t0) gx + (t3 - t1) fx);
//     duv sums dout_c times the bracket over the channels ascending, multiplies by the extent, and blends the two levels like the
//     output.  d out_c / d tex[level, tap k] = lw w_k with lw = 1 - f or f (texture_tap_weight); nearest: one tap of weight 1, duv = 0.
#pragma once
#include "ra_raster_rules.hpp"
#include <cstdint>
#include <cstring>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

enum { TEX_NEAREST = 0, TEX_LINEAR = 1, TEX_TRILINEAR = 2 };       // the filter modes of the C entry points (RA_TEX_FILTER_*)
enum { TEX_WRAP = 0, TEX_CLAMP = 1 };                               // the boundary modes (RA_TEX_BOUNDARY_*)
constexpr int TEX_MAX_LEVELS = 16;
constexpr int TEX_MAX_CHANNELS = 64;
constexpr int TEX_MAX_EXTENT = 1 << 15;
constexpr float TEX_SQRT2 = 1.41421354f;
constexpr float TEX_K1 = 2.88539004f, TEX_K3 = 0.961796701f, TEX_K5 = 0.577078044f, TEX_K7 = 0.412198603f, TEX_K9 = 0.320598900f;

struct TexLevels {
    int n;                              // levels 0 .. n - 1: Lmax = n - 1
    int w[TEX_MAX_LEVELS], h[TEX_MAX_LEVELS];
    long long off[TEX_MAX_LEVELS + 1];  // in texels of one texture; off[n] is the chain's size
};

// host arithmetic from the sizes alone
RA_RASTER_HD void texture_levels(int TH, int TW, int max_mip_level, TexLevels& L) {
    L.n = 1; L.w[0] = TW; L.h[0] = TH; L.off[0] = 0; L.off[1] = (long long)TW * TH;
    while (L.n - 1 < max_mip_level && L.n < TEX_MAX_LEVELS) {
        const int w = L.w[L.n - 1], h = L.h[L.n - 1];
        if (w < 2 || h < 2 || (w & 1) || (h & 1)) break;
        L.w[L.n] = w / 2; L.h[L.n] = h / 2;
        L.off[L.n + 1] = L.off[L.n] + (long long)(w / 2) * (h / 2);
        ++L.n;
    }
}

RA_RASTER_HD float texture_mean(float a, float b, float c, float d) {
    const float ab = a + b, cd = c + d;
    const float s = ab + cd;
    return s * 0.25f;
}

// rast_db of one covered pixel.  p0, p1, p2: clip-space corners, i0, i1, i2 their vertex indices; (px, py) the pixel's centre
RA_RASTER_HD void texture_db(const float* p0, const float* p1, const float* p2, int i0, int i1, int i2, float px, float py, int H, int W, float* o) {
    float c[9];
    bool n0 = false, n1 = false, n2 = false;
    if (i1 < i2) raster_edge(p1, p2, c); else { raster_edge(p2, p1, c); n0 = true; }
    if (i2 < i0) raster_edge(p2, p0, c + 3); else { raster_edge(p0, p2, c + 3); n1 = true; }
    if (i0 < i1) raster_edge(p0, p1, c + 6); else { raster_edge(p1, p0, c + 6); n2 = true; }
    const float E0 = raster_edge_at(c, px, py), E1 = raster_edge_at(c + 3, px, py), E2 = raster_edge_at(c + 6, px, py);
    const float e0 = n0 ? -E0 : E0, e1 = n1 ? -E1 : E1, e2 = n2 ? -E2 : E2;
    const float e01 = e0 + e1;
    const float S = e01 + e2;
    const float b0 = e0 / S, b1 = e1 / S;
    const float tw = 2.0f / (float)W, th = 2.0f / (float)H;
#pragma unroll
    for (int a = 0; a < 2; ++a) {            // a = 0: x, 1: y
        const float c0 = n0 ? -c[a] : c[a], c1 = n1 ? -c[3 + a] : c[3 + a], c2 = n2 ? -c[6 + a] : c[6 + a];
        const float c01 = c0 + c1;
        const float cs = c01 + c2;
        const float t0 = b0 * cs, t1 = b1 * cs;
        const float m0 = c0 - t0, m1 = c1 - t1;
        const float q0 = m0 / S, q1 = m1 / S;
        o[a] = q0 * (a ? th : tw);
        o[2 + a] = q1 * (a ? th : tw);
    }
}

// one channel's (da/dX, da/dY) from the pixel's rast_db and the three corner values
RA_RASTER_HD void texture_attr_da(const float* db, float a0, float a1, float a2, float* o) {
    const float d0 = a0 - a2, d1 = a1 - a2;
    const float px = db[0] * d0, qx = db[2] * d1;
    const float py = db[1] * d0, qy = db[3] * d1;
    o[0] = px + qx; o[1] = py + qy;
}

// log2 of a normal x > 0
RA_RASTER_HD float texture_log2(float x) {
    uint32_t bits;
    memcpy(&bits, &x, 4);
    int e = (int)((bits >> 23) & 0xffu) - 127;
    uint32_t mb = (bits & 0x007fffffu) | 0x3f800000u;
    float m;
    memcpy(&m, &mb, 4);
    if (m > TEX_SQRT2) { m = m * 0.5f; e = e + 1; }
    const float num = m - 1.0f, den = m + 1.0f;
    const float s = num / den;
    const float z = s * s;
    float p = TEX_K9 * z;
    p = p + TEX_K7;
    p = p * z;
    p = p + TEX_K5;
    p = p * z;
    p = p + TEX_K3;
    p = p * z;
    p = p + TEX_K1;
    const float frac = s * p;
    return (float)e + frac;
}

// the level pair of a pixel: *l0 and the return value f (0 <= f < 1; f == 0: level l0 alone)
RA_RASTER_HD float texture_lod(const float* da, int TH, int TW, int Lmax, int* l0) {
    *l0 = 0;
    const float ax = da[0] * (float)TW, ay = da[1] * (float)TW, bx = da[2] * (float)TH, by = da[3] * (float)TH;
    const float axx = ax * ax, ayy = ay * ay, bxx = bx * bx, byy = by * by, abx = ax * bx, aby = ay * by;
    const float A = axx + ayy, Bq = bxx + byy, Cq = abx + aby;
    const float hs = A + Bq;
    const float h = 0.5f * hs;
    const float d = A - Bq;
    const float d2 = d * d;
    const float q = 0.25f * d2;
    const float c2 = Cq * Cq;
    const float r = q + c2;
    const float sq = sqrtf(r);
    const float m2 = h + sq;
    if (!(m2 > 1.0f)) return 0.0f;              // NaN, m2 <= 0, and log2 <= 0
    if (!(m2 < 3.0e38f)) { *l0 = Lmax; return 0.0f; }
    const float lg = texture_log2(m2);
    const float lod = 0.5f * lg;
    if (!(lod < (float)Lmax)) { *l0 = Lmax; return 0.0f; }
    const float fl = floorf(lod);
    *l0 = (int)fl;
    return lod - fl;
}

RA_RASTER_HD bool texture_uv_ok(float u, float v, int TH, int TW) {
    const float a = u * (float)TW, b = v * (float)TH;
    return fabsf(a) < 1073741824.0f && fabsf(b) < 1073741824.0f;         // a NaN or an inf fails
}

RA_RASTER_HD int texture_index(int i, int n, int boundary) {
    if (boundary == TEX_CLAMP) return i < 0 ? 0 : i > n - 1 ? n - 1 : i;
    const int r = i % n;
    return r < 0 ? r + n : r;
}

// one axis of the linear filter at a level of extent n: the two tap indices and the fraction
RA_RASTER_HD float texture_axis(float u, int n, int boundary, int* i0, int* i1) {
    const float m = u * (float)n;
    const float x = m - 0.5f;
    const float fl = floorf(x);
    const int i = (int)fl;
    *i0 = texture_index(i, n, boundary);
    *i1 = texture_index(i + 1, n, boundary);
    return x - fl;
}

RA_RASTER_HD int texture_nearest(float u, int n, int boundary) {
    const float m = u * (float)n;
    return texture_index((int)floorf(m), n, boundary);
}

struct TexTaps {
    int idx[4];         // texel y w + x of the four taps, in the fixed tap order
    float w[4];
    float fx, fy, gx, gy;
};

RA_RASTER_HD void texture_taps(float u, float v, int w, int h, int boundary, TexTaps& t) {
    int x0, x1, y0, y1;
    t.fx = texture_axis(u, w, boundary, &x0, &x1);
    t.fy = texture_axis(v, h, boundary, &y0, &y1);
    t.gx = 1.0f - t.fx; t.gy = 1.0f - t.fy;
    t.idx[0] = y0 * w + x0; t.idx[1] = y0 * w + x1; t.idx[2] = y1 * w + x0; t.idx[3] = y1 * w + x1;
    t.w[0] = t.gx * t.gy; t.w[1] = t.fx * t.gy; t.w[2] = t.gx * t.fy; t.w[3] = t.fx * t.fy;
}

RA_RASTER_HD float texture_bilinear(const TexTaps& t, float t0, float t1, float t2, float t3) {
    const float p0 = t.w[0] * t0, p1 = t.w[1] * t1, p2 = t.w[2] * t2, p3 = t.w[3] * t3;
    const float s1 = p0 + p1;
    const float s2 = s1 + p2;
    return s2 + p3;
}

// (1 - f) a + f b
RA_RASTER_HD float texture_mix(float f, float a, float b) {
    const float g = 1.0f - f;
    const float p = g * a, q = f * b;
    return p + q;
}

// one channel's brackets of d out / d u and d out / d v at a level (before the extent)
RA_RASTER_HD void texture_duv_term(const TexTaps& t, float t0, float t1, float t2, float t3, float* du, float* dv) {
    const float dx0 = t1 - t0, dx1 = t3 - t2, dy0 = t2 - t0, dy1 = t3 - t1;
    const float a = dx0 * t.gy, b = dx1 * t.fy, c = dy0 * t.gx, d = dy1 * t.fx;
    *du = a + b; *dv = c + d;
}

// d out_c / d tex of tap k at the first (second == 0) or second level of the pair
RA_RASTER_HD float texture_tap_weight(float f, int second, float w) {
    const float lw = second ? f : 1.0f - f;
    return lw * w;
}

// everything a pixel decides before it touches a texel
struct TexPixel {
    int ok;             // 0: the output is 0 and nothing receives a gradient
    int l0, two;        // the first level; two: level l0 + 1 is read as well (f != 0)
    float f;
    TexTaps t[2];       // nearest: t[0].idx[0] alone
};

// da: the pixel's uv_da, read only with TEX_TRILINEAR
RA_RASTER_HD void texture_pixel(float u, float v, const float* da, const TexLevels& L, int filter, int boundary, TexPixel& p) {
    p.ok = texture_uv_ok(u, v, L.h[0], L.w[0]) ? 1 : 0;
    p.l0 = 0; p.two = 0; p.f = 0.0f;
    if (!p.ok) return;
    if (filter == TEX_NEAREST) {
        p.t[0].idx[0] = texture_nearest(v, L.h[0], boundary) * L.w[0] + texture_nearest(u, L.w[0], boundary);
        return;
    }
    if (filter == TEX_TRILINEAR) p.f = texture_lod(da, L.h[0], L.w[0], L.n - 1, &p.l0);
    p.two = p.f != 0.0f ? 1 : 0;
    texture_taps(u, v, L.w[p.l0], L.h[p.l0], boundary, p.t[0]);
    if (p.two) texture_taps(u, v, L.w[p.l0 + 1], L.h[p.l0 + 1], boundary, p.t[1]);
}

// one channel of the output; a, b: that channel of texel 0 of levels l0 and l0 + 1 (b is not read unless p.two), C the channel stride
RA_RASTER_HD float texture_value(const TexPixel& p, const float* a, const float* b, int C) {
    const TexTaps& t = p.t[0];
    const float v0 = texture_bilinear(t, a[(long long)t.idx[0] * C], a[(long long)t.idx[1] * C], a[(long long)t.idx[2] * C], a[(long long)t.idx[3] * C]);
    if (!p.two) return v0;
    const TexTaps& s = p.t[1];
    const float v1 = texture_bilinear(s, b[(long long)s.idx[0] * C], b[(long long)s.idx[1] * C], b[(long long)s.idx[2] * C], b[(long long)s.idx[3] * C]);
    return texture_mix(p.f, v0, v1);
}

// duv of a pixel: a, b: channel 0 of texel 0 of the two levels; dout: the pixel's C values; (w0, h0), (w1, h1): the levels' extents
RA_RASTER_HD void texture_duv(const TexPixel& p, const float* a, const float* b, const float* dout, int C, int w0, int h0, int w1, int h1, float* o) {
    float U[2] = {0.0f, 0.0f}, V[2] = {0.0f, 0.0f};
    for (int k = 0; k <= p.two; ++k) {
        const TexTaps& t = p.t[k];
        const float* src = k ? b : a;
        float su = 0.0f, sv = 0.0f;
        for (int c = 0; c < C; ++c) {
            float du, dv;
            texture_duv_term(t, src[(long long)t.idx[0] * C + c], src[(long long)t.idx[1] * C + c], src[(long long)t.idx[2] * C + c], src[(long long)t.idx[3] * C + c],
                             &du, &dv);
            const float pu = dout[c] * du, pv = dout[c] * dv;
            su = su + pu; sv = sv + pv;
        }
        U[k] = su * (float)(k ? w1 : w0);
        V[k] = sv * (float)(k ? h1 : h0);
    }
    o[0] = p.two ? texture_mix(p.f, U[0], U[1]) : U[0];
    o[1] = p.two ? texture_mix(p.f, V[0], V[1]) : V[0];
}

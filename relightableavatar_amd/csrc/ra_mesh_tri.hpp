// The per-triangle arithmetic of ra_mesh.hip and its box bounds, as host + device functions: the query kernel inlines them, and a
// stand-alone CPU program (tests/native/mesh_tri_main.cpp) runs the same operations — IEEE fp32 multiply, fused multiply-add and
// division, no contraction — to check the lemma the sweep's exactness rests on: box bound <= computed d2 <= far-corner bound.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define RA_MESH_HD __host__ __device__ __forceinline__
#else
#define RA_MESH_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// a leaf box is widened by this share of its largest coordinate: more than a computed closest point can leave its triangle's exact box
constexpr float MESH_BOX_PAD = 0x1p-19f;

// every product, fused multiply-add and division of the arithmetic below by name: ONE rounding order, whoever inlines it.  On the device
// the round-to-nearest intrinsics, which no fast-math or divide-precision option of the build can weaken; on the host the IEEE operators
// (the stand-alone program is built with -ffp-contract=off and without fast-math)
#if defined(__HIP_DEVICE_COMPILE__)
RA_MESH_HD float m_mul(float a, float b) { return __fmul_rn(a, b); }
RA_MESH_HD float m_fma(float a, float b, float c) { return __fmaf_rn(a, b, c); }
RA_MESH_HD float m_div(float a, float b) { return __fdiv_rn(a, b); }
#else
RA_MESH_HD float m_mul(float a, float b) { return a * b; }
RA_MESH_HD float m_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
RA_MESH_HD float m_div(float a, float b) { return a / b; }
#endif

RA_MESH_HD float m_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return m_fma(az, bz, m_fma(ax, bx, m_mul(ay, by)));      // the order of ra_hdq.hip's dist2
}
// num / den clamped to [0, 1]; a denominator that is not positive (an edge of no length) gives 0: the edge acts as its first point
RA_MESH_HD float m_ratio(float num, float den) { return den > 0.f ? fminf(fmaxf(m_div(num, den), 0.f), 1.f) : 0.f; }

struct MeshHit { float d2, x, y, z, u, v, w; };

// closest point of segment o + t e, t in [0, 1]
RA_MESH_HD float m_segment(const float p[3], const float o[3], const float e[3], float num, float q[3], float& t) {
    t = m_ratio(num, m_dot(e[0], e[1], e[2], e[0], e[1], e[2]));
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = m_fma(t, e[k], o[k]);
    return m_dot(p[0] - q[0], p[1] - q[1], p[2] - q[2], p[0] - q[0], p[1] - q[1], p[2] - q[2]);
}

// Ericson, Real-Time Collision Detection 5.1.5 (ClosestPtPointTriangle): the vertex, edge and face regions of p's projection
// An edge region is only taken for an edge of some length: Ericson's conditions hold trivially for a == b (d1 = d3 = vc = 0) and would
// answer a where the face, then the segment ac, has a closer point.
RA_MESH_HD MeshHit mesh_closest_tri(const float p[3], const float a[3], const float b[3], const float c[3]) {
    float ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; bp[k] = p[k] - b[k]; cp[k] = p[k] - c[k]; }
    const float d1 = m_dot(ab[0], ab[1], ab[2], ap[0], ap[1], ap[2]), d2 = m_dot(ac[0], ac[1], ac[2], ap[0], ap[1], ap[2]);
    const float d3 = m_dot(ab[0], ab[1], ab[2], bp[0], bp[1], bp[2]), d4 = m_dot(ac[0], ac[1], ac[2], bp[0], bp[1], bp[2]);
    const float d5 = m_dot(ab[0], ab[1], ab[2], cp[0], cp[1], cp[2]), d6 = m_dot(ac[0], ac[1], ac[2], cp[0], cp[1], cp[2]);
    const float vc = m_fma(d1, d4, -m_mul(d3, d2));
    const float vb = m_fma(d5, d2, -m_mul(d1, d6));
    const float va = m_fma(d3, d6, -m_mul(d5, d4));
    const float e43 = d4 - d3, e56 = d5 - d6;
    float q[3], u, v, w;
    if (d1 <= 0.f && d2 <= 0.f) {
        u = 1.f; v = 0.f; w = 0.f;
        q[0] = a[0]; q[1] = a[1]; q[2] = a[2];
    } else if (d3 >= 0.f && d4 <= d3) {
        u = 0.f; v = 1.f; w = 0.f;
        q[0] = b[0]; q[1] = b[1]; q[2] = b[2];
    } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f && d1 - d3 > 0.f) {    // edge ab (of some length: with a == b, d1 = d3 = 0 say nothing)
        v = m_ratio(d1, d1 - d3); u = 1.f - v; w = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = m_fma(v, ab[k], a[k]);
    } else if (d6 >= 0.f && d5 <= d6) {
        u = 0.f; v = 0.f; w = 1.f;
        q[0] = c[0]; q[1] = c[1]; q[2] = c[2];
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f && d2 - d6 > 0.f) {    // edge ac
        w = m_ratio(d2, d2 - d6); u = 1.f - w; v = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = m_fma(w, ac[k], a[k]);
    } else if (va <= 0.f && e43 >= 0.f && e56 >= 0.f && e43 + e56 > 0.f) {   // edge bc
        w = m_ratio(e43, e43 + e56); v = 1.f - w; u = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = m_fma(w, c[k] - b[k], b[k]);
    } else {
        // the face, or no region at all (a collinear face: the areas carry no sign).  On a sliver, and for a point far away, the three
        // areas are rounding noise and "all positive" says little, so the face's answer must also beat its three edges: what is kept
        // is never farther than the nearest edge point, and a face of no area acts as its edges
        float bc[3], q1[3], q2[3], q3[3], t1, t2, t3;
#pragma unroll
        for (int k = 0; k < 3; ++k) bc[k] = c[k] - b[k];
        const float e1 = m_segment(p, a, ab, d1, q1, t1);
        const float e2 = m_segment(p, a, ac, d2, q2, t2);
        const float e3 = m_segment(p, b, bc, m_dot(bc[0], bc[1], bc[2], bp[0], bp[1], bp[2]), q3, t3);
        float e;
        if (e1 <= e2 && e1 <= e3) { e = e1; u = 1.f - t1; v = t1; w = 0.f; q[0] = q1[0]; q[1] = q1[1]; q[2] = q1[2]; }
        else if (e2 <= e3) { e = e2; u = 1.f - t2; v = 0.f; w = t2; q[0] = q2[0]; q[1] = q2[1]; q[2] = q2[2]; }
        else { e = e3; u = 0.f; v = 1.f - t3; w = t3; q[0] = q3[0]; q[1] = q3[1]; q[2] = q3[2]; }
        if (va > 0.f && vb > 0.f && vc > 0.f) {                          // all three areas positive, so is their sum
            const float s = (va + vb) + vc;
            const float vi = fminf(m_div(vb, s), 1.f), wi = fminf(m_div(vc, s), 1.f);
            float qi[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) qi[k] = m_fma(wi, ac[k], m_fma(vi, ab[k], a[k]));
            if (m_dot(p[0] - qi[0], p[1] - qi[1], p[2] - qi[2], p[0] - qi[0], p[1] - qi[1], p[2] - qi[2]) <= e) {
                v = vi; w = wi; u = (1.f - vi) - wi;
                q[0] = qi[0]; q[1] = qi[1]; q[2] = qi[2];
            }
        }
    }
    MeshHit h;
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    h.d2 = m_dot(dx, dy, dz, dx, dy, dz);
    h.x = q[0]; h.y = q[1]; h.z = q[2]; h.u = u; h.v = v; h.w = w;
    return h;
}

// squared distance from p to a box and to its farthest corner, in d2's operations (an empty box, lo = +inf and hi = -inf: +inf both)
RA_MESH_HD float m_box_near(const float p[3], const float* bx) {
    const float dx = fmaxf(fmaxf(bx[0] - p[0], p[0] - bx[3]), 0.f);
    const float dy = fmaxf(fmaxf(bx[1] - p[1], p[1] - bx[4]), 0.f);
    const float dz = fmaxf(fmaxf(bx[2] - p[2], p[2] - bx[5]), 0.f);
    return m_dot(dx, dy, dz, dx, dy, dz);
}
RA_MESH_HD float m_box_far(const float p[3], const float* bx) {
    const float dx = fmaxf(fabsf(p[0] - bx[0]), fabsf(p[0] - bx[3]));
    const float dy = fmaxf(fabsf(p[1] - bx[1]), fabsf(p[1] - bx[4]));
    const float dz = fmaxf(fabsf(p[2] - bx[2]), fabsf(p[2] - bx[5]));
    return m_dot(dx, dy, dz, dx, dy, dz);
}

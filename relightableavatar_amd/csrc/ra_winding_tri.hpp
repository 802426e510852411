// The per-pair arithmetic of ra_winding.hip as a host + device function: the signed solid angle of one triangle (a, b, c) seen from a
// point p, in named fp32 operations (ra_mesh_tri.hpp's m_mul / m_fma / m_div, contraction off), so that a (point, face) pair has ONE
// value whatever kernel, loop or launch shape computes it, and a stand-alone CPU program (tests/native/winding_tri_main.cpp) runs the
// same operations.
//
// The function is the reference's winding_number (lib/utils/mesh_utils.py:614-680), its eps included:
//     u_i = (v_i - p) / |v_i - p|,  sign = sign(det[u0 u1 u2]),  Omega = 4 atan(sqrt(T + 1e-10)),  T = tan^2(Omega_0 / 4),
// contribution sign * Omega, exactly 0 where det == 0.  The reference forms T by L'Huilier's product of four half-angle tangents over
// asin(l / 2), which is ill-conditioned in fp32; here tan(Omega_0 / 4) comes from the half-angle form of Van Oosterom and Strackee,
//     tan(Omega_0 / 2) = |det| / den,  den = 1 + u0.u1 + u1.u2 + u2.u0,
//     tan(Omega_0 / 4) = |det| / (hypot(det, den) + den)          den >= 0
//                      = (hypot(det, den) - den) / |det|          den <  0      (the same value; no cancellation on either side),
// with det = (ab x bc) . (v - p) / (|a - p| |b - p| |c - p|), v the vertex nearest to p: the edges are differences of the inputs,
// not of unit vectors that nearly coincide for a small or distant face.
// NaN rules: a non-finite p gives NaN (inf - inf); p bit-equal to a vertex gives a zero length, 1 / 0 = inf and 0 * inf = NaN in den.
#pragma once
#include "ra_mesh_tri.hpp"

constexpr float WIND_EPS = 1e-10f;               // the reference's eps, under the root
constexpr float WIND_TAN_3PI_8 = 2.414213562373095f, WIND_TAN_PI_8 = 0.4142135623730950f;
constexpr float WIND_PI_2 = 1.5707963267948966f, WIND_PI_4 = 0.7853981633974483f;

#if defined(__HIP_DEVICE_COMPILE__)
RA_MESH_HD float w_sqrt(float a) { return __fsqrt_rn(a); }
#else
RA_MESH_HD float w_sqrt(float a) { return __builtin_sqrtf(a); }
#endif

// atan(x) for x >= 0 (+inf included; NaN stays NaN): the reduction and the degree-4 polynomial in x^2 of Cephes' atanf, with selects
// instead of branches and one division.  Within 2 units of 2^-24 of pi / 2 in absolute terms.
RA_MESH_HD float w_atan(float x) {
    const bool big = x > WIND_TAN_3PI_8, mid = x > WIND_TAN_PI_8;
    const float num = big ? -1.f : (mid ? x - 1.f : x), den = big ? x : (mid ? x + 1.f : 1.f);
    const float y0 = big ? WIND_PI_2 : (mid ? WIND_PI_4 : 0.f);
    const float r = m_div(num, den), z = m_mul(r, r);
    float q = m_fma(8.05374449538e-2f, z, -1.38776856032e-1f);
    q = m_fma(q, z, 1.99777106478e-1f);
    q = m_fma(q, z, -3.33329491539e-1f);
    return y0 + m_fma(m_mul(q, z), r, r);
}

// the signed solid angle of (a, b, c) seen from p, in [-2 pi, 2 pi]: positive where p is on the side the right-hand normal points AWAY
// from (inside a mesh whose faces are wound outwards)
RA_MESH_HD float winding_tri(const float p[3], const float a[3], const float b[3], const float c[3]) {
    float d0[3], d1[3], d2[3], ab[3], bc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { d0[k] = a[k] - p[k]; d1[k] = b[k] - p[k]; d2[k] = c[k] - p[k]; ab[k] = b[k] - a[k]; bc[k] = c[k] - b[k]; }
    const float q0 = m_dot(d0[0], d0[1], d0[2], d0[0], d0[1], d0[2]), q1 = m_dot(d1[0], d1[1], d1[2], d1[0], d1[1], d1[2]);
    const float q2 = m_dot(d2[0], d2[1], d2[2], d2[0], d2[1], d2[2]);
    const float i0 = m_div(1.f, w_sqrt(q0)), i1 = m_div(1.f, w_sqrt(q1)), i2 = m_div(1.f, w_sqrt(q2));
    const float nx = m_fma(ab[1], bc[2], -m_mul(ab[2], bc[1]));
    const float ny = m_fma(ab[2], bc[0], -m_mul(ab[0], bc[2]));
    const float nz = m_fma(ab[0], bc[1], -m_mul(ab[1], bc[0]));
    // (ab x bc) . (v - p) is the same for the three vertices v up to rounding, and the rounding grows with |v - p|: the nearest one
    const bool s01 = q1 < q0, s2 = q2 < fminf(q0, q1);
    const float ex = s2 ? d2[0] : (s01 ? d1[0] : d0[0]), ey = s2 ? d2[1] : (s01 ? d1[1] : d0[1]), ez = s2 ? d2[2] : (s01 ? d1[2] : d0[2]);
    const float det = m_mul(m_mul(m_dot(nx, ny, nz, ex, ey, ez), i2), m_mul(i0, i1));
    const float c01 = m_mul(m_dot(d0[0], d0[1], d0[2], d1[0], d1[1], d1[2]), m_mul(i0, i1));
    const float c12 = m_mul(m_dot(d1[0], d1[1], d1[2], d2[0], d2[1], d2[2]), m_mul(i1, i2));
    const float c20 = m_mul(m_dot(d2[0], d2[1], d2[2], d0[0], d0[1], d0[2]), m_mul(i2, i0));
    const float den = (1.f + c01) + (c12 + c20);
    const float ad = fabsf(det), h = w_sqrt(m_fma(det, det, m_mul(den, den)));
    const bool front = den >= 0.f;             // one division, operands selected: no divergence between lanes
    const float t = m_div(front ? ad : h - den, front ? h + den : ad);
    const float omega = m_mul(4.f, w_atan(w_sqrt(m_fma(t, t, WIND_EPS))));
    return det == 0.f ? 0.f : copysignf(omega, det);      // a NaN det (p on a vertex, a non-finite p) has a NaN omega
}

// The per-pair arithmetic of ra_winding_grad.hip as a host + device function: the signed solid angle of one triangle (a, b, c) seen
// from a point p AND its gradient with respect to p, in the named fp32 operations of ra_mesh_tri.hpp (contraction off), so that a
// (point, face) pair has ONE value and ONE gradient whatever kernel, loop or launch shape computes it, and a stand-alone CPU program
// (tests/native/winding_grad_tri_main.cpp) runs the same operations.
//
// The value is winding_tri's (ra_winding_tri.hpp), operation for operation: the same bits.  Everything it normalises with — d_i = v_i
// - p, their squared lengths q_i and reciprocal lengths i_i, the cosines c_ij, det, den, t = tan(Omega_0 / 4) and the root under the
// arctangent — is formed once and serves both results.
//
// The gradient is that of the function winding_tri computes, the reference's eps under the root included, in closed form:
//     grad_p (sign Omega) = k(T) sum over the edges (x, y) = (d0, d1), (d1, d2), (d2, d0) of (x cross y) (|x| + |y|) / (|x| |y| (|x| |y| + x.y))
//     k(T) = (1 + T) sqrt(T) / ((1 + T + eps) sqrt(T + eps)),      T = t^2,  eps = 1e-10.
// The edge sum is the Biot-Savart form of the gradient of the signed solid angle (it carries the sign); k is the derivative of
// 4 atan(sqrt(T + eps)) over that of 4 atan(sqrt(T)): far from 1 for a small or distant face (Omega_0 = 1e-5 gives T = 6e-12 < eps).
// In these operations
//     (|x| + |y|) / (|x| |y| (|x| |y| + x.y)) = (i_x + i_y) (i_x i_y) / (1 + c_xy)         with the cosine c_xy the value already has,
//     d0 cross d1 = d0 cross (b - a),  d1 cross d2 = d1 cross (c - b),  d2 cross d0 = d2 cross (a - c)
// (an edge is a difference of the inputs, not of two long vectors that nearly coincide for a distant face), and
//     k = t / sqrt(t^2 + eps):  (1 + T) / (1 + T + eps) differs from 1 by less than 1e-10, below fp32's resolution of 1.
// Rules.  det == 0 (a point in a face's plane, a face of no area): value 0 and gradient 0, as winding_tri's value.  Non-finite: a
// non-finite p, p bit-equal to a vertex (0 * inf in a cosine), and p on the segment of an edge, which is where the computed 1 + c_xy
// of an edge is not positive: the gradient is NaN there (the rule comes before det == 0: such a point lies in the face's plane).
#pragma once
#include "ra_winding_tri.hpp"

struct WindGrad { float omega, gx, gy, gz; };

RA_MESH_HD WindGrad winding_grad_tri(const float p[3], const float a[3], const float b[3], const float c[3]) {
    float d0[3], d1[3], d2[3], ab[3], bc[3], ca[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d0[k] = a[k] - p[k]; d1[k] = b[k] - p[k]; d2[k] = c[k] - p[k];
        ab[k] = b[k] - a[k]; bc[k] = c[k] - b[k]; ca[k] = a[k] - c[k];
    }
    // ---- winding_tri, line for line
    const float q0 = m_dot(d0[0], d0[1], d0[2], d0[0], d0[1], d0[2]), q1 = m_dot(d1[0], d1[1], d1[2], d1[0], d1[1], d1[2]);
    const float q2 = m_dot(d2[0], d2[1], d2[2], d2[0], d2[1], d2[2]);
    const float i0 = m_div(1.f, w_sqrt(q0)), i1 = m_div(1.f, w_sqrt(q1)), i2 = m_div(1.f, w_sqrt(q2));
    const float nx = m_fma(ab[1], bc[2], -m_mul(ab[2], bc[1]));
    const float ny = m_fma(ab[2], bc[0], -m_mul(ab[0], bc[2]));
    const float nz = m_fma(ab[0], bc[1], -m_mul(ab[1], bc[0]));
    const bool s01 = q1 < q0, s2 = q2 < fminf(q0, q1);
    const float ex = s2 ? d2[0] : (s01 ? d1[0] : d0[0]), ey = s2 ? d2[1] : (s01 ? d1[1] : d0[1]), ez = s2 ? d2[2] : (s01 ? d1[2] : d0[2]);
    const float i01 = m_mul(i0, i1), i12 = m_mul(i1, i2), i20 = m_mul(i2, i0);
    const float det = m_mul(m_mul(m_dot(nx, ny, nz, ex, ey, ez), i2), i01);
    const float c01 = m_mul(m_dot(d0[0], d0[1], d0[2], d1[0], d1[1], d1[2]), i01);
    const float c12 = m_mul(m_dot(d1[0], d1[1], d1[2], d2[0], d2[1], d2[2]), i12);
    const float c20 = m_mul(m_dot(d2[0], d2[1], d2[2], d0[0], d0[1], d0[2]), i20);
    const float den = (1.f + c01) + (c12 + c20);
    const float ad = fabsf(det), h = w_sqrt(m_fma(det, det, m_mul(den, den)));
    const bool front = den >= 0.f;
    const float t = m_div(front ? ad : h - den, front ? h + den : ad);
    const float root = w_sqrt(m_fma(t, t, WIND_EPS));
    const float omega = m_mul(4.f, w_atan(root));
    // ---- the gradient
    const float e01 = 1.f + c01, e12 = 1.f + c12, e20 = 1.f + c20;
    const float w01 = m_div(m_mul(i0 + i1, i01), e01), w12 = m_div(m_mul(i1 + i2, i12), e12), w20 = m_div(m_mul(i2 + i0, i20), e20);
    const float x01[3] = {m_fma(d0[1], ab[2], -m_mul(d0[2], ab[1])), m_fma(d0[2], ab[0], -m_mul(d0[0], ab[2])), m_fma(d0[0], ab[1], -m_mul(d0[1], ab[0]))};
    const float x12[3] = {m_fma(d1[1], bc[2], -m_mul(d1[2], bc[1])), m_fma(d1[2], bc[0], -m_mul(d1[0], bc[2])), m_fma(d1[0], bc[1], -m_mul(d1[1], bc[0]))};
    const float x20[3] = {m_fma(d2[1], ca[2], -m_mul(d2[2], ca[1])), m_fma(d2[2], ca[0], -m_mul(d2[0], ca[2])), m_fma(d2[0], ca[1], -m_mul(d2[1], ca[0]))};
    // t^2 overflows where the point all but lies in the face (root = inf): k is 1 there, as it is from t = 0.03 on
    const float k = root < INFINITY ? m_div(t, root) : 1.f;
    const bool off_edges = e01 > 0.f && e12 > 0.f && e20 > 0.f;      // false for a NaN cosine too
    const bool flat = det == 0.f;
    WindGrad g;
    g.omega = flat ? 0.f : copysignf(omega, det);
    g.gx = !off_edges ? NAN : (flat ? 0.f : m_mul(k, m_dot(x01[0], x12[0], x20[0], w01, w12, w20)));
    g.gy = !off_edges ? NAN : (flat ? 0.f : m_mul(k, m_dot(x01[1], x12[1], x20[1], w01, w12, w20)));
    g.gz = !off_edges ? NAN : (flat ? 0.f : m_mul(k, m_dot(x01[2], x12[2], x20[2], w01, w12, w20)));
    return g;
}

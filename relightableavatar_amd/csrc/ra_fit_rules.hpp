// The per-element rules of ra_fit.hip as host + device functions, so that a result has ONE value whatever kernel, loop or launch
// shape computes it, and a stand-alone CPU program (tests/native/fit_rules_main.cpp) runs the same operations.
//
// Everything here is float64 state behind fp32 inputs and outputs: an fp32 value is widened exactly, every line below is one named
// operation of one rounding (contraction off), and a stored fp32 result is rounded once at the end.
//
// The operator M = I + lambda L, L = D - A the combinatorial Laplacian of the unique edges (largesteps' compute_matrix): for ONE
// (vertex, channel) with value x, deg neighbours OTHER than the vertex itself and their ascending sum s (from 0; an entry of the
// neighbour list that names the vertex itself, which an edge (a, a) makes, is skipped in both: it cancels between D and A):
//     t = deg * x,   u = t - s,   w = lambda * u,   M x = x + w                                   (fit_diffuse)
// The Jacobi preconditioner is M's diagonal, d = 1 + lambda * deg (fit_diag).
//
// Normals.  e1 = b - a, e2 = c - b, n = e1 x e2 with every component (p = y1 z2, q = z1 y2, p - q); |n| = sqrt((nx nx + ny ny) + nz nz)
// (fit_cross, fit_norm).  Face normal n / (|n| + 1e-8); face area |(c - a) x (b - a)| / 2; vertex normal: the ascending sum of the
// unnormalised n over the outgoing half-edges, divided by max(|.|, 1e-6).
//
// ICP.  delta = p - closest; kept when d2 < fl32(dist_th dist_th) (fp32, d2 as ra_mesh_closest gives it) and
// (n1x n0x + n1y n0y) + n1z n0z > angle_th (float64 of the fp32 inputs); |delta|^2 = (dx dx + dy dy) + dz dz;
// grad = (2 / count) delta, rounded once.
//
// AdamUniform (largesteps.optimize), per element with the tensor's one scalar m = max |grad| (so max grad^2 = m m, exact in float64):
//     g1' = fl32(b1 g1 + (1 - b1) grad)            a = b1 g1, c = (1 - b1) grad, a + c
//     g2' = fl32(b2 g2 + (1 - b2) (m m))
//     p'  = fl32(p - lr (g1' / c1) / (1e-8 + sqrt(g2' / c2)))        c1 = 1 - b1^t, c2 = 1 - b2^t, the powers by t - 1 multiplications
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define RA_FIT_HD __host__ __device__ __forceinline__
#else
#define RA_FIT_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

RA_FIT_HD double fit_diffuse(double x, double s, int deg, double lambda) {
    const double t = (double)deg * x;
    const double u = t - s;
    const double w = lambda * u;
    return x + w;
}
RA_FIT_HD double fit_diag(int deg, double lambda) {
    const double w = lambda * (double)deg;
    return 1.0 + w;
}

RA_FIT_HD void fit_cross(const double* a, const double* b, double* o) {
    const double p0 = a[1] * b[2], q0 = a[2] * b[1];
    const double p1 = a[2] * b[0], q1 = a[0] * b[2];
    const double p2 = a[0] * b[1], q2 = a[1] * b[0];
    o[0] = p0 - q0; o[1] = p1 - q1; o[2] = p2 - q2;
}
RA_FIT_HD double fit_dot(const double* a, const double* b) {
    const double x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
    const double xy = x + y;
    return xy + z;
}
RA_FIT_HD double fit_norm(const double* a) { return sqrt(fit_dot(a, a)); }

// the unnormalised normal (b - a) x (c - b) of a triangle of fp32 corners
RA_FIT_HD void fit_face_normal_raw(const float* a, const float* b, const float* c, double* n) {
    double e1[3], e2[3];
    for (int k = 0; k < 3; ++k) { e1[k] = (double)b[k] - (double)a[k]; e2[k] = (double)c[k] - (double)b[k]; }
    fit_cross(e1, e2, n);
}
RA_FIT_HD void fit_face_normal(const double* n, float* out) {
    const double d = fit_norm(n) + 1e-8;
    for (int k = 0; k < 3; ++k) out[k] = (float)(n[k] / d);
}
RA_FIT_HD float fit_face_area(const float* a, const float* b, const float* c) {
    double u[3], v[3], x[3];
    for (int k = 0; k < 3; ++k) { u[k] = (double)c[k] - (double)a[k]; v[k] = (double)b[k] - (double)a[k]; }
    fit_cross(u, v, x);
    return (float)(fit_norm(x) / 2.0);
}
RA_FIT_HD void fit_vert_normal(const double* sum, float* out) {
    const double l = fit_norm(sum), d = l > 1e-6 ? l : 1e-6;      // a NaN length divides by 1e-6 and stays NaN through the sum
    for (int k = 0; k < 3; ++k) out[k] = (float)(sum[k] / d);
}

RA_FIT_HD bool fit_icp_keep(float d2, float dist_th, const float* n1, const float* n0, float angle_th) {
    const float th2 = dist_th * dist_th;
    const double a[3] = {(double)n1[0], (double)n1[1], (double)n1[2]}, b[3] = {(double)n0[0], (double)n0[1], (double)n0[2]};
    return d2 < th2 && fit_dot(a, b) > (double)angle_th;
}
RA_FIT_HD float fit_icp_grad(double delta, double count) {
    const double w = 2.0 / count;
    return (float)(w * delta);
}

inline double fit_pow(double b, int t) {      // b^t by t - 1 multiplications: the same bits on every host
    double p = 1.0;
    for (int i = 0; i < t; ++i) p = p * b;
    return p;
}
RA_FIT_HD float fit_adam_moment(float state, double value, double b) {
    const double a = b * (double)state;
    const double c = (1.0 - b) * value;
    return (float)(a + c);
}
RA_FIT_HD float fit_adam_param(float p, float g1, float g2, double lr, double c1, double c2) {
    const double m1 = (double)g1 / c1;
    const double m2 = (double)g2 / c2;
    const double den = 1e-8 + sqrt(m2);
    const double q = m1 / den;
    const double step = lr * q;
    return (float)((double)p - step);
}

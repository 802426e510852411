// The per-element rules of ra_cloth.hip as host + device functions, so that an element has ONE value whatever kernel or launch shape
// computes it, and a stand-alone CPU program (tests/native/cloth_rules_main.cpp) runs the same operations.
//
// Every function is a template on the scalar type: the kernels instantiate float (every line below is then one named fp32 operation of
// one rounding, contraction off), the host program also instantiates double and compares the two.  What the reference's
// lib/utils/physx_utils.py computes, per element:
//
// Material space (Garment.__init__): Dm = [m0 - m2 | m1 - m2] of the 2-D triangle, inverted as torch_inverse_2x2 does:
//     det = (a d - b c) + 2^-23,  Dm_inv = [d, -b; -c, a] / det.       The 2^-23 is added in WHATEVER precision.
//
// Stretch (stretch_energy, :242-267), one face: Ds = [x0 - x2 | x1 - x2], F = Ds Dm_inv (3 x 2), C = F^T F, G = (C - I) / 2,
//     tr = G00 + G11, S = mu G + (lambda / 2) tr I, psi = sum_ij S_ij G_ij, E = (area thickness) psi.
// Gradient: dpsi/dF = 2 F S =: P, dpsi/dDs = P Dm_inv^T =: H, dE/dx0 = k H0, dE/dx1 = k H1, dE/dx2 = -(dE/dx0 + dE/dx1).
//
// Bending (bending_energy, :270-311), one hinge = two faces (a0 a1 a2), (b0 b1 b2) over the edge v0 -> v1:
//     r = (a1 - a0) x (a2 - a1), n0 = r / (|r| + 1e-8), n1 likewise, e = v1 - v0, l = |e|, en = e / l,
//     cos = n0 . n1, sin = en . (n0 x n1), theta = atan2(sin, cos), E = coeff (l l / (4 (area0 + area1))) theta theta / 2.
// The energy does not depend on which of the two faces comes first: swapping them negates sin when the edge keeps its direction and
// theta enters squared, so the reference's unstable argsort inside get_face_connectivity does not matter.
// Gradient: reverse mode through theta, sin, cos, en, l and both normalisations, written out in cloth_bending.
//
// Gravity: g mass y.   Inertia (inertia_term / dynamic_term, :322-351): d = x_next - (x_curr + dt v (+ dt dt a)),
//     value = (d . d) mass / (2 dt dt); d/dx_next = d mass / (dt dt), d/dx_curr = -that, d/dv = -dt that.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define RA_CLOTH_HD __host__ __device__ __forceinline__
#else
#define RA_CLOTH_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

template <typename T> RA_CLOTH_HD T cloth_sqrt(T x) { return (T)sqrt((double)x); }
template <> RA_CLOTH_HD float cloth_sqrt<float>(float x) { return sqrtf(x); }
template <typename T> RA_CLOTH_HD T cloth_atan2(T y, T x) { return (T)atan2((double)y, (double)x); }
template <> RA_CLOTH_HD float cloth_atan2<float>(float y, float x) { return atan2f(y, x); }

template <typename T> RA_CLOTH_HD T cloth_dot(const T* a, const T* b) {
    const T x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
    const T xy = x + y;
    return xy + z;
}
template <typename T> RA_CLOTH_HD void cloth_cross(const T* a, const T* b, T* o) {
    const T p0 = a[1] * b[2], q0 = a[2] * b[1];
    const T p1 = a[2] * b[0], q1 = a[0] * b[2];
    const T p2 = a[0] * b[1], q2 = a[1] * b[0];
    o[0] = p0 - q0; o[1] = p1 - q1; o[2] = p2 - q2;
}
template <typename T> RA_CLOTH_HD void cloth_sub(const T* a, const T* b, T* o) { o[0] = a[0] - b[0]; o[1] = a[1] - b[1]; o[2] = a[2] - b[2]; }
// o = a s + b t
template <typename T> RA_CLOTH_HD void cloth_comb(const T* a, T s, const T* b, T t, T* o) {
    for (int k = 0; k < 3; ++k) {
        const T p = a[k] * s, q = b[k] * t;
        o[k] = p + q;
    }
}

// get_face_areas: |(c - a) x (b - a)| / 2
template <typename T> RA_CLOTH_HD T cloth_face_area(const T* a, const T* b, const T* c) {
    T u[3], v[3], x[3];
    cloth_sub(c, a, u);
    cloth_sub(b, a, v);
    cloth_cross(u, v, x);
    return cloth_sqrt(cloth_dot(x, x)) / (T)2;
}

// Dm_inv (row-major 2 x 2) of the material triangle m0, m1, m2 (2-D each)
template <typename T> RA_CLOTH_HD void cloth_dm_inv(const T* m0, const T* m1, const T* m2, T* dm, T* inv) {
    const T a = m0[0] - m2[0], b = m1[0] - m2[0], c = m0[1] - m2[1], d = m1[1] - m2[1];
    const T ad = a * d, bc = b * c;
    const T det0 = ad - bc;
    const T det = det0 + (T)1.1920928955078125e-07;
    if (dm) { dm[0] = a; dm[1] = b; dm[2] = c; dm[3] = d; }
    inv[0] = d / det; inv[1] = -b / det; inv[2] = -c / det; inv[3] = a / det;
}

// one face's share of a corner's mass: (density area) / 3
template <typename T> RA_CLOTH_HD T cloth_mass_share(T density, T area) {
    const T m = density * area;
    return m / (T)3;
}

// stretch energy of one face and (g != nullptr) its gradient with respect to the three corners, g[3 k + c]
template <typename T> RA_CLOTH_HD T cloth_stretch(const T* x0, const T* x1, const T* x2, const T* m, T area, T thickness, T mu, T lambda, T* g) {
    T d0[3], d1[3], f0[3], f1[3];
    cloth_sub(x0, x2, d0);
    cloth_sub(x1, x2, d1);
    cloth_comb(d0, m[0], d1, m[2], f0);
    cloth_comb(d0, m[1], d1, m[3], f1);
    const T c00 = cloth_dot(f0, f0), c01 = cloth_dot(f0, f1), c11 = cloth_dot(f1, f1);
    const T h = (T)0.5;
    const T g00 = h * (c00 - (T)1), g01 = h * c01, g11 = h * (c11 - (T)1);
    const T tr = g00 + g11;
    const T hl = h * lambda;
    const T iso = hl * tr;
    const T s00 = mu * g00 + iso, s01 = mu * g01, s11 = mu * g11 + iso;
    const T p00 = s00 * g00, p01 = s01 * g01, p11 = s11 * g11;
    const T off = p01 + p01;
    const T psi = (p00 + off) + p11;
    const T k = area * thickness;
    if (g) {
        T P0[3], P1[3], H0[3], H1[3];
        cloth_comb(f0, s00, f1, s01, P0);
        cloth_comb(f0, s01, f1, s11, P1);
        cloth_comb(P0, m[0], P1, m[1], H0);
        cloth_comb(P0, m[2], P1, m[3], H1);
        const T k2 = k + k;
        for (int c = 0; c < 3; ++c) {
            const T a = k2 * H0[c], b = k2 * H1[c];
            g[c] = a; g[3 + c] = b; g[6 + c] = -(a + b);
        }
    }
    return k * psi;
}

// r = (p1 - p0) x (p2 - p1), n = r / (|r| + 1e-8); keeps what the gradient needs
template <typename T> struct ClothNormal { T p[3], q[3], r[3], n[3], len, d; };
template <typename T> RA_CLOTH_HD void cloth_normal(const T* p0, const T* p1, const T* p2, ClothNormal<T>& o) {
    cloth_sub(p1, p0, o.p);
    cloth_sub(p2, p1, o.q);
    cloth_cross(o.p, o.q, o.r);
    o.len = cloth_sqrt(cloth_dot(o.r, o.r));
    o.d = o.len + (T)1e-8;
    for (int k = 0; k < 3; ++k) o.n[k] = o.r[k] / o.d;
}
// the gradient gn with respect to n, pulled back to the three corners: g[3 k + c] = ... (9 values, written)
template <typename T> RA_CLOTH_HD void cloth_normal_back(const ClothNormal<T>& o, const T* gn, T* g) {
    const T w = cloth_dot(gn, o.r) / o.len;
    T gr[3], gp[3], gq[3];
    for (int k = 0; k < 3; ++k) {
        const T t = o.n[k] * w;
        gr[k] = (gn[k] - t) / o.d;
    }
    cloth_cross(o.q, gr, gp);
    cloth_cross(gr, o.p, gq);
    for (int c = 0; c < 3; ++c) {
        g[c] = (T)0 - gp[c];
        g[3 + c] = gp[c] - gq[c];
        g[6 + c] = gq[c];
    }
}

// bending energy of one hinge: faces a[0..2], b[0..2] (pointers to corners), the edge from a[k0] to b[k1]; area_sum = area0 + area1 of
// the rest faces.  GRAD: g receives 18 values, the gradient with respect to a0 a1 a2 b0 b1 b2, the edge's share folded into a[k0], b[k1];
// else g is not touched.  A template argument, and the fold below selects VALUES at constant indices: g stays in registers on the device.
template <bool GRAD, typename T> RA_CLOTH_HD T cloth_bending(const T* const* a, const T* const* b, int k0, int k1, T area_sum, T coeff, T* g) {
    ClothNormal<T> A, B;
    cloth_normal(a[0], a[1], a[2], A);
    cloth_normal(b[0], b[1], b[2], B);
    T e[3], en[3], nx[3];
    const T* v0 = k0 == 0 ? a[0] : k0 == 1 ? a[1] : a[2];     // selects, not indexed: the arrays stay in registers
    const T* v1 = k1 == 0 ? b[0] : k1 == 1 ? b[1] : b[2];
    cloth_sub(v1, v0, e);
    const T l = cloth_sqrt(cloth_dot(e, e));
    for (int k = 0; k < 3; ++k) en[k] = e[k] / l;
    const T cs = cloth_dot(A.n, B.n);
    cloth_cross(A.n, B.n, nx);
    const T sn = cloth_dot(en, nx);
    const T theta = cloth_atan2(sn, cs);
    const T ll = l * l, a4 = (T)4 * area_sum;
    const T scale = ll / a4;
    const T cscale = coeff * scale;
    const T t2 = theta * theta;
    const T energy = cscale * t2 / (T)2;
    if (GRAD) {
        const T gth = cscale * theta;                       // dE/dtheta
        const T gl = coeff * t2 * l / a4;                   // dE/dl through the scale
        const T r2 = sn * sn + cs * cs;
        const T gsn = gth * cs / r2, gcs = -(gth * sn) / r2;
        T x0[3], x1[3], gn0[3], gn1[3], gen[3], ge[3];
        cloth_cross(B.n, en, x0);                           // d sin / d n0
        cloth_cross(en, A.n, x1);                           // d sin / d n1
        cloth_comb(B.n, gcs, x0, gsn, gn0);
        cloth_comb(A.n, gcs, x1, gsn, gn1);
        for (int k = 0; k < 3; ++k) gen[k] = gsn * nx[k];
        const T along = cloth_dot(gen, en);
        for (int k = 0; k < 3; ++k) {
            const T t = en[k] * along;
            const T u = (gen[k] - t) / l;
            const T v = gl * en[k];
            ge[k] = u + v;
        }
        cloth_normal_back(A, gn0, g);
        cloth_normal_back(B, gn1, g + 9);
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < 3; ++c) {
                const T s0 = k == k0 ? ge[c] : (T)0, s1 = k == k1 ? ge[c] : (T)0;
                g[3 * k + c] = g[3 * k + c] - s0;
                g[9 + 3 * k + c] = g[9 + 3 * k + c] + s1;
            }
    }
    return energy;
}

template <typename T> RA_CLOTH_HD T cloth_gravity(T g, T mass, T y) {
    const T gm = g * mass;
    return gm * y;
}

// accel nullable (inertia_term); g_next (nullable) receives d value / d x_next
template <typename T> RA_CLOTH_HD T cloth_inertia(const T* xn, const T* xc, const T* vc, T mass, T dt, const T* accel, T* g_next) {
    T d[3];
    const T dt2 = dt * dt;
    for (int k = 0; k < 3; ++k) {
        const T step = dt * vc[k];
        T pred = xc[k] + step;
        if (accel) {
            const T acc = dt2 * accel[k];
            pred = pred + acc;
        }
        d[k] = xn[k] - pred;
    }
    const T sq = cloth_dot(d, d);
    const T den = (T)2 * dt2;
    if (g_next)
        for (int k = 0; k < 3; ++k) g_next[k] = d[k] * mass / dt2;
    return sq * mass / den;
}

// the StVK coefficients of the reference's StVKMaterial.__init__, in double: out = A, stretch_coeff, bending_coeff, lame_mu, lame_lambda
inline void cloth_material(double thickness, double young, double poisson, double bend_mul, double stretch_mul, double mat_mul, double* out) {
    const double A = young / (1.0 - poisson * poisson);
    double sc = A;
    sc *= stretch_mul * mat_mul;
    double bc = A / 12.0 * pow(thickness, 3.0);
    bc *= bend_mul * mat_mul;
    out[0] = A; out[1] = sc; out[2] = bc; out[3] = 0.5 * sc * (1.0 - poisson); out[4] = sc * poisson;
}

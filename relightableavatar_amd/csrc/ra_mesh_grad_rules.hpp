// The per-row rule of ra_mesh_grad.hip (ra_mesh_closest_backward) as host + device functions, in the style of ra_mesh_tri.hpp whose
// named fp32 operations it uses: a row has ONE result whichever thread, kernel or CPU program (tests/native/
// mesh_closest_grad_rules_main.cpp) evaluates it.  Every line is one named fp32 operation of one rounding, contraction off.
//
// Row i: p the query point, q / f / b the forward's stored closest point, face and barycentrics, g the upstream gradient of d2 (the
//     SQUARED distance), ga[C] the upstream gradient of C attribute channels interpolated at the closest point.
// closest = sum_k b_k v_k minimises |p - x|^2 over a feasible set (the triangle) that does not depend on the vertices' positions in
//     barycentric coordinates, so with (f, b) held fixed   d(d2)/dp = 2 (p - q),   d(d2)/dv_k = -2 b_k (p - q)
//     in the face, edge and vertex regions alike.
// Live: 0 <= f < F and the face's three vertex indices lie in [0, V).  Otherwise dead.
//     live:  dpts[i][c] = (2 g) * (p[c] - q[c]): one subtraction, one product (2 g is exact);
//            slot (i, k), k = 0..2, belongs to vertex faces[f][k] and carries  -(b[k] * dpts[i][c])  for dverts (the negation is exact)
//            and  b[k] * ga[ch]  for dattr.
//     dead:  dpts[i] = +0, no slot.
// Non-finite values of a live row are not filtered: they reach that row's dpts and its three vertices and nothing else.
// A vertex's result is the sum of its slots in ascending 3 i + k, taken as the wave sum of ra_texture.hip's header: lane l adds terms
//     l, l + 64, ... from +0, the lanes meet in the xor tree 32, 16, .., 1.  A vertex without a slot gets +0.
#pragma once
#include "ra_mesh_tri.hpp"

constexpr int MESHG_MAX_C = 64;         // attribute channels per row at most

// the three vertex indices of row's face into idx; false for a dead row (idx is then not to be read)
RA_MESH_HD bool mesh_grad_live(int f, const int* faces, int F, int V, int idx[3]) {
    if (f < 0 || f >= F) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        idx[k] = faces[3ll * f + k];
        if (idx[k] < 0 || idx[k] >= V) return false;
    }
    return true;
}

// d L / d p of a live row
RA_MESH_HD void mesh_grad_dpts(const float p[3], const float q[3], float g, float out[3]) {
    const float g2 = m_mul(2.f, g);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = m_mul(g2, p[c] - q[c]);
}

// the payload of a slot: what corner k (barycentric b) of the row's face receives of one component of dpts, of one attribute channel
RA_MESH_HD float mesh_grad_vert_term(float b, float dp) { return -m_mul(b, dp); }
RA_MESH_HD float mesh_grad_attr_term(float b, float ga) { return m_mul(b, ga); }

// The per-element rules of ra_topo.hip as host + device functions, so that a result has ONE value whatever kernel, loop or launch
// shape computes it, and a stand-alone CPU program (tests/native/topo_rules_main.cpp) runs the same operations.
//
// Half-edges.  Half-edge h = 3 f + k starts at corner k of face f and runs to corner (k + 1) % 3; topo_next / topo_prev stay inside
// the face.  Its edge key is (min << 32) | max of its two vertices: the unsigned order of the keys is the lexicographic order of
// (min, max), the order the reference's hash.unique numbers edges in (lib/utils/mesh_utils.py:564-566).
//
// Taubin smoothing (laplacian / laplacian_smoothing, mesh_utils.py:943-1015), one pass for ONE (vertex, channel), named fp32
// operations with one rounding each, contraction off:
//     s  = ((0 + x[n_0]) + x[n_1]) + ...          the neighbours n_k in ascending order (taubin_sum is the caller's loop)
//     m  = s * inv                                 inv = 1.0f / deg, or 0 for deg = 0
//     l  = m - v
//     v' = v + c * l                               p = c * l, then v + p
// with c = alpha in the first pass of an iteration and c = -(alpha + 0.01f) (one rounded sum, negated) in the second.  A vertex
// without neighbours has l = -v, as the reference's L = -I row has.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RA_TOPO_HD __host__ __device__ __forceinline__
#else
#define RA_TOPO_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

RA_TOPO_HD int topo_next(int h) { return h - h % 3 + (h + 1) % 3; }
RA_TOPO_HD int topo_prev(int h) { return h - h % 3 + (h + 2) % 3; }

RA_TOPO_HD uint64_t topo_edge_key(int a, int b) {
    const uint32_t lo = (uint32_t)(a < b ? a : b), hi = (uint32_t)(a < b ? b : a);
    return ((uint64_t)lo << 32) | (uint64_t)hi;
}
RA_TOPO_HD int topo_key_min(uint64_t key) { return (int)(uint32_t)(key >> 32); }
RA_TOPO_HD int topo_key_max(uint64_t key) { return (int)(uint32_t)key; }

// twin of the half-edge at position `pos` of its edge's run [start, start + count) in the sorted order: the other one of a pair,
// -count otherwise (mesh_utils.py:580-593)
RA_TOPO_HD int topo_twin_pos(int pos, int start, int count) { return count == 2 ? 2 * start + 1 - pos : -1; }

RA_TOPO_HD float taubin_inv(int deg) { return deg > 0 ? 1.0f / (float)deg : 0.0f; }
RA_TOPO_HD float taubin_coeff(float alpha, int second) { return second ? -(alpha + 0.01f) : alpha; }
RA_TOPO_HD float taubin_step(float v, float s, float inv, float c) {
    const float m = s * inv;
    const float l = m - v;
    const float p = c * l;
    return v + p;
}

// ---- one Loop subdivision step (halfedge_loop_subdivision, mesh_utils.py:382-514) ----------------------------------------------
// Positions are sums of per-half-edge contributions; the caller adds them in ascending half-edge order from 0.  For half-edge h from
// v = vert[h] to v_next, v_prev the third corner, every line one rounded fp32 operation:
//   the edge vertex V + edge[h]:   twin[h] >= 0:  a = 3 v, b = a + v_prev, b * 0.125        (loop_edge_inner; * 0.125 is exact)
//                                  twin[h] = -c:  s = v + v_next, s / (2 c)                  (loop_edge_open)
//   the old vertex vert[h], none of whose outgoing half-edges has twin < 0:
//                                  a = w_self v, b = beta v_next, a + b                      (loop_vert_inner)
//       w_self = 1 / n - beta, beta = (1 / n)(5 / 8 - (3 / 8 + cos(2 pi / n) / 4)^2), n the half-edges that leave the vertex:
//       computed in double and rounded ONCE to fp32 (loop_weights; the library's table, ra_loop_weights)
//   any other old vertex: 0, plus   a = 0.125 v_next, b = 0.375 v, a + b                     (loop_vert_open)  when twin[h] < 0
//                                   the same with (w, v)                                      when tp = twin[prev h] >= 0 and
//       twin[prev tp] < 0, w = the start of prev tp: the boundary half-edge that ARRIVES at the vertex (mesh_utils.py:489-490).
//       A contribution is ((0 | inner) + open) + mirrored, in that order.
// A vertex that belongs to one face only gets half its stencil and an unreferenced vertex moves to the origin, as in the reference.
#include <cmath>

RA_TOPO_HD float loop_edge_inner(float v, float v_prev) {
    const float a = 3.0f * v;
    const float b = a + v_prev;
    return b * 0.125f;
}
RA_TOPO_HD float loop_edge_open(float v, float v_next, int count) {
    const float s = v + v_next;
    return s / (float)(2 * count);
}
RA_TOPO_HD float loop_vert_inner(float v, float v_next, float w_self, float beta) {
    const float a = w_self * v;
    const float b = beta * v_next;
    return a + b;
}
RA_TOPO_HD float loop_vert_open(float v, float other) {
    const float a = 0.125f * other;
    const float b = 0.375f * v;
    return a + b;
}
inline void loop_weights(int n, float* w_self, float* beta) {       // host: double, rounded once
    if (n < 1) { *w_self = 0.0f; *beta = 0.0f; return; }
    const double k = 0.375 + 0.25 * std::cos(2.0 * 3.14159265358979323846 / (double)n);
    const double b = (1.0 / (double)n) * (0.625 - k * k);
    *w_self = (float)(1.0 / (double)n - b);
    *beta = (float)b;
}

// The child's connectivity (mesh_utils.py:419-451).  Half-edge h of HE becomes 3 h (from vert[h] to the edge vertex), 3 h + 1 (edge
// vertex of h to edge vertex of prev h) and 3 h + 2 (edge vertex of prev h to vert[h]): the corner face of vert[h]; 3 HE + h is the
// half-edge of the middle face opposite 3 h + 1.  tw = twin[h], tp = twin[prev h]; nothing is read through a negative twin.
RA_TOPO_HD int child_twin0(int tw) { return tw >= 0 ? 3 * topo_next(tw) + 2 : tw; }
RA_TOPO_HD int child_twin2(int tp) { return tp >= 0 ? 3 * tp : tp; }
RA_TOPO_HD int child_edge0(int e, int h, int tw) { return tw >= 0 ? 2 * e + (h < tw ? 1 : 0) : 2 * e; }
RA_TOPO_HD int child_edge2(int e_prev, int prev, int tp) { return tp >= 0 ? 2 * e_prev + (prev > tp ? 1 : 0) : 2 * e_prev + 1; }

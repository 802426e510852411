// The per-edge rule of ra_mcubes_grad.hip as host + device functions, in the style of ra_raster_rules.hpp: a crossed grid edge has ONE
// result whichever thread, kernel or CPU program (tests/native/mcubes_grad_rules_main.cpp) evaluates it.  Every line is one named fp32
// operation of one rounding, contraction off.  Nothing here is read by the forward (ra_mcubes.hip); the two statements of t — mc_interp
// there, mcg_edge here — are the same three operations and the tests hold them to the same bits.
//
// Edge.  Owned by grid point p along `axis`, q its other end, a = vol[p], b = vol[q]; crossed when (a < iso) != (b < iso) (a NaN is
//     not below).  Its vertex index is off[p] + popc(mask[p] & ((1 << axis) - 1)): the forward's rule.
// d = b - a (never 0 on a crossed edge), t = (iso - a) / d.
// Attribute forward: attr[v][c] = (1 - t) A[p][c] + t A[q][c]: two products, one add.
// Backward, the set of crossed edges held fixed.  gt = dverts[v][axis] (+0 without dverts), then for c ascending
//     gt += dattr[v][c] * (A[q][c] - A[p][c]), each product rounded, then added.  s = gt / d.
//     to p: ca = (t - 1) s;  to q: cb = -(t s);  dA[p][c] += (1 - t) dattr[v][c];  dA[q][c] += t dattr[v][c].
// A grid point g adds its terms from +0 in the order: its own edges towards +x, +y, +z (g is the a end), then the edges arriving from
//     -x, -y, -z (g is the b end); absent edges are skipped.  A gather: no atomics, one order, the same bits every time.
// An edge with a non-finite end contributes nothing to either end (its vertex is NaN in the forward; its incoming gradient is not read).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define RA_MCG_HD __host__ __device__ __forceinline__
#else
#define RA_MCG_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr int MCG_MAX_C = 64;       // attribute channels per grid point at most

struct McgEdge {
    float d, t;
    float omt;      // 1 - t: the weight of the p end
    float tm1;      // t - 1
};

RA_MCG_HD bool mcg_finite(float x) { return x - x == 0.0f; }

// the forward's test: the two ends lie on two sides of iso
RA_MCG_HD bool mcg_crossed(float a, float b, float iso) { return (a < iso) != (b < iso); }

RA_MCG_HD unsigned mcg_popc3(unsigned m) { return (m & 1u) + ((m >> 1) & 1u) + ((m >> 2) & 1u); }

// the vertex of the edge along `axis` among those its owner carries
RA_MCG_HD unsigned mcg_slot(unsigned mask, int axis) { return mcg_popc3(mask & ((1u << axis) - 1u)); }

// false: the edge contributes nothing (a non-finite end)
RA_MCG_HD bool mcg_edge(float a, float b, float iso, McgEdge& e) {
    e.d = b - a;
    const float num = iso - a;
    e.t = num / e.d;
    e.omt = 1.0f - e.t;
    e.tm1 = e.t - 1.0f;
    return mcg_finite(a) && mcg_finite(b);
}

RA_MCG_HD float mcg_attr(const McgEdge& e, float Ap, float Aq) {
    const float l = e.omt * Ap, r = e.t * Aq;
    return l + r;
}

// one channel's term of gt
RA_MCG_HD float mcg_gt_add(float gt, float dattr, float Ap, float Aq) {
    const float diff = Aq - Ap;
    const float prod = dattr * diff;
    return gt + prod;
}

RA_MCG_HD float mcg_s(const McgEdge& e, float gt) { return gt / e.d; }
RA_MCG_HD float mcg_ca(const McgEdge& e, float s) { return e.tm1 * s; }
RA_MCG_HD float mcg_cb(const McgEdge& e, float s) { const float ts = e.t * s; return -ts; }
RA_MCG_HD float mcg_dAp(const McgEdge& e, float dattr) { return e.omt * dattr; }
RA_MCG_HD float mcg_dAq(const McgEdge& e, float dattr) { return e.t * dattr; }

"""Brute-force closest point on a triangle mesh in numpy, generic in the dtype: in float64 it is the truth of the mesh-distance tests, in
float32 the restatement whose own error sets their tolerance.  N points x F faces, Ericson's region method
(Real-Time Collision Detection 5.1.5) with every division guarded; where no region claims a point (a collinear face) the face acts as
its three edges, and the face region's answer is kept only where it is not farther than the nearest edge point.  The lowest face index wins among equal distances (np.argmin)."""
import numpy as np


def _dot(a, b):
    return (a * b).sum(-1)


def _ratio(num, den):
    """num / den clamped to [0, 1]; 0 where the denominator is not positive"""
    ok = den > 0
    return np.where(ok, np.clip(num / np.where(ok, den, 1), 0, 1), 0).astype(num.dtype)


def closest_on_triangles(p, a, b, c):
    """p, a, b, c broadcastable (..., 3) of one dtype -> d2 (...), closest (..., 3), bary (..., 3) per (point, triangle) pair"""
    dt = p.dtype
    one, zero = dt.type(1), dt.type(0)
    ab, ac, bc = b - a, c - a, c - b
    ap, bp, cp = p - a, p - b, p - c
    ab, ac, bc = np.broadcast_to(ab, ap.shape), np.broadcast_to(ac, ap.shape), np.broadcast_to(bc, ap.shape)
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    # every region's (v, w); the first whose condition holds is taken
    t_ab, t_ac, t_bc = _ratio(d1, d1 - d3), _ratio(d2, d2 - d6), _ratio(e43, e43 + e56)
    inside = (va > 0) & (vb > 0) & (vc > 0)
    s = np.where(inside, (va + vb) + vc, one)
    vi, wi = np.minimum(vb / s, one), np.minimum(vc / s, one)
    # the fall-back: the nearest of the three edges
    s_ab, s_ac, s_bc = _ratio(d1, _dot(ab, ab)), _ratio(d2, _dot(ac, ac)), _ratio(_dot(bc, bp), _dot(bc, bc))
    q1, q2, q3 = a + s_ab[..., None] * ab, a + s_ac[..., None] * ac, b + s_bc[..., None] * bc
    e1, e2, e3 = _dot(p - q1, p - q1), _dot(p - q2, p - q2), _dot(p - q3, p - q3)
    f1 = (e1 <= e2) & (e1 <= e3)
    f2 = ~f1 & (e2 <= e3)
    fu = np.where(f1, one - s_ab, np.where(f2, one - s_ac, zero))
    fv = np.where(f1, s_ab, np.where(f2, zero, one - s_bc))
    fw = np.where(f1, zero, np.where(f2, s_ac, s_bc))
    # an edge region needs an edge of some length: with a == b Ericson's condition holds trivially (d1 = d3 = vc = 0)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0) & (d1 - d3 > 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0) & (d2 - d6 > 0), (va <= 0) & (e43 >= 0) & (e56 >= 0) & (e43 + e56 > 0), inside]
    zeros, ones = np.zeros_like(d1), np.ones_like(d1)
    us = [ones, zeros, one - t_ab, zeros, one - t_ac, zeros, (one - vi) - wi]
    vs = [zeros, ones, t_ab, zeros, zeros, one - t_bc, vi]
    ws = [zeros, zeros, zeros, ones, t_ac, t_bc, wi]
    u, v, w = np.select(conds, us, fu), np.select(conds, vs, fv), np.select(conds, ws, fw)
    region = np.select(conds, list(range(7)), 7)
    # the closest point as each region forms it: a vertex itself, a + t e on an edge, a + v ab + w ac inside
    q = a + v[..., None] * ab + w[..., None] * ac
    q = np.where((region == 0)[..., None], a, q)
    q = np.where((region == 1)[..., None], b, q)
    q = np.where((region == 3)[..., None], c, q)
    q = np.where((region == 5)[..., None], b + w[..., None] * bc, q)
    fq = np.where(f1[..., None], q1, np.where(f2[..., None], q2, q3))
    q = np.where((region == 7)[..., None], fq, q).astype(dt)
    d = p - q
    dd = _dot(d, d)
    # the face's own answer must also beat the three edges: on a sliver, and far away, "all areas positive" is rounding noise
    worse = (region == 6) & ~(dd <= np.minimum(np.minimum(e1, e2), e3))
    q = np.where(worse[..., None], fq, q).astype(dt)
    u, v, w = np.where(worse, fu, u), np.where(worse, fv, v), np.where(worse, fw, w)
    d = p - q
    return _dot(d, d), q, np.stack([u, v, w], -1).astype(dt)


def closest_point(points, verts, faces, dtype=np.float64, chunk=512):
    """points (N,3), verts (V,3), faces (F,3) -> d2 (N,), closest (N,3), face (N,) int64, bary (N,3), all arithmetic in `dtype`.
    Faces with a non-finite vertex are never the answer; a point with a non-finite coordinate gets NaN and face -1; without a finite
    face every point gets d2 = +inf and face -1."""
    points, verts = np.asarray(points, dtype=dtype).reshape(-1, 3), np.asarray(verts, dtype=dtype)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    tri = verts[faces]                                                   # (F,3,3)
    keep = np.isfinite(tri).all((1, 2))
    ids = np.nonzero(keep)[0]
    tri = tri[keep]
    n = points.shape[0]
    d2 = np.full(n, np.inf, dtype=dtype)
    closest, bary = np.full((n, 3), np.nan, dtype=dtype), np.full((n, 3), np.nan, dtype=dtype)
    face = np.full(n, -1, dtype=np.int64)
    fin = np.isfinite(points).all(1)
    d2[~fin] = np.nan
    if len(ids):
        for i0 in range(0, n, chunk):
            sel = np.nonzero(fin[i0:i0 + chunk])[0] + i0
            if not len(sel):
                continue
            dd, q, br = closest_on_triangles(points[sel, None], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
            k = np.argmin(dd, 1)
            r = np.arange(len(sel))
            d2[sel], closest[sel], bary[sel], face[sel] = dd[r, k], q[r, k], br[r, k], ids[k]
    return d2, closest, face, bary


def distance_to_face(points, verts, faces, face_ids):
    """float64 distance (not squared) of every point to ONE given face each: the check of a returned face id"""
    points, verts = np.asarray(points, dtype=np.float64).reshape(-1, 3), np.asarray(verts, dtype=np.float64)
    tri = verts[np.asarray(faces, dtype=np.int64)[np.asarray(face_ids, dtype=np.int64)]]
    return np.sqrt(closest_on_triangles(points, tri[:, 0], tri[:, 1], tri[:, 2])[0])

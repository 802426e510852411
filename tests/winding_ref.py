"""References of the winding-number tests, in numpy, and the meshes and points they share.

    winding_number(points, verts, faces, dtype)   the reference's formula (lib/utils/mesh_utils.py:614-680) with its eps: unit vectors,
                                                  sign of cross(u1 - u0, u2 - u1) . u2, L'Huilier's product of four half-angle tangents
                                                  over 2 asin(l / 2), 4 atan(sqrt(|T| + 1e-10)).  In float64 it is the truth of the tests.
    winding_number_kernel32(points, verts, faces) the float32 restatement of the kernel's named operations (csrc/ra_winding_tri.hpp: the
                                                  half-angle form, the Cephes arctangent), summed in float64 in chunks: its own error
                                                  against the truth sets the tolerance of the parity tests (the 10 x float32 rule)
    winding_shift / winding_distance / remesh     the shift's three lines and the remesh, composed from mesh_distance_ref and
                                                  mesh_extract_ref in float64

A face with a non-finite vertex is dropped, as ra_mesh_create drops it.  A point with a non-finite coordinate and a point equal to a
vertex come out NaN of both functions by their arithmetic alone.
"""
import functools

import numpy as np
import torch

import mesh_distance_ref as M
import mesh_extract_ref as X
from relightableavatar_amd import synthetic

EPS = 1e-10
CHUNK = 1024                                      # the kernel's chunk (ra_winding_tile(1)): the restatement sums the same way
MESHES = ('hull', 'opened', 'two', 'far', 'degenerate', 'flipped', 'single')
SETS = ('near', 'grid')
FAR_OFFSET = np.float32([60, -80, 0])
GRID = dict(voxel=0.04, pad=0.05, shape=(20, 18, 26))
THRESHOLDS = (0.45, 0.75)


# ------------------------------------------------------------------------------------------------ meshes and points
@functools.lru_cache(None)
def hull(n_verts=301):
    """the convex hull of the synthetic body's template vertices (598 faces at 301 vertices), wound outwards"""
    b = synthetic.make_body(0, posed=False, n_verts=n_verts)
    tv = b.tverts[0].numpy()
    return tv, synthetic._template_faces(tv.astype(np.float64) / (0.4 * np.array([0.8, 0.7, 1.1])))


@functools.lru_cache(None)
def mesh_case(name):
    v, f = hull()
    if name == 'hull':
        return v, f
    if name == 'opened':                       # a hole at the top: every face that touches the top vertex or one of its neighbours is gone
        top = int(np.argmax(v[:, 2]))
        ring = np.unique(f[(f == top).any(1)])
        return v, f[~np.isin(f, ring).any(1)]
    if name == 'two':                          # two copies 5 m apart
        return np.concatenate([v, v + np.float32([5, 0, 0])]), np.concatenate([f, f + len(v)])
    if name == 'far':                          # 100 m from the origin
        return v + FAR_OFFSET, f
    if name == 'degenerate':                   # plus a collinear face and a face of three equal vertices, both outside the hull
        a, b = np.float32([0.5, 0.0, 0.0]), np.float32([0.6, 0.05, 0.02])
        extra = np.stack([a, b, a + np.float32(2) * (b - a), np.float32([0.0, 0.5, 0.3])])
        n = len(v)
        return np.concatenate([v, extra]), np.concatenate([f, [[n, n + 1, n + 2], [n + 3, n + 3, n + 3]]])
    if name == 'flipped':                      # one face wound the other way
        g = f.copy()
        g[100] = g[100, ::-1]
        return v, g
    if name == 'single':                       # one triangle
        return v, f[:1].copy()
    raise KeyError(name)


def grid_points(v):
    """a voxel grid that covers the box of v widened by the pad: float32 arange per axis, the last point at or past the box"""
    lo, hi = v.min(0) - np.float32(GRID['pad']), v.max(0) + np.float32(GRID['pad'])
    vs = GRID['voxel']
    ax = [np.arange(float(lo[k]), float(hi[k]) + vs, vs, dtype=np.float32) for k in range(3)]
    return np.stack(np.meshgrid(*ax, indexing='ij'), -1)


@functools.lru_cache(None)
def point_sets(name):
    """near: 1e-4, 1e-2 and 0.3 off the centroids of every 7th face on both sides, points in those faces' planes outside them, one
    point 1 km away.  grid: the 20 x 18 x 26 grid of voxel 0.04 around the hull's box + 0.05 (moved with the mesh that is 100 m off)."""
    v, f = mesh_case(name)
    v64 = v.astype(np.float64)
    tri = v64[f[::7]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    cen = tri.mean(1)
    near = [cen + s * nrm for s in (1e-4, -1e-4, 1e-2, -1e-2, 0.3, -0.3)]
    near += [cen + 3.0 * (tri[:, 0] - cen), cen - 2.0 * (tri[:, 1] - cen)]              # in the plane, outside the triangle
    near += [v64.mean(0, keepdims=True) + [[600.0, 800.0, 0.0]]]
    g = grid_points(hull()[0])
    assert g.shape[:3] == GRID['shape'], g.shape
    g = g.reshape(-1, 3) + (FAR_OFFSET if name == 'far' else np.float32(0))
    return {'near': np.concatenate(near).astype(np.float32), 'grid': np.ascontiguousarray(g.astype(np.float32))}


def checksum(name, group):
    """what the golden stores of its inputs: they are regenerated by seed"""
    v, f = mesh_case(name)
    p = point_sets(name)[group]
    return np.array([v.astype(np.float64).sum(), float(f.sum()), p.astype(np.float64).sum(), len(f), len(p)])


# ------------------------------------------------------------------------------------------------ the reference's formula
def _kept(verts, faces, dtype):
    tri = np.asarray(verts, dtype=dtype)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    return tri[np.isfinite(tri).all((1, 2))]


def winding_number(points, verts, faces, dtype=np.float64, chunk=256):
    """torch on the CPU, in the reference's order of operations: where a determinant is zero up to rounding (a collinear face, a point
    in a face's plane) its sign, and with it the sign of the eps term, is then the reference's too"""
    tdt = {np.float64: torch.float64, np.float32: torch.float32}[dtype]
    points = torch.from_numpy(np.asarray(points, dtype=dtype).reshape(-1, 3))
    tri = torch.from_numpy(_kept(verts, faces, dtype))
    out = torch.zeros(len(points), dtype=tdt)
    for i in range(0, len(points), chunk):
        u = tri[None] - points[i:i + chunk, None, None, :]                     # (n, F, 3 corners, 3)
        u = u / u.norm(dim=-1, keepdim=True)
        u0, u1, u2 = u[:, :, 0], u[:, :, 1], u[:, :, 2]
        e0, e1, e2 = u1 - u0, u2 - u1, u0 - u2
        sign = (torch.linalg.cross(e0, e1) * u2).sum(dim=-1).sign()
        l = 2 * (torch.stack([e0.norm(dim=-1), e1.norm(dim=-1), e2.norm(dim=-1)], dim=-1) / 2).arcsin()
        s = l.sum(dim=-1) / 2
        t = (s / 2).tan() * ((s - l[..., 0]) / 2).tan() * ((s - l[..., 1]) / 2).tan() * ((s - l[..., 2]) / 2).tan()
        solid = 4 * (t.abs() + EPS).sqrt().arctan()
        out[i:i + chunk] = (solid * sign).sum(dim=-1) / (4 * torch.pi)
    return out.numpy()


# ------------------------------------------------------------------------------------------------ the kernel's operations, in float32
F32 = np.float32


def _fma32(a, b, c):
    """m_fma: the product of two float32 is exact in float64, so this is one rounding (two in the rare case where the float64 sum
    falls on a float32 tie)"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def _dot32(a, b):
    return _fma32(a[..., 2], b[..., 2], _fma32(a[..., 0], b[..., 0], a[..., 1] * b[..., 1]))          # m_dot


def atan32(x):
    """w_atan: Cephes' reduction and polynomial, selects instead of branches"""
    big, mid = x > F32(2.414213562373095), x > F32(0.4142135623730950)
    num = np.where(big, F32(-1), np.where(mid, x - F32(1), x))
    den = np.where(big, x, np.where(mid, x + F32(1), F32(1)))
    y0 = np.where(big, F32(1.5707963267948966), np.where(mid, F32(0.7853981633974483), F32(0)))
    r = (num / den).astype(F32)
    z = r * r
    q = _fma32(F32(8.05374449538e-2), z, F32(-1.38776856032e-1))
    q = _fma32(q, z, F32(1.99777106478e-1))
    q = _fma32(q, z, F32(-3.33329491539e-1))
    return (y0 + _fma32(q * z, r, r)).astype(F32)


def solid_angle32(p, a, b, c):
    """winding_tri on float32 arrays that broadcast against each other: the signed solid angle, float32"""
    d0, d1, d2, ab, bc = a - p, b - p, c - p, b - a, c - b
    q0, q1, q2 = _dot32(d0, d0), _dot32(d1, d1), _dot32(d2, d2)
    i0, i1, i2 = F32(1) / np.sqrt(q0), F32(1) / np.sqrt(q1), F32(1) / np.sqrt(q2)
    n = np.stack([_fma32(ab[..., 1], bc[..., 2], -(ab[..., 2] * bc[..., 1])), _fma32(ab[..., 2], bc[..., 0], -(ab[..., 0] * bc[..., 2])),
                  _fma32(ab[..., 0], bc[..., 1], -(ab[..., 1] * bc[..., 0]))], -1)
    n = np.broadcast_to(n, d2.shape)
    e = np.where((q2 < np.minimum(q0, q1))[..., None], d2, np.where((q1 < q0)[..., None], d1, d0))          # the nearest vertex
    det = (_dot32(n, e) * i2) * (i0 * i1)
    den = (F32(1) + _dot32(d0, d1) * (i0 * i1)) + (_dot32(d1, d2) * (i1 * i2) + _dot32(d2, d0) * (i2 * i0))
    ad, h = np.abs(det), np.sqrt(_fma32(det, det, den * den))
    front = den >= 0
    t = np.where(front, ad, h - den) / np.where(front, h + den, ad)
    omega = F32(4) * atan32(np.sqrt(_fma32(t, t, F32(EPS))))
    assert omega.dtype == np.float32 and det.dtype == np.float32 and den.dtype == np.float32 and t.dtype == np.float32
    return np.where(det == 0, F32(0), np.copysign(omega, det))


def winding_number_kernel32(points, verts, faces, chunk=256):
    points = np.asarray(points, dtype=F32).reshape(-1, 3)
    tri = _kept(verts, faces, F32)
    out = np.zeros(len(points), dtype=np.float64)
    with np.errstate(all='ignore'):
        for i in range(0, len(points), chunk):
            p = points[i:i + chunk, None, :]
            for k in range(0, len(tri), CHUNK):
                t = tri[None, k:k + CHUNK]
                out[i:i + chunk] += solid_angle32(p, t[:, :, 0], t[:, :, 1], t[:, :, 2]).astype(np.float64).sum(-1)
    return (out * (1 / (4 * np.pi))).astype(F32)


# ------------------------------------------------------------------------------------------------ the shift and the remesh
def winding_shift(w, level_set=0.5, winding_th=0.45):
    """((w - level_set) * 2).clip(-1, 1), then -1 below -1 + th and +1 above 1 - th, both strict; in w's dtype"""
    s = np.clip((w - w.dtype.type(level_set)) * w.dtype.type(2), -1, 1)
    lo, hi = s < (-1 + winding_th), s > (+1 - winding_th)
    s = s.copy()
    s[lo], s[hi] = -1, +1
    return s


def shift_state(w, level_set=0.5, winding_th=0.45):
    """-1 / 0 / +1: clamped low, in between, clamped high"""
    s = np.clip((w - level_set) * 2, -1, 1)
    return np.where(s < (-1 + winding_th), -1, np.where(s > (1 - winding_th), 1, 0))


def threshold_margin(w, level_set=0.5, winding_th=0.45):
    """the distance of every winding number from the nearest value at which the shift changes its branch (the two strict thresholds)"""
    edges = np.array([level_set + (-1 + winding_th) / 2, level_set + (1 - winding_th) / 2])
    return np.abs(np.asarray(w, dtype=np.float64)[:, None] - edges[None]).min(1)


def winding_distance(points, verts, faces, winding_th=0.45, level_set=0.5):
    """float64: (signed distance, winding number, plain distance)"""
    w = winding_number(points, verts, faces)
    d = np.sqrt(M.closest_point(points, verts, faces, np.float64)[0])
    return winding_shift(w, level_set, winding_th) * d, w, d


def remesh_grid(verts, voxel_size, dist_th_tris):
    """the remesh's grid (X,Y,Z,3) float32: arange(lo, hi + voxel / 2, voxel) per axis over the box of the vertices widened by dist_th_tris"""
    v = np.asarray(verts, dtype=F32)
    lo, hi = v.min(0) - F32(dist_th_tris), v.max(0) + F32(dist_th_tris)
    ax = [np.arange(float(lo[k]), float(hi[k]) + voxel_size / 2, voxel_size, dtype=F32) for k in range(3)]
    return np.stack(np.meshgrid(*ax, indexing='ij'), -1)


def remesh(verts, faces, voxel_size, dist_th_verts, dist_th_tris, level_set=0.5, winding_th=0.75):
    """the remesh without a guide, composed in float64 (the grid in float32, as the library makes it): (verts, faces, cube float32)"""
    v = np.asarray(verts, dtype=F32)
    g = remesh_grid(v, voxel_size, dist_th_tris)
    p = g.reshape(-1, 3)
    d_vert = np.sqrt(((p[:, None, :].astype(np.float64) - v[None].astype(np.float64)) ** 2).sum(-1).min(1))
    cube = np.full(len(p), -10.0)
    k1 = np.nonzero(d_vert < dist_th_verts)[0]
    wd, _, d = winding_distance(p[k1], v, faces, winding_th, level_set)
    k2 = d < dist_th_tris
    cube[k1[k2]] = wd[k2]
    cube = cube.reshape(g.shape[:3]).astype(F32)
    mv, mf = X.largest_component(*X.marching_cubes(cube, 0.0))
    return (mv * F32(voxel_size) + g[0, 0, 0]).astype(F32), mf, cube

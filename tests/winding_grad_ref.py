"""References of the winding-gradient tests, in numpy.  Meshes and points are tests/winding_ref.py's.

    winding_grad(points, verts, faces)            the float64 oracle: the closed form of the gradient of the function the winding
                                                  kernels compute (the reference's value, its 1e-10 under the root included),
                                                      grad_p (sign Omega) = k(T) sum over the edges (x, y) of (x cross y) (|x| + |y|) / (|x| |y| (|x| |y| + x.y)),
                                                      k(T) = (1 + T) sqrt(T) / ((1 + T + eps) sqrt(T + eps)),  T = tan^2(Omega_0 / 4),
                                                  with T from the half-angle form tan(Omega_0 / 4) = |det| / (hypot(det, den) + den).
                                                  tests/test_oracle_winding_grad.py pins it to the reference's own float64 autograd.
    winding_grad_kernel32(points, verts, faces)   the float32 restatement of the kernel's named operations (csrc/ra_winding_grad_tri.hpp),
                                                  summed in float64 in chunks: its own error against the oracle sets the tolerance of the
                                                  parity tests (the 10 x float32 rule)
    winding_distance_grad(points, verts, faces, winding_th)    the oracle composed in float64: value and gradient of shift(w) * d

Both return (winding (n,), grad (n,3)).  Rules, in both: det == 0 gives value 0 and gradient 0; a point on the segment of an edge
(|x| |y| + x.y <= 0 as computed) gives a NaN gradient; a non-finite point and a point equal to a vertex give NaN by the arithmetic.
A face with a non-finite vertex is dropped.
"""
import numpy as np

import mesh_distance_ref as M
import winding_ref as W

EPS = W.EPS
F32 = np.float32
INV_4PI = 1 / (4 * np.pi)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def edge_gadget(offset=8.0):
    """(verts, faces, point): two faces that share the edge (o, o + 2 x) and the point in its middle.  Every difference is exact and
    |x| |y| + x.y is exactly 0 in float32 as in float64: the row whose gradient is NaN by the edge rule"""
    o = np.float32([offset] * 3)
    v = np.stack([o, o + np.float32([2, 0, 0]), o + np.float32([0, 2, 0]), o + np.float32([0, 0, 2])])
    return v, np.array([[0, 1, 2], [1, 0, 3]]), o + np.float32([1, 0, 0])


# ------------------------------------------------------------------------------------------------ the float64 oracle
def solid_angle_grad64(p, a, b, c):
    """float64 arrays that broadcast against each other -> (signed solid angle (...), its gradient in p (..., 3))"""
    d0, d1, d2, ab, bc, ca = a - p, b - p, c - p, b - a, c - b, a - c
    n0, n1, n2 = np.linalg.norm(d0, axis=-1), np.linalg.norm(d1, axis=-1), np.linalg.norm(d2, axis=-1)
    q = np.stack([n0, n1, n2], -1)
    e = np.take_along_axis(np.stack([d0, d1, d2], -2), np.argmin(q, -1)[..., None, None], -2)[..., 0, :]       # the nearest vertex
    det = (np.broadcast_to(_cross(ab, bc), e.shape) * e).sum(-1) / (n0 * n1 * n2)
    c01, c12, c20 = (d0 * d1).sum(-1) / (n0 * n1), (d1 * d2).sum(-1) / (n1 * n2), (d2 * d0).sum(-1) / (n2 * n0)
    den = 1 + c01 + c12 + c20
    ad, h = np.abs(det), np.hypot(det, den)
    front = den >= 0
    t = np.where(front, ad, h - den) / np.where(front, h + den, ad)
    T = t * t
    omega = 4 * np.arctan(np.sqrt(T + EPS))
    k = np.where(np.isfinite(T), (1 + T) * t / ((1 + T + EPS) * np.sqrt(T + EPS)), 1.0)
    total, off_edges = 0.0, True
    for x, y, nx, ny, edge in ((d0, d1, n0, n1, ab), (d1, d2, n1, n2, bc), (d2, d0, n2, n0, ca)):
        s = nx * ny + (x * y).sum(-1)
        off_edges = off_edges & (s > 0)
        total = total + _cross(x, np.broadcast_to(edge, x.shape)) * ((nx + ny) / (nx * ny * s))[..., None]      # x cross y = x cross (y - x)
    flat = det == 0
    grad = np.where(flat[..., None], 0.0, k[..., None] * total)
    return np.where(flat, 0.0, np.copysign(omega, det)), np.where(off_edges[..., None], grad, np.nan)


# ------------------------------------------------------------------------------------------------ the kernel's operations, in float32
def _cross32(a, b):
    """the header's x cross edge: m_fma(a1, b2, -m_mul(a2, b1)) per component"""
    return np.stack([W._fma32(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])), W._fma32(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                     W._fma32(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], -1)


def solid_angle_grad32(p, a, b, c):
    """winding_grad_tri on float32 arrays that broadcast against each other: (signed solid angle (...), gradient (..., 3)), float32"""
    d0, d1, d2, ab, bc, ca = a - p, b - p, c - p, b - a, c - b, a - c
    q0, q1, q2 = W._dot32(d0, d0), W._dot32(d1, d1), W._dot32(d2, d2)
    i0, i1, i2 = F32(1) / np.sqrt(q0), F32(1) / np.sqrt(q1), F32(1) / np.sqrt(q2)
    n = np.broadcast_to(_cross32(ab, bc), d2.shape)
    e = np.where((q2 < np.minimum(q0, q1))[..., None], d2, np.where((q1 < q0)[..., None], d1, d0))
    i01, i12, i20 = i0 * i1, i1 * i2, i2 * i0
    det = (W._dot32(n, e) * i2) * i01
    c01, c12, c20 = W._dot32(d0, d1) * i01, W._dot32(d1, d2) * i12, W._dot32(d2, d0) * i20
    den = (F32(1) + c01) + (c12 + c20)
    ad, h = np.abs(det), np.sqrt(W._fma32(det, det, den * den))
    front = den >= 0
    t = np.where(front, ad, h - den) / np.where(front, h + den, ad)
    root = np.sqrt(W._fma32(t, t, F32(EPS)))
    omega = F32(4) * W.atan32(root)
    e01, e12, e20 = F32(1) + c01, F32(1) + c12, F32(1) + c20
    w01, w12, w20 = ((i0 + i1) * i01) / e01, ((i1 + i2) * i12) / e12, ((i2 + i0) * i20) / e20
    x01, x12, x20 = _cross32(d0, np.broadcast_to(ab, d0.shape)), _cross32(d1, np.broadcast_to(bc, d1.shape)), _cross32(d2, np.broadcast_to(ca, d2.shape))
    k = np.where(root < np.inf, t / root, F32(1)).astype(F32)
    # m_dot(x01, x12, x20, w01, w12, w20) per component: fma(x20, w20, fma(x01, w01, x12 * w12))
    total = W._fma32(x20, w20[..., None], W._fma32(x01, w01[..., None], x12 * w12[..., None]))
    off_edges = (e01 > 0) & (e12 > 0) & (e20 > 0)
    flat = det == 0
    grad = np.where(flat[..., None], F32(0), k[..., None] * total)
    grad = np.where(off_edges[..., None], grad, F32(np.nan))
    value = np.where(flat, F32(0), np.copysign(omega, det))
    assert value.dtype == np.float32 and grad.dtype == np.float32 and k.dtype == np.float32 and total.dtype == np.float32
    return value, grad


# ------------------------------------------------------------------------------------------------ sums over a mesh
def _sweep(pair, points, verts, faces, dtype, rows):
    points = np.asarray(points, dtype=dtype).reshape(-1, 3)
    tri = W._kept(verts, faces, dtype)
    w, g = np.zeros(len(points)), np.zeros((len(points), 3))
    with np.errstate(all='ignore'):
        for i in range(0, len(points), rows):
            p = points[i:i + rows, None, :]
            for k in range(0, len(tri), W.CHUNK):                                # the kernel's chunks, each summed from 0 in float64
                t = tri[None, k:k + W.CHUNK]
                v, d = pair(p, t[:, :, 0], t[:, :, 1], t[:, :, 2])
                w[i:i + rows] += v.astype(np.float64).sum(-1)
                g[i:i + rows] += d.astype(np.float64).sum(-2)
    return w * INV_4PI, g * INV_4PI


def winding_grad(points, verts, faces, rows=128):
    """the float64 oracle: (winding (n,), grad (n,3)) float64"""
    return _sweep(solid_angle_grad64, points, verts, faces, np.float64, rows)


def winding_grad_kernel32(points, verts, faces, rows=128):
    """the float32 restatement: (winding (n,), grad (n,3)) float32, each rounded once from its float64 sum"""
    w, g = _sweep(solid_angle_grad32, points, verts, faces, F32, rows)
    return w.astype(F32), g.astype(F32)


# ------------------------------------------------------------------------------------------------ compositions, float64
def distance_grad(points, verts, faces):
    """(d (n,), grad (n,3)) float64: the distance to the mesh and (p - closest) / d, 0 where d == 0"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    d2, closest = M.closest_point(p, verts, faces, np.float64)[:2]
    d = np.sqrt(d2)
    with np.errstate(all='ignore'):
        return d, np.where((d > 0)[:, None], (p - closest) / d[:, None], 0.0)


def shift_slope(w, level_set=0.5, winding_th=0.45):
    """d shift / d w: 2 where the shift is neither clipped nor snapped, else 0"""
    return np.where(W.shift_state(w, level_set, winding_th) == 0, 2.0, 0.0)


def winding_distance_grad(points, verts, faces, winding_th=0.45, level_set=0.5, wg=None, dg=None):
    """(value (n,), grad (n,3), winding term of the gradient (n,3)) float64 of shift(w) * d; wg / dg: winding_grad / distance_grad of
    the same inputs, where the caller has them"""
    w, gw = wg if wg is not None else winding_grad(points, verts, faces)
    d, gd = dg if dg is not None else distance_grad(points, verts, faces)
    s = W.winding_shift(w, level_set, winding_th)
    term = (shift_slope(w, level_set, winding_th) * d)[:, None] * gw
    return s * d, term + s[:, None] * gd, term

"""ra_mesh_closest_backward in numpy: the float32 rule in the kernel's order — what the device must equal bit for
bit —, the same rule in float64 in closed form, and a float64 restatement of mesh_utils.point_cloud_fitting.

Row i: p the point, q / f / b the forward's closest point, face and barycentrics, g the upstream gradient of d2 (the SQUARED distance),
ga[C] the upstream gradient of C attribute channels interpolated at the closest point.  Live: 0 <= f < F and the face's three indices in
[0, V).  dpts = (2 g) (p - q); slot (i, k) belongs to vertex faces[f][k] and carries -(b_k dpts) for dverts and b_k ga for dattr; a
vertex's result is the wave sum (raster_ref._wave_sum) of its slots in ascending 3 i + k, +0 without a slot.  A dead row: dpts 0, no slot."""
import functools

import numpy as np

import mesh_distance_ref as M
from raster_ref import _wave_sum

F32 = np.float32


@functools.lru_cache(None)
def hull():
    """the 598-face hull of synthetic.make_body(0, posed=False, n_verts=301): (verts float32, faces), the body of the mesh-distance tests"""
    from relightableavatar_amd import synthetic
    tv = synthetic.make_body(0, posed=False, n_verts=301).tverts[0].numpy()
    return tv, synthetic._template_faces(tv.astype(np.float64) / (0.4 * np.array([0.8, 0.7, 1.1])))


@functools.lru_cache(None)
def generic_points(seed=3):
    """about 360 points of the hull in general position: off the centroids of every second face (outwards, with random offsets along
    the face that carry some past its edges), inside the body, and a little outwards of vertices with a random offset.  None sits on a
    vertex or on the midpoint of a shared edge, where the minimum over faces has a kink."""
    v, f = hull()
    v64 = v.astype(np.float64)
    rng = np.random.default_rng(seed)
    tri = v64[f[::2]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    size = np.linalg.norm(tri[:, 1] - tri[:, 0], axis=-1, keepdims=True)
    off = tri.mean(1) + rng.uniform(0.005, 0.05, (len(tri), 1)) * nrm + 0.35 * size * rng.standard_normal((len(tri), 3))
    inside = v64.mean(0) + 0.3 * (v64[rng.choice(len(v64), 30, replace=False)] - v64.mean(0)) + 0.01 * rng.standard_normal((30, 3))
    pick = rng.choice(len(v64), 34, replace=False)
    out = v64[pick] - v64.mean(0)
    out /= np.linalg.norm(out, axis=-1, keepdims=True)
    around = v64[pick] + 0.02 * out + 0.002 * rng.standard_normal((34, 3))
    return np.concatenate([off, inside, around]).astype(np.float32)


def live_rows(face, faces, V):
    """(n,) bool, and the (n,3) vertex indices of every row's face (0 in the dead rows)"""
    face, faces = np.asarray(face, np.int64), np.asarray(faces, np.int64).reshape(-1, 3)
    ok = (face >= 0) & (face < len(faces))
    idx = faces[np.where(ok, face, 0)]
    ok = ok & ((idx >= 0) & (idx < V)).all(1)
    return ok, np.where(ok[:, None], idx, 0)


def _run_sums(vert, slot, terms, V):
    """terms (m, C) float32 of the slots (vert, slot) -> (V, C) float32: per vertex the wave sum of its terms in ascending slot"""
    out = np.zeros((V, terms.shape[1]), F32)
    order = np.lexsort((slot, vert))
    vert, terms = vert[order], terms[order]
    heads = np.flatnonzero(np.r_[True, vert[1:] != vert[:-1]]) if len(vert) else np.zeros(0, np.int64)
    ends = np.r_[heads[1:], len(vert)]
    for a, b in zip(heads, ends):
        out[vert[a]] = _wave_sum(terms[a:b])
    return out


def backward32(pts, closest, face, bary, faces, V, g_d2=None, g_attr=None):
    """the kernels' float32 operations in the kernels' order -> dict(dpts (n,3), dverts (V,3), dattr (V,C)); dpts and dverts without
    g_d2, dattr without g_attr are None"""
    p, q, b = (np.asarray(a, F32).reshape(-1, 3) for a in (pts, closest, bary))
    n = len(p)
    ok, idx = live_rows(face, faces, V)
    rows = np.flatnonzero(ok)
    vert = idx[rows].reshape(-1)                                     # slot order: 3 i + k ascending
    slot = (3 * rows[:, None] + np.arange(3)).reshape(-1)
    res = dict(dpts=None, dverts=None, dattr=None)
    with np.errstate(all='ignore'):
        if g_d2 is not None:
            g2 = F32(2) * np.asarray(g_d2, F32).reshape(-1)
            dpts = np.zeros((n, 3), F32)
            dpts[rows] = g2[rows, None] * (p[rows] - q[rows])
            res['dpts'] = dpts
            terms = -(b[rows][:, :, None] * dpts[rows][:, None, :])  # (m, 3 corners, 3 components)
            res['dverts'] = _run_sums(vert, slot, terms.reshape(3 * len(rows), 3).astype(F32), V)
        if g_attr is not None:
            ga = np.asarray(g_attr, F32).reshape(n, np.shape(g_attr)[-1])
            terms = b[rows][:, :, None] * ga[rows][:, None, :]
            res['dattr'] = _run_sums(vert, slot, terms.reshape(3 * len(rows), ga.shape[1]).astype(F32), V)
    return res


def forward_on_face(pts, verts, faces, face):
    """float64 closest point and barycentrics of every point in ONE given face each (rows with a face outside [0, F): NaN)"""
    p, v = np.asarray(pts, np.float64).reshape(-1, 3), np.asarray(verts, np.float64)
    faces, face = np.asarray(faces, np.int64).reshape(-1, 3), np.asarray(face, np.int64)
    ok = (face >= 0) & (face < len(faces))
    tri = v[faces[np.where(ok, face, 0)]]
    with np.errstate(all='ignore'):
        d2, q, b = M.closest_on_triangles(p, tri[:, 0], tri[:, 1], tri[:, 2])
    return np.where(ok, d2, np.nan), np.where(ok[:, None], q, np.nan), np.where(ok[:, None], b, np.nan)


def flat_faces(verts, faces):
    """(F,) bool: faces of no area — twice the area at most 2^-16 of the longest edge's square, far below any face a mesh is made of
    and far above the rounding of float32 coordinates.  On such a face the barycentrics of a point are not unique (a point of a
    collinear face a, b, c lies on ab AND on ac), so no reference can say how a row's gradient is shared among its three vertices."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all='ignore'):
        twice = np.linalg.norm(np.cross(b - a, c - a), axis=-1)
        longest = np.maximum(np.maximum(((b - a) ** 2).sum(-1), ((c - a) ** 2).sum(-1)), ((c - b) ** 2).sum(-1))
        return ~(twice > 2.0 ** -16 * longest)


def backward64(pts, verts, faces, face, g_d2=None, g_attr=None, closest=None, bary=None, flat_bary=None):
    """the closed form in float64 at the given faces: d(d2)/dp = 2 (p - q), d(d2)/dv_k = -2 b_k (p - q), dattr_k = b_k ga, summed per
    vertex.  closest / bary: given (e.g. the float32 forward's own), or the float64 closest point in that face.  flat_bary (n,3): the
    barycentrics to take on the rows whose face has no area (flat_faces), where float64 has no unique ones of its own: the caller's
    returned barycentrics, with closest = sum b v in float64."""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    V = len(verts)
    if closest is None or bary is None:
        _, closest, bary = forward_on_face(p, verts, faces, face)
        if flat_bary is not None and len(p):
            ok, idx = live_rows(face, faces, V)
            flat = ok & flat_faces(verts, faces)[np.where(ok, np.asarray(face, np.int64), 0)]
            fb = np.asarray(flat_bary, np.float64)
            bary = np.where(flat[:, None], fb, bary)
            closest = np.where(flat[:, None], (fb[:, :, None] * np.asarray(verts, np.float64)[idx]).sum(1), closest)
    q, b = np.asarray(closest, np.float64), np.asarray(bary, np.float64)
    ok, idx = live_rows(face, faces, V)
    rows = np.flatnonzero(ok)
    res = dict(dpts=None, dverts=None, dattr=None)
    if g_d2 is not None:
        g = np.asarray(g_d2, np.float64).reshape(-1)
        dpts = np.zeros_like(p)
        dpts[rows] = 2 * g[rows, None] * (p[rows] - q[rows])
        dverts = np.zeros((V, 3))
        for k in range(3):
            np.add.at(dverts, idx[rows, k], -b[rows, k, None] * dpts[rows])
        res['dpts'], res['dverts'] = dpts, dverts
    if g_attr is not None:
        ga = np.asarray(g_attr, np.float64).reshape(len(p), np.shape(g_attr)[-1])
        dattr = np.zeros((V, ga.shape[1]))
        for k in range(3):
            np.add.at(dattr, idx[rows, k], b[rows, k, None] * ga[rows])
        res['dattr'] = dattr
    return res


def weighted_d2(pts, verts, faces, g):
    """L = sum_i g_i d2_i in float64 from the exhaustive closest point: what the central differences differentiate"""
    return float((np.asarray(g, np.float64) * M.closest_point(pts, verts, faces, np.float64)[0]).sum())


def regions(bary):
    """per row 0 face, 1 edge, 2 vertex: the number of barycentrics that are exactly 0"""
    return (np.asarray(bary) == 0).sum(1)


# ---------------------------------------------------------------------------------------------- run-sum cases
RUN_COUNTS = (0, 1, 63, 64, 65, 129, 257)


def run_case(C, seed=5):
    """Synthetic rows that give vertex t exactly RUN_COUNTS[t] slots: face t = (t, D1, D2) with two collecting vertices D1, D2 behind
    the targets, RUN_COUNTS[t] rows per face in a shuffled order, and among them dead rows — face -1, face F, and a face with a vertex
    index outside [0, V) — whose values are NaN so that a leak shows.  The forward's outputs are made up (any stored values are legal
    inputs); the barycentrics do not sum to 1."""
    rng = np.random.default_rng(seed + C)
    T = len(RUN_COUNTS)
    V = T + 2
    faces = np.array([[t, T, T + 1] for t in range(T)] + [[0, V, 1]], np.int32)       # the last face is out of range: its rows are dead
    face = np.concatenate([np.full(c, t) for t, c in enumerate(RUN_COUNTS)])
    rng.shuffle(face)
    dead = np.array([-1, len(faces), len(faces) - 1, -7])
    at = np.sort(rng.choice(np.arange(1, len(face)), len(dead), replace=False))
    face = np.insert(face, at, dead).astype(np.int32)
    n = len(face)
    pts, closest = rng.standard_normal((n, 3)).astype(F32), rng.standard_normal((n, 3)).astype(F32)
    bary = rng.uniform(0, 1, (n, 3)).astype(F32)
    g, ga = rng.standard_normal(n).astype(F32), rng.standard_normal((n, C)).astype(F32)
    is_dead = ~live_rows(face, faces, V)[0]
    pts[is_dead], g[is_dead] = np.nan, np.nan
    ga[is_dead] = np.nan
    return dict(faces=faces, V=V, face=face, pts=pts, closest=closest, bary=bary, g=g, ga=ga, dead=is_dead)


# ---------------------------------------------------------------------------------------------- the fitting loop
def fit(v0, faces, tar, lam=29, opt_iter=20, lr=1e-3, chunks=None, dtype=np.float64):
    """mesh_utils.point_cloud_fitting from the definitions (a sparse LU solve, the exhaustive closest point, the closed-form gradient,
    AdamUniform's definition), all in `dtype`: float64 is the truth, float32 the same algorithm in the format of the inputs, whose
    error is the yardstick of the 10 x rule -> (verts, losses).  chunks: per iteration the rows of tar the loss sees (None: all)."""
    from scipy.sparse.linalg import splu

    import fit_ref as R
    v0 = np.asarray(v0, F32).astype(dtype)                            # the device's inputs
    tar = np.asarray(tar, F32).astype(dtype)
    A = R.truth_matrix(faces, len(v0), lam).astype(dtype)
    lu = splu(A)
    p = A @ v0
    g1, g2 = np.zeros_like(p), dtype(0)
    losses = []
    for it in range(1, opt_iter + 1):
        v = lu.solve(p)
        q = tar if chunks is None else tar[chunks[it - 1]]
        d2, closest, face, bary = M.closest_point(q, v, faces, dtype)
        losses.append(d2.mean())
        g = np.full(len(q), 1.0 / len(q), dtype)
        dv = backward32(q, closest, face, bary, faces, len(v), g)['dverts'] if dtype == np.float32 else \
            backward64(q, v, faces, face, g_d2=g, closest=closest, bary=bary)['dverts']
        p, g1, g2 = R.adam_literal(p, lu.solve(dv), g1, g2, it, lr)
    return lu.solve(p), np.asarray(losses)


def mean_d2(pts, verts, faces):
    """the mean squared distance of the points to the mesh in float64: the fitting's loss, evaluated apart from any loop"""
    return float(M.closest_point(np.asarray(pts, np.float64), np.asarray(verts, np.float64), faces, np.float64)[0].mean())

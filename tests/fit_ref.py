"""The project's own restatement of the mesh-fitting kernels (include/relightableavatar.h: ra_topo_diffuse_apply / _solve,
ra_mesh_normals, ra_icp_residual, ra_adam_uniform_step; csrc/ra_fit_rules.hpp), in numpy, in the kernels' operation order.

Written from the rules, not from any program text:
  - M = I + lambda L, L = D - A the combinatorial Laplacian of the unique edges; per (vertex, channel)
        t = deg x,  u = t - s,  w = lambda u,  M x = x + w,     s the ascending sum of the neighbours OTHER than the vertex itself;
  - the solve is Jacobi-preconditioned conjugate gradients with float64 state, one system per channel; a sum over a channel is a
    tree sum inside every tile of `tile` vertices (a[t] + a[t + s] for s = tile / 2 ... 1); the tiles' sums are then added by `tile`
    threads, thread t the tiles t, t + tile, ... in ascending order from 0, and the same tree over the threads;
  - normals, the ICP residual and AdamUniform as ra_fit_rules.hpp names them.
`state` is the dtype of the arithmetic: float64 is the kernels', float32 exists to measure what float32 arithmetic would cost.
`truth_*` are the plain float64 definitions (scipy.sparse, spsolve) the restatement itself is tested against.
"""
import numpy as np

TILE = 256      # ra_fit_tile(0) and (1); the GPU tests pass the library's own value


# ---------------------------------------------------------------------------------------------- the operator
def neighbours(topo):
    """(start (V+1,), nbr) of a tests/topology_ref.py topology without the entries that name the vertex itself"""
    start, nbr = topo['nbr_start'], topo['nbr']
    V = len(start) - 1
    owner = np.repeat(np.arange(V), np.diff(start))
    keep = nbr != owner
    deg = np.bincount(owner[keep], minlength=V)
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), nbr[keep]


def nbr_sum(x, nb):
    """the ascending neighbour sum of every row of x (V,C), from 0"""
    start, nbr = nb
    deg = np.diff(start)
    s = np.zeros_like(x)
    for k in range(int(deg.max()) if len(deg) else 0):
        has = deg > k
        s[has] = s[has] + x[nbr[start[:-1][has] + k]]
    return s


def diffuse(x, nb, lam):
    deg = np.diff(nb[0]).astype(x.dtype)[:, None]
    t = deg * x
    u = t - nbr_sum(x, nb)
    w = x.dtype.type(lam) * u
    return x + w


def apply(x32, topo, lam, state=np.float64):
    """fl32(M x) of float32 rows (V,C)"""
    x = np.asarray(x32, dtype=np.float32).astype(state)
    x = x.reshape(len(x), -1)
    return diffuse(x, neighbours(topo), np.float32(lam)).astype(np.float32)


def truth_matrix(faces, n_verts, lam):
    """M as scipy.sparse CSC in float64, from the definition: A[i, j] = 1 for every unique undirected edge i != j of the faces"""
    import scipy.sparse as sp
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b = f.reshape(-1), np.roll(f, -1, axis=1).reshape(-1)
    pairs = {(min(i, j), max(i, j)) for i, j in zip(a.tolist(), b.tolist()) if i != j}
    ij = np.asarray(sorted(pairs), dtype=np.int64).reshape(-1, 2)
    A = sp.coo_matrix((np.ones(len(ij)), (ij[:, 0], ij[:, 1])), shape=(n_verts, n_verts))
    A = (A + A.T).tocsc()
    D = sp.diags(np.asarray(A.sum(1)).reshape(-1))
    return (sp.identity(n_verts) + float(lam) * (D - A)).tocsc()


def truth_solve(faces, n_verts, lam, b, dtype=np.float64):
    from scipy.sparse.linalg import spsolve
    M = truth_matrix(faces, n_verts, lam).astype(dtype)
    b = np.asarray(b, dtype=dtype).reshape(n_verts, -1)
    return np.stack([spsolve(M, b[:, k]) for k in range(b.shape[1])], axis=1).astype(dtype)


# ---------------------------------------------------------------------------------------------- fixed-order sums
def tile_sum(v, tile=TILE):
    """the sum of a vector as the kernels form it"""
    v = np.asarray(v)
    n_tiles = (len(v) + tile - 1) // tile
    a = np.zeros(n_tiles * tile, dtype=v.dtype)
    a[:len(v)] = v
    a = a.reshape(n_tiles, tile)
    s = tile // 2
    while s > 0:
        a = a[:, :s] + a[:, s:2 * s]
        s //= 2
    # the second stage, one workgroup: thread t adds the partials t, t + tile, ... in ascending order from 0, then the same tree
    rows = (n_tiles + tile - 1) // tile
    part = np.zeros(max(rows, 1) * tile, dtype=v.dtype)
    part[:n_tiles] = a[:, 0]
    acc = np.zeros(tile, dtype=v.dtype)
    for row in part.reshape(-1, tile):
        acc = acc + row
    s = tile // 2
    while s > 0:
        acc = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0]


# ---------------------------------------------------------------------------------------------- the solve
STOP_NONE, STOP_CONVERGED, STOP_ZERO, STOP_NAN, STOP_BREAKDOWN = range(5)


def cg_channel(b32, nb, lam, x0_32=None, tol=1e-9, max_iter=256, tile=TILE, state=np.float64):
    """one channel: float32 b (V,), x0 -> (x float32 (V,), iters, stop, relres)"""
    f = state
    lam = f(np.float32(lam))
    b = np.asarray(b32, dtype=np.float32).astype(f)[:, None]
    x = np.zeros_like(b) if x0_32 is None else np.asarray(x0_32, dtype=np.float32).astype(f)[:, None]
    diag = f(1) + lam * np.diff(nb[0]).astype(f)[:, None]
    with np.errstate(all='ignore'):
        r = b - diffuse(x, nb, lam)
        z = r / diag
        p = z.copy()
        rz, rr, bb = tile_sum((r * z)[:, 0], tile), tile_sum((r * r)[:, 0], tile), tile_sum((b * b)[:, 0], tile)
        nan = np.full(len(b), np.nan, dtype=np.float32)
        if not (np.isfinite(rz) and np.isfinite(rr) and np.isfinite(bb)):
            return nan, 0, STOP_NAN, np.nan
        if bb == 0:
            return np.zeros(len(b), dtype=np.float32), 0, STOP_ZERO, 0.0
        relres = np.sqrt(rr) / np.sqrt(bb)
        if np.sqrt(rr) <= f(tol) * np.sqrt(bb):
            return x[:, 0].astype(np.float32), 0, STOP_CONVERGED, float(relres)
        beta, iters, stop = f(0), 0, STOP_NONE
        for _ in range(max_iter):
            bp = beta * p
            p = z + bp
            q = diffuse(p, nb, lam)
            pq = tile_sum((p * q)[:, 0], tile)
            if not pq > 0:
                stop = STOP_BREAKDOWN
                break
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * q
            z = r / diag
            rz_new, rr = tile_sum((r * z)[:, 0], tile), tile_sum((r * r)[:, 0], tile)
            iters += 1
            if not (np.isfinite(rz_new) and np.isfinite(rr)):
                return nan, iters, STOP_NAN, np.nan
            relres = np.sqrt(rr) / np.sqrt(bb)
            if np.sqrt(rr) <= f(tol) * np.sqrt(bb):
                stop = STOP_CONVERGED
                break
            beta = rz_new / rz
            rz = rz_new
    return x[:, 0].astype(np.float32), iters, stop, float(relres)


def solve(b32, topo, lam, x0_32=None, tol=1e-9, max_iter=256, tile=TILE, state=np.float64):
    """float32 rows (V,C) -> (x float32 (V,C), iters (C,), stop (C,), relres (C,))"""
    b = np.asarray(b32, dtype=np.float32)
    b = b.reshape(len(b), -1)
    x0 = None if x0_32 is None else np.asarray(x0_32, dtype=np.float32).reshape(b.shape)
    nb = neighbours(topo)
    cols = [cg_channel(b[:, k], nb, lam, None if x0 is None else x0[:, k], tol, max_iter, tile, state) for k in range(b.shape[1])]
    return (np.stack([c[0] for c in cols], axis=1), np.asarray([c[1] for c in cols]), np.asarray([c[2] for c in cols]),
            np.asarray([c[3] for c in cols], dtype=np.float64))


# ---------------------------------------------------------------------------------------------- normals
def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def normals(v32, faces, topo, state=np.float64):
    """float32 verts (V,3) -> face_normal (F,3), face_area (F,), vert_normal (V,3), all float32"""
    v = np.asarray(v32, dtype=np.float32).astype(state)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all='ignore'):
        n = _cross(b - a, c - b)
        fn = n / (np.sqrt(_dot(n, n)) + state(1e-8))[:, None]
        x = _cross(c - a, b - a)
        area = np.sqrt(_dot(x, x)) / state(2)
        start, out_he = topo['out_start'], topo['out_he']
        deg = np.diff(start)
        s = np.zeros_like(v)
        for k in range(int(deg.max()) if len(deg) else 0):
            has = deg > k
            s[has] = s[has] + n[out_he[start[:-1][has] + k] // 3]
        l = np.sqrt(_dot(s, s))
        vn = s / np.where(l > state(1e-6), l, state(1e-6))[:, None]
    return fn.astype(np.float32), area.astype(np.float32), vn.astype(np.float32)


def edge_length(v, e):
    v = np.asarray(v)
    d = v[e[:, 0]] - v[e[:, 1]]
    return np.sqrt((d * d).sum(-1))


# ---------------------------------------------------------------------------------------------- ICP residual
def icp_residual(p32, n0_32, n1_32, d2_32, closest32, face, dist_th, angle_th, tile=TILE):
    """the residual behind a closest-point answer (d2, closest, face as ra_mesh_closest gives them, float32 / int):
    -> sums (2,) float64, grad (n,3) float32, keep (n,) bool"""
    p, c = np.asarray(p32, dtype=np.float32), np.asarray(closest32, dtype=np.float32)
    n0, n1 = np.asarray(n0_32, dtype=np.float32).astype(np.float64), np.asarray(n1_32, dtype=np.float32).astype(np.float64)
    face = np.asarray(face, dtype=np.int64)
    th = np.float32(dist_th)
    th2 = th * th
    ok = (face >= 0) & (face < len(n1)) & np.isfinite(p).all(1)
    with np.errstate(all='ignore'):
        keep = ok & (np.asarray(d2_32, dtype=np.float32) < th2) & (_dot(n1[np.clip(face, 0, max(len(n1) - 1, 0))], n0) > np.float64(np.float32(angle_th)))
        delta = p.astype(np.float64) - c.astype(np.float64)
        sq = np.where(keep, _dot(delta, delta), 0.0)
    sums = np.asarray([tile_sum(sq, tile), tile_sum(keep.astype(np.float64), tile)]) if len(p) else np.zeros(2)
    grad = np.zeros((len(p), 3), dtype=np.float32)
    if sums[1] > 0:
        w = 2.0 / sums[1]
        grad[keep] = (w * delta[keep]).astype(np.float32)
    return sums, grad, keep


def truth_icp(p, n0, tv, tf, n1, dist_th, angle_th, dtype=np.float64):
    """from the definition in `dtype` (float64: the truth), with the exhaustive closest point of tests/mesh_distance_ref.py:
    loss, grad, keep, d2, dot"""
    import mesh_distance_ref as R
    p, n0, n1 = np.asarray(p, dtype=dtype), np.asarray(n0, dtype=dtype), np.asarray(n1, dtype=dtype)
    d2, closest, face, _ = R.closest_point(p, tv, tf, dtype)
    dot = (n1[face] * n0).sum(-1)
    keep = (d2 < dtype(dist_th) ** 2) & (dot > dtype(angle_th))
    delta = p - closest
    count = keep.sum()
    with np.errstate(all='ignore'):
        loss = dtype((delta[keep] ** 2).sum(-1).sum()) / dtype(count)
    grad = np.zeros_like(p)
    if count:
        grad[keep] = dtype(2.0) / dtype(count) * delta[keep]
    return loss, grad, keep, d2, dot


# ---------------------------------------------------------------------------------------------- AdamUniform
def fit_pow(b, t):
    p = np.float64(1)
    for _ in range(t):
        p = p * b
    return p


def adam_step(p32, g32, g1_32, g2_32, step, lr=0.1, betas=(0.9, 0.999)):
    """one step on float32 arrays -> (p, g1, g2) float32, g2 a float32 scalar"""
    lr, b1, b2 = (np.float64(np.float32(x)) for x in (lr, betas[0], betas[1]))
    p, g, g1 = (np.asarray(a, dtype=np.float32) for a in (p32, g32, g1_32))
    m = np.float64(np.abs(g).max())
    g1n = (b1 * g1.astype(np.float64) + (1.0 - b1) * g.astype(np.float64)).astype(np.float32)
    g2n = np.float32(b2 * np.float64(np.float32(g2_32)) + (1.0 - b2) * (m * m))
    c1, c2 = 1.0 - fit_pow(b1, step), 1.0 - fit_pow(b2, step)
    m1 = g1n.astype(np.float64) / c1
    m2 = np.float64(g2n) / c2
    den = 1e-8 + np.sqrt(m2)
    q = m1 / den
    return (p.astype(np.float64) - lr * q).astype(np.float32), g1n, g2n


def adam_literal(p, g, g1, g2, t, lr=0.1, b1=0.9, b2=0.999):
    """the definition, transcribed line by line in the dtype of p (float64: the truth): (p, g1, g2)"""
    f = p.dtype.type
    lr, b1, b2 = f(lr), f(b1), f(b2)
    g1 = b1 * g1 + (f(1) - b1) * g
    g2 = b2 * g2 + (f(1) - b2) * (g ** 2).max()
    m1 = g1 / (f(1) - b1 ** f(t))
    m2 = g2 / (f(1) - b2 ** f(t))
    return p - lr * m1 / (f(1e-8) + np.sqrt(m2)), g1, g2


# ---------------------------------------------------------------------------------------------- the fitting loop
# The learning rate of the fitting tests.  AdamUniform moves no coordinate by more than about lr per step (|m1| <= sqrt(m2) up to the
# bias corrections), and M^-1 does not amplify; the two sheets of fit_pair start 0.01 apart and approach each other, so with
# 20 steps x 2 meshes x lr = 0.008 < 0.01 they cannot pass through each other and the loss falls in every iteration.  The reference's
# default 3e-2 is for bodies a metre tall that are centimetres apart; on this fixture it overshoots in the first step.
FIT_LR = 2e-4
FIT_ITERS = 20


def fit_pair(seed=11, n=9, offset=0.01):
    """two jittered open n x n patches (tests/topology_ref.py: patch), the second a copy moved `offset` along +z with its own small
    jitter: float64 verts and the shared faces"""
    import topology_ref as T
    v0, f = T.patch(n, seed)
    v0 = v0.copy()
    v0[:, 2] *= 0.2          # a gently curved sheet: every normal stays within a few degrees of +z
    rng = np.random.default_rng(seed + 1)
    v1 = v0 + np.array([0.0, 0.0, offset]) + rng.uniform(-0.001, 0.001, v0.shape)
    return v0, v1, f


def boundary_rows(faces, n_verts, dilate=0):
    """the rows boundary_focus selects: the ends of every edge without exactly two half-edges, then `dilate` times 'set when a
    neighbour was set' (the adjacency has no diagonal)"""
    import topology_ref as T
    t = T.halfedge_build(faces, n_verts)
    vm = np.zeros(n_verts, dtype=bool)
    vm[t['edges'][t['edge_counts'] != 2].reshape(-1)] = True
    start, nbr = neighbours(t)
    for _ in range(dilate):
        vm = np.asarray([vm[nbr[start[k]:start[k + 1]]].any() for k in range(n_verts)])
    return np.flatnonzero(vm)


def fit(v0, f0, v1, f1, lam=29, opt_iter=20, lr=3e-2, sel0=None, sel1=None, dist_th=0.1, angle_th=np.cos(np.deg2rad(45.0)), margins=None,
        dtype=np.float64):
    """bidirectional_icp_fitting from the definitions (a sparse LU solve, exhaustive closest point, AdamUniform's definition), all in
    `dtype`: float64 is the truth, float32 the same algorithm in the format of the inputs, whose error is the yardstick of the 10 x
    rule -> (v0, v1, losses).  sel0 / sel1: the rows the loss sees (None: all).  margins: a list that receives, per iteration, the
    smallest relative distance of any row from either filter threshold."""
    from scipy.sparse.linalg import splu
    v0, v1 = np.asarray(v0, dtype=np.float32).astype(dtype), np.asarray(v1, dtype=np.float32).astype(dtype)      # the device's inputs
    A = [truth_matrix(f0, len(v0), lam).astype(dtype), truth_matrix(f1, len(v1), lam).astype(dtype)]
    M = [splu(A[0]), splu(A[1])]
    import topology_ref as T
    topo = [T.halfedge_build(f0, len(v0)), T.halfedge_build(f1, len(v1))]
    faces, sel = [f0, f1], [sel0, sel1]
    p = [A[0] @ v0, A[1] @ v1]
    g1, g2 = [np.zeros_like(p[0]), np.zeros_like(p[1])], [dtype(0), dtype(0)]
    losses = []
    for it in range(1, opt_iter + 1):
        v = [M[k].solve(p[k]) for k in range(2)]
        nrm = [normals64(v[k], faces[k], topo[k]) for k in range(2)]
        total, grads = 0.0, []
        for k in range(2):
            o = 1 - k
            rows = np.arange(len(v[k])) if sel[k] is None else np.asarray(sel[k])
            loss, g, keep, d2, dot = truth_icp(v[k][rows], nrm[k][2][rows], v[o], faces[o], nrm[o][0], dist_th, angle_th, dtype)
            if margins is not None:
                margins.append(min(np.abs(d2 / dist_th ** 2 - 1).min(), np.abs(dot / angle_th - 1).min(), 1.0 if keep.all() else 0.0))
            full = np.zeros_like(v[k])
            full[rows] = g
            grads.append(M[k].solve(full))
            total += loss
        losses.append(total)
        for k in range(2):
            p[k], g1[k], g2[k] = adam_literal(p[k], grads[k], g1[k], g2[k], it, lr)
    return M[0].solve(p[0]), M[1].solve(p[1]), np.asarray(losses)


def normals64(v, faces, topo):
    """the normals from their definitions in the dtype of v (float64 unless v is float32), nothing rounded on the way in or out"""
    v = np.asarray(v)
    v = v if v.dtype == np.float32 else v.astype(np.float64)
    e = v.dtype.type
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = _cross(b - a, c - b)
    fn = n / (np.sqrt(_dot(n, n)) + e(1e-8))[:, None]
    x = _cross(c - a, b - a)
    s = np.zeros_like(v)
    np.add.at(s, f.reshape(-1), np.repeat(n, 3, axis=0))
    l = np.sqrt(_dot(s, s))
    return fn, np.sqrt(_dot(x, x)) / e(2), s / np.maximum(l, e(1e-6))[:, None]

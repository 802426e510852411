"""The project's own restatement of the mesh connectivity and Taubin smoothing that ra_topo_create / ra_mesh_smooth compute
(include/relightableavatar.h), in numpy, and the seed-built meshes the topology tests share.

Written from the rules, not from the reference's program text:
  - half-edge 3 f + k leaves corner k of face f towards corner (k + 1) % 3;
  - an edge is the unordered pair of a half-edge's ends, its id the rank in lexicographic (min, max) order;
  - twin = the other half-edge of an edge that has exactly two, else -(the edge's number of half-edges);
  - a Taubin pass, per (vertex, channel), every step one rounded operation of `dtype`:
        s = ((0 + x[n_0]) + x[n_1]) + ...  over the neighbours ascending,  l = s * inv - v,  v' = v + c * l,
    inv = 1 / deg (0 for deg = 0), c = alpha then -(alpha + 0.01); every pass reads the previous pass's rows (Jacobi).
"""
import numpy as np


# ---------------------------------------------------------------------------------------------- connectivity
def halfedge_build(faces, n_verts):
    """faces (F,3) int, n_verts -> dict of int64 arrays: vert, twin, edge (3F,), edges (E,2), edge_counts (E,), edge_he_start (E+1,),
    edge_he (3F,), nbr_start (V+1,), nbr (2E,), out_start (V+1,), out_he (3F,), and E, max_valence, max_outgoing"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F, V = len(faces), int(n_verts)
    HE = 3 * F
    vert = faces.reshape(-1)
    nxt = np.roll(faces, -1, axis=1).reshape(-1)
    lo, hi = np.minimum(vert, nxt), np.maximum(vert, nxt)
    key = lo * (1 << 32) + hi
    order = np.argsort(key, kind='stable')          # half-edges ascending inside an edge
    ks = key[order]
    head = np.ones(HE, dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    eid = np.cumsum(head) - 1
    E = int(head.sum())
    edge = np.empty(HE, dtype=np.int64)
    edge[order] = eid
    start = np.flatnonzero(head)
    edge_he_start = np.append(start, HE).astype(np.int64)
    counts = np.diff(edge_he_start)
    edges = np.stack([lo[order][start], hi[order][start]], axis=1).reshape(-1, 2).astype(np.int64)
    twin = np.empty(HE, dtype=np.int64)
    for e in range(E):
        s, c = edge_he_start[e], counts[e]
        hs = order[s:s + c]
        if c == 2:
            twin[hs[0]], twin[hs[1]] = hs[1], hs[0]
        else:
            twin[hs] = -c
    nb = [[] for _ in range(V)]
    for a, b in edges:
        nb[a].append(b)
        nb[b].append(a)         # an edge (a, a) lists a twice under a
    nb = [sorted(x) for x in nb]
    nbr_start = np.concatenate([[0], np.cumsum([len(x) for x in nb])]).astype(np.int64)
    nbr = np.asarray([y for x in nb for y in x], dtype=np.int64)
    out = [[] for _ in range(V)]
    for h in range(HE):
        out[vert[h]].append(h)
    out_start = np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.int64)
    out_he = np.asarray([y for x in out for y in x], dtype=np.int64)
    return dict(vert=vert.copy(), twin=twin, edge=edge, edges=edges, edge_counts=counts.astype(np.int64), edge_he_start=edge_he_start,
                edge_he=order.astype(np.int64), nbr_start=nbr_start, nbr=nbr, out_start=out_start, out_he=out_he, E=E,
                max_valence=int(max([len(x) for x in nb], default=0)), max_outgoing=int(max([len(x) for x in out], default=0)))


def face_connectivity(topo):
    """(edges_connecting_faces (M,2), connected_faces (M,2)) over the manifold edges in edge order, the lower half-edge first"""
    first = topo['edge_he_start'][:-1][topo['edge_counts'] == 2]
    inds = np.stack([topo['edge_he'][first], topo['edge_he'][first + 1]], axis=1).reshape(-1, 2)
    return topo['vert'][inds], inds // 3


def reference_decoded_edges(edges, faces):
    """what the reference's get_edges returns for the true `edges`: it hashes with V = faces.max() and decodes u // V, u % V"""
    Vm = int(np.asarray(faces).max())
    u = edges[:, 0] * Vm + edges[:, 1]
    return np.stack([u // Vm, u % Vm], axis=1)


# ---------------------------------------------------------------------------------------------- Taubin smoothing
def taubin(values, topo, inds=None, alpha=0.33, iters=90, dtype=np.float32):
    """values (V,C) -> (V,C) of dtype, in the kernel's operation order"""
    x = np.array(values, dtype=dtype)
    x = x.reshape(len(x), x.size // max(len(x), 1))
    V = x.shape[0]
    start, nbr = topo['nbr_start'], topo['nbr']
    deg = np.diff(start)
    one = dtype(1)
    inv = np.zeros(V, dtype=dtype)
    inv[deg > 0] = one / deg[deg > 0].astype(dtype)
    alpha = dtype(alpha)
    coeff = (alpha, -(alpha + dtype(0.01)))
    move = np.ones(V, dtype=bool)
    if inds is not None:
        move[:] = False
        move[np.asarray(inds)] = True
    maxdeg = int(deg.max()) if V else 0
    for it in range(2 * iters):
        s = np.zeros_like(x)
        for k in range(maxdeg):
            has = deg > k
            s[has] = s[has] + x[nbr[start[:-1][has] + k]]
        m = s * inv[:, None]
        l = m - x
        p = coeff[it & 1] * l
        y = x + p
        x = np.where(move[:, None], y, x).astype(dtype)
    return x


# ---------------------------------------------------------------------------------------------- one Loop step
def _next(h):
    return h - h % 3 + (h + 1) % 3


def _prev(h):
    return h - h % 3 + (h + 2) % 3


def loop_table(n_max, dtype=np.float64):
    """(n_max + 1, 2): w_self = 1 / n - beta and beta = (1 / n)(5 / 8 - (3 / 8 + cos(2 pi / n) / 4)^2) for n outgoing half-edges,
    computed in float64 and rounded once to dtype; row 0 is unused"""
    n = np.arange(1, n_max + 1, dtype=np.float64)
    beta = (1.0 / n) * (0.625 - (0.375 + 0.25 * np.cos(2.0 * np.pi / n)) ** 2)
    t = np.zeros((n_max + 1, 2), dtype=np.float64)
    t[1:, 0], t[1:, 1] = 1.0 / n - beta, beta
    return t.astype(dtype)


def loop_step(values, topo, table, dtype=np.float32):
    """values (V,C) -> (V + E, C) of dtype: every row the sum of its half-edges' contributions in ascending half-edge order, every
    contribution in the named operations of csrc/ra_topo_rules.hpp, one rounding each"""
    x = np.array(values, dtype=dtype)
    x = x.reshape(len(x), x.size // max(len(x), 1))
    V, E = len(x), topo['E']
    vert, twin = topo['vert'], topo['twin']
    table = np.asarray(table, dtype=dtype)
    c3, c8, c18, c38 = dtype(3), dtype(0.125), dtype(0.125), dtype(0.375)
    out = np.zeros((V + E, x.shape[1]), dtype=dtype)

    def open_term(v, other):
        a = c18 * other
        b = c38 * v
        return a + b
    for v in range(V):
        hs = topo['out_he'][topo['out_start'][v]:topo['out_start'][v + 1]]
        is_open = any(twin[h] < 0 for h in hs)
        w_self, beta = table[len(hs)]
        acc = np.zeros(x.shape[1], dtype=dtype)
        for h in hs:
            xv, xn = x[vert[h]], x[vert[_next(h)]]
            if is_open:
                c = np.zeros(x.shape[1], dtype=dtype)
            else:
                a = w_self * xv
                b = beta * xn
                c = a + b
            if twin[h] < 0:
                c = c + open_term(xv, xn)
            tp = twin[_prev(h)]
            if tp >= 0 and twin[_prev(tp)] < 0:
                c = c + open_term(x[vert[tp]], x[vert[_prev(tp)]])
            acc = acc + c
        out[v] = acc
    for e in range(E):
        acc = np.zeros(x.shape[1], dtype=dtype)
        for h in topo['edge_he'][topo['edge_he_start'][e]:topo['edge_he_start'][e + 1]]:
            xv = x[vert[h]]
            if twin[h] >= 0:
                a = c3 * xv
                b = a + x[vert[_prev(h)]]
                c = b * c8
            else:
                s = xv + x[vert[_next(h)]]
                c = s / dtype(2 * -twin[h])
            acc = acc + c
        out[V + e] = acc
    return out


def child_topology(topo, n_verts):
    """the connectivity of the subdivided mesh by index arithmetic on the parent's twin / vert / edge: the same keys as halfedge_build.
    Edge e splits into 2 e and 2 e + 1, the middle edge opposite half-edge h is 2 E + h; `edges` lists the ends of each id's lowest
    half-edge; the neighbour lists come from `edges`, as the build makes them"""
    vert, twin, edge, E, V = topo['vert'], topo['twin'], topo['edge'], topo['E'], int(n_verts)
    HE = len(vert)
    nv, nt, ne = (np.empty(4 * HE, dtype=np.int64) for _ in range(3))
    for h in range(HE):
        pv = _prev(h)
        tw, tp = twin[h], twin[pv]
        i0, i1, i2, i3 = 3 * h, 3 * h + 1, 3 * h + 2, 3 * HE + h
        nt[i0] = 3 * _next(tw) + 2 if tw >= 0 else tw
        nt[i1], nt[i3] = i3, i1
        nt[i2] = 3 * tp if tp >= 0 else tp
        ne[i0] = 2 * edge[h] + (1 if h < tw else 0) if tw >= 0 else 2 * edge[h]
        ne[i1] = ne[i3] = 2 * E + h
        ne[i2] = 2 * edge[pv] + (1 if pv > tp else 0) if tp >= 0 else 2 * edge[pv] + 1
        nv[i0], nv[i1], nv[i2], nv[i3] = vert[h], V + edge[h], V + edge[pv], V + edge[pv]
    E2, V2 = 2 * E + HE, V + E
    order = np.argsort(ne, kind='stable')
    counts = np.bincount(ne, minlength=E2).astype(np.int64)
    ehe_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    edges = np.empty((E2, 2), dtype=np.int64)
    for e in range(E2):
        x = order[ehe_start[e]]
        a, b = nv[x], nv[_next(x)]
        edges[e] = (min(a, b), max(a, b))
    nb = [[] for _ in range(V2)]
    for a, b in edges:
        nb[a].append(b)
        nb[b].append(a)
    nb = [sorted(x) for x in nb]
    out = [[] for _ in range(V2)]
    for h in range(4 * HE):
        out[nv[h]].append(h)
    cat = lambda ls: np.asarray([y for x in ls for y in x], dtype=np.int64)
    starts = lambda ls: np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64)
    return dict(vert=nv, twin=nt, edge=ne, edges=edges, edge_counts=counts, edge_he_start=ehe_start, edge_he=order.astype(np.int64),
                nbr_start=starts(nb), nbr=cat(nb), out_start=starts(out), out_he=cat(out), E=E2,
                max_valence=int(max([len(x) for x in nb], default=0)), max_outgoing=int(max([len(x) for x in out], default=0)))


def subdivide(values, topo, steps, dtype=np.float32, table_dtype=None):
    """`steps` Loop steps: (values, faces (F,3), topo) of the last level"""
    x = np.array(values, dtype=dtype)
    for _ in range(steps):
        table = loop_table(max(topo['max_outgoing'], 1), table_dtype or dtype)
        y = loop_step(x, topo, table, dtype)
        topo = child_topology(topo, len(x))
        x = y
    return x, topo['vert'].reshape(-1, 3), topo


# ---------------------------------------------------------------------------------------------- meshes
def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int64)
    return v, f


def midpoint_split(v, f):
    """every face into four through its edge midpoints, pushed to the unit sphere (a way to build test meshes, not Loop subdivision)"""
    mid, nv, nf = {}, list(v), []

    def m(a, b):
        k = (min(a, b), max(a, b))
        if k not in mid:
            p = (v[a] + v[b]) / 2
            mid[k] = len(nv)
            nv.append(p / np.linalg.norm(p))
        return mid[k]
    for a, b, c in f:
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
    return np.asarray(nv), np.asarray(nf, dtype=np.int64)


def sphere(levels, seed):
    """the octahedron split `levels` times (V = 6, 18, 66, 258, 1026), vertices jittered"""
    v, f = octahedron()
    for _ in range(levels):
        v, f = midpoint_split(v, f)
    rng = np.random.default_rng(seed)
    return 0.8 * v + rng.uniform(-0.02, 0.02, v.shape) * (levels > 0), f


def drop_vertices(v, f, k):
    """without the last k vertices and the faces that use them (an open cap per vertex), re-indexed"""
    keep = np.all(f < len(v) - k, axis=1)
    return v[:len(v) - k], f[keep]


def patch(n, seed=0):
    """an n x n vertex grid, two triangles per cell, the diagonals all one way: the corners (0, n-1) and (n-1, 0) belong to one face
    each (the two ears)"""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    v = np.stack([xs.ravel(), ys.ravel(), np.zeros(n * n)], axis=1).astype(np.float64) / (n - 1)
    # general position in all three coordinates.  On the bare grid x and y are multiples of 1 / 4 and every product and sum of a
    # subdivision step is exact in float32, so the reference's float32 run has no error there to measure anything against (it was
    # 3.7e-9 of the extent, all of it from z, against the half ulp 6.0e-8 that any float32 sum of six terms near 0.5 may be off by)
    v[:, :2] += rng.uniform(-0.02, 0.02, (n * n, 2))
    v[:, 2] = 0.05 * rng.standard_normal(n * n)
    f = []
    for y in range(n - 1):
        for x in range(n - 1):
            a, b, c, d = y * n + x, y * n + x + 1, (y + 1) * n + x, (y + 1) * n + x + 1
            f += [[a, b, d], [a, d, c]]
    return v, np.asarray(f, dtype=np.int64)


def fin():
    """the 5 x 5 patch plus a third face on an interior edge"""
    v, f = patch(5, seed=1)
    v = np.vstack([v, [[0.5, 0.5, 0.6]]])
    a, b = 6, 7          # an interior grid edge
    return v, np.vstack([f, [[a, b, len(v) - 1]]])


def two_components():
    v0, f0 = sphere(1, seed=2)
    v1, f1 = patch(4, seed=3)
    return np.vstack([v0, v1 + 2.0]), np.vstack([f0, f1 + len(v0)])


def fan(n=40):
    """n triangles around vertex 0: valence n, open"""
    t = np.linspace(0, 1.9 * np.pi, n + 1)
    v = np.vstack([[[0, 0, 0.3]], np.stack([np.cos(t), np.sin(t), 0 * t], axis=1)])
    f = np.asarray([[0, k + 1, k + 2] for k in range(n)], dtype=np.int64)
    return v, f


def unreferenced():
    """an octahedron with a vertex no face uses in the middle of the numbering and one at the end"""
    v, f = sphere(0, seed=0)
    v = np.vstack([v[:3], [[0.3, 0.2, 0.1]], v[3:], [[-0.4, 0.5, 0.6]]])
    f = np.where(f >= 3, f + 1, f)
    return v, f


def repeated_index():
    """a patch one of whose faces is [a, a, b]"""
    v, f = patch(4, seed=4)
    f = f.copy()
    f[5] = [f[5][0], f[5][0], f[5][1]]
    return v, f


def _append(v, f, k):
    return np.vstack([v, np.full((k, 3), 0.25) + 0.01 * np.arange(k)[:, None]]), f


MESHES = {
    'octa': lambda: sphere(0, 0),
    'sphere66': lambda: sphere(2, 5),
    'sphere258': lambda: sphere(3, 6),
    'sphere1026': lambda: sphere(4, 7),
    'v63': lambda: drop_vertices(*sphere(2, 5), 3),
    'v64': lambda: drop_vertices(*sphere(2, 5), 2),
    'v65': lambda: drop_vertices(*sphere(2, 5), 1),
    'v255': lambda: drop_vertices(*sphere(3, 6), 3),
    'v256': lambda: drop_vertices(*sphere(3, 6), 2),
    'v257': lambda: _append(*drop_vertices(*sphere(3, 6), 3), 2),
    'patch5': lambda: patch(5, 0),
    'fin': fin,
    'two': two_components,
    'fan40': fan,
    'unref': unreferenced,
    'repeat': repeated_index,
}
# the meshes whose every vertex is used by a face: the reference's get_edges / triangle_to_halfedge(None, faces) see the same vertex count
SMOOTH_GOLDEN = ('octa', 'sphere66', 'v65', 'patch5', 'fin', 'two', 'fan40', 'unref', 'repeat')
_cache = {}


def mesh(name):
    """(verts float64 (V,3), faces int64 (F,3)), built once and shared read-only"""
    if name not in _cache:
        v, f = MESHES[name]()
        v, f = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64)
        v.setflags(write=False), f.setflags(write=False)
        _cache[name] = (v, f)
    return _cache[name]


def topo(name):
    key = ('topo', name)
    if key not in _cache:
        v, f = mesh(name)
        _cache[key] = halfedge_build(f, len(v))
    return _cache[key]


def smooth_inds(name):
    """the `inds` subset of the smoothing cases: every third vertex"""
    return np.arange(0, len(mesh(name)[0]), 3)


def loop_steps(name):
    """the Loop steps the golden holds for a mesh: 1 and 2 below 255 vertices, 1 for sphere258, none for the others (the file's size)"""
    return (1, 2) if len(mesh(name)[0]) < 255 else (1,) if name == 'sphere258' else ()


def smooth_iters(name):
    """the iteration counts the golden holds the reference's smoothing for: the largest mesh has the long run only"""
    return (90,) if len(mesh(name)[0]) > 1000 else (1, 2, 90)

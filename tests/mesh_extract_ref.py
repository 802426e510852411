"""Host restatements for the mesh-extraction tests: a numpy marching cubes with the library's vertex and face order rule, the
float32 interpolation, the component rule, the property list that holds for ANY correct marching cubes, and the test volumes.

Nothing here knows mcubes or trimesh (neither is installed): the evidence for the iso-surface is the property list, computed from
the input volume and the returned mesh only.  The triangle table is the package's (relightableavatar_amd/mcubes_tables.py, derived by
rule); the properties do not use it.

The numpy marching cubes and the device share that ONE table, so bit equality between the two says that the device applies the table,
the ownership rule and the interpolation as stated — it says nothing about the table itself.  What vouches for the table is the
property list alone (closed, consistently oriented, one vertex per crossed edge, normals towards smaller values), on all 256 cases
and on volumes that make every face ambiguous."""
import numpy as np

from relightableavatar_amd import mcubes_tables as T

F32 = np.float32


def interp32(base, a, b, iso):
    """the vertex coordinate: base + (iso - a) / (b - a), every step one rounded float32 operation"""
    base, a, b, iso = (np.asarray(v, F32) for v in (base, a, b, iso))
    with np.errstate(all='ignore'):
        return (base + ((iso - a).astype(F32) / (b - a).astype(F32)).astype(F32)).astype(F32)


def crossed_edges(vol, iso):
    """(nx,ny,nz,3) bool: the edge leaving each grid point along x / y / z has its ends on two sides of iso (below: v < iso)"""
    below = vol < F32(iso)
    c = np.zeros(vol.shape + (3,), bool)
    c[:-1, :, :, 0] = below[:-1] != below[1:]
    c[:, :-1, :, 1] = below[:, :-1] != below[:, 1:]
    c[:, :, :-1, 2] = below[:, :, :-1] != below[:, :, 1:]
    return c


def edge_vertices(vol, iso):
    """the vertex of every crossed edge, in (owning point's linear index, axis) order: (V,3) float32"""
    vol = np.ascontiguousarray(vol, F32)
    c = crossed_edges(vol, iso)
    p, axis = np.nonzero(c.reshape(-1, 3))
    xyz = np.stack(np.unravel_index(p, vol.shape), 1)
    other = xyz.copy()
    other[np.arange(len(p)), axis] += 1
    a, b = vol[tuple(xyz.T)], vol[tuple(other.T)]
    v = xyz.astype(F32)
    v[np.arange(len(p)), axis] = interp32(xyz[np.arange(len(p)), axis].astype(F32), a, b, iso)
    return v


def marching_cubes(vol, iso):
    """(verts (V,3) float32 in index coordinates, faces (F,3) int32): vertices by (owning grid point, axis), faces by (cell, table order)"""
    vol = np.ascontiguousarray(vol, F32)
    nx, ny, nz = vol.shape
    verts = edge_vertices(vol, iso)
    c = crossed_edges(vol, iso)
    vid = (np.cumsum(c.reshape(-1)) - 1).reshape(nx, ny, nz, 3)
    below = vol < F32(iso)
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for k, (dx, dy, dz) in enumerate(T.CORNERS):
        case |= below[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << k
    _, n_tri, tri_table, _ = T.build_tables()
    cells = np.stack(np.nonzero(n_tri[case] > 0), 1)            # row-major: by linear index
    cc = case[tuple(cells.T)]
    owner, axis = np.array(T.EDGE_OWNER), np.array(T.EDGE_AXIS)
    e = tri_table[cc]                                           # (cells, 3 * MAX_TRI)
    ok = e >= 0
    es = np.where(ok, e, 0)
    q = cells[:, None, :] + owner[es]
    idx = vid[q[..., 0], q[..., 1], q[..., 2], axis[es]]
    assert c[q[..., 0], q[..., 1], q[..., 2], axis[es]][ok].all()
    faces = idx[ok].reshape(-1, 3).astype(np.int32)
    return verts, faces


# ---------------------------------------------------------------------------------------------- components
def face_labels(faces):
    """per face the lowest face index of its component; faces are connected through shared (undirected) edges"""
    faces = np.asarray(faces).reshape(-1, 3)
    parent = list(range(len(faces)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    first = {}
    for f, tri in enumerate(faces.tolist()):
        for j in range(3):
            a, b = tri[j], tri[(j + 1) % 3]
            key = (a, b) if a < b else (b, a)
            g = first.setdefault(key, f)
            ra, rb = find(f), find(g)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(len(faces))], np.int64)


def largest_component(verts, faces):
    """the component with the most (distinct, referenced) vertices, ties to the one with the lowest face index; referenced vertices and
    faces in their original order, faces re-indexed"""
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    if len(faces) == 0:
        return np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)
    lab = face_labels(faces)
    best, best_n = None, -1
    for l in np.unique(lab):            # ascending: a later equal does not replace
        n = len(np.unique(faces[lab == l]))
        if n > best_n:
            best, best_n = l, n
    kept = faces[lab == best]
    used = np.zeros(len(verts), bool)
    used[kept.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return verts[used], new[kept].astype(np.int32)


# ---------------------------------------------------------------------------------------------- properties
def mesh_figures(verts, faces):
    """closedness and orientation figures of a mesh: how many directed edges occur more than once, how many lack their opposite"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = max(len(verts), 1)
    de = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    key, rev = de[:, 0] * V + de[:, 1], de[:, 1] * V + de[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    und = np.unique(np.minimum(key, rev))
    return dict(repeated_directed=int((cnt > 1).sum()), unmatched=int((~np.isin(rev, uniq)).sum()), n_edges=len(und),
                out_of_range=int(((faces < 0) | (faces >= len(verts))).sum()),
                repeats_in_face=int(((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 2] == faces[:, 0])).sum()))


def check_properties(vol, iso, verts, faces, closed=True):
    """properties 1, 2, 3 and 5 of the list (module docstring of test_oracle_mesh_extract.py); returns the figures it checked"""
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    want = edge_vertices(vol, iso)
    fig = dict(n_verts=len(verts), n_faces=len(faces), n_crossed_edges=len(want))
    assert len(verts) == len(want), fig                                                     # 1
    rows = lambda a: sorted(np.ascontiguousarray(a, F32).view(np.uint32).reshape(-1, 3).tolist())
    assert rows(verts) == rows(want), 'a vertex is not on a crossed edge at the restated t'  # 2 (as multisets: bit for bit)
    fig.update(mesh_figures(verts, faces))
    assert fig['out_of_range'] == 0 and fig['repeats_in_face'] == 0, fig                    # 5
    if closed:
        assert fig['repeated_directed'] == 0 and fig['unmatched'] == 0, fig                 # 3: two faces per edge, opposite directions
    if len(faces):
        assert len(np.unique(faces)) == len(verts), 'a vertex no face refers to'
    return fig


def euler(verts, faces):
    return len(verts) - mesh_figures(verts, faces)['n_edges'] + len(faces)


def signed_volume(verts, faces):
    """positive when the face normals point out of the enclosed region"""
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum('ij,ij->i', v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def edge_directions(vol, iso):
    """per vertex, in edge_vertices' order, the unit vector along its grid edge from the end that is not below to the end that is"""
    vol = np.ascontiguousarray(vol, F32)
    c = crossed_edges(vol, iso)
    p, axis = np.nonzero(c.reshape(-1, 3))
    xyz = np.unravel_index(p, vol.shape)
    d = np.zeros((len(p), 3))
    d[np.arange(len(p)), axis] = np.where(vol[xyz] < F32(iso), -1.0, 1.0)       # the owning point below: towards it
    return d


def normals_towards_smaller(vol, iso, verts, faces):
    """the number of components whose face normals do NOT point towards smaller volume values.  Needs vertices in the library's order
    and a consistently oriented mesh (property 3): then one sign per component decides, and it is taken from all its faces together —
    the sum over faces of (area normal) . (the three vertices' edge directions towards the below end) must be positive.  Also returns
    the number of single faces for which that product is not positive (a figure: a face of a fan may lean either way)."""
    if len(faces) == 0:
        return 0, 0
    faces = np.asarray(faces, np.int64)
    v = np.asarray(verts, np.float64)[faces]
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    s = np.einsum('ij,ij->i', n, edge_directions(vol, iso)[faces].sum(1))
    lab = face_labels(faces)
    return int(sum(s[lab == l].sum() <= 0 for l in np.unique(lab))), int((s <= 0).sum())


# ---------------------------------------------------------------------------------------------- volumes
OUTSIDE = F32(-1.0)      # the volumes are -sdf: below iso = 0 is outside


def pattern_volume(case):
    """one cell with the corner signs of `case` (bit k: corner k below) in a 4 x 4 x 4 volume of outside; every corner its own magnitude"""
    vol = np.full((4, 4, 4), OUTSIDE, F32)
    for k, (dx, dy, dz) in enumerate(T.CORNERS):
        mag = F32(0.25) + F32(0.1) * F32(k)
        vol[1 + dx, 1 + dy, 1 + dz] = -mag if (case >> k) & 1 else mag
    return vol


def all_patterns_volume():
    """the 256 pattern volumes side by side along z: (4, 4, 1024); the layers of outside keep them apart"""
    return np.concatenate([pattern_volume(c) for c in range(256)], 2)


SPHERE = dict(n=24, centre=(11.3, 11.6, 11.45), R=8.0)
TORUS = dict(n=24, centre=(11.3, 11.6, 11.45), R=7.0, r=3.0)


def _grid(n, centre):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing='ij'), -1)
    return g - np.array(centre)


def sphere_volume(n=SPHERE['n'], centre=SPHERE['centre'], R=SPHERE['R']):
    return (R - np.linalg.norm(_grid(n, centre), axis=-1)).astype(F32)


def torus_volume(n=TORUS['n'], centre=TORUS['centre'], R=TORUS['R'], r=TORUS['r']):
    g = _grid(n, centre)
    return (r - np.sqrt((np.linalg.norm(g[..., :2], axis=-1) - R) ** 2 + g[..., 2] ** 2)).astype(F32)


def random_volume(shape=(9, 10, 11), seed=0, pad=1):
    """uniform values in (-1, 1) inside a border of outside, so that no surface reaches the border"""
    vol = np.full(shape, OUTSIDE, F32)
    inner = tuple(s - 2 * pad for s in shape)
    vol[pad:-pad, pad:-pad, pad:-pad] = np.random.default_rng(seed).uniform(-1, 1, inner).astype(F32)
    return vol


def exact_iso_volume():
    """corners exactly equal to iso = 0 (they count as not below): a blob whose surface runs through grid points"""
    vol = np.full((7, 8, 9), OUTSIDE, F32)
    vol[2:5, 2:6, 2:7] = 0.0
    vol[3, 3:5, 3:6] = 1.0
    vol[2, 2, 2] = 0.5
    return vol


def sphere_volume_bounds(R, h=1.0):
    """[lo, hi] of the volume a marching-cubes mesh of f = R - |x - c| encloses, from the voxel size h alone.
    Along a grid edge f'' = -d^2 / r^3 (d: the edge's line's distance from the centre), so within a crossed edge (r >= R - h) the linear
    interpolant is off by at most eps = h^2 / (8 (R - h)): since f is the exact distance, every vertex has |r - R| <= eps.  A point of a
    triangle, x = sum l_i v_i, has |x|^2 = sum l_i |v_i|^2 - sum_{i<j} l_i l_j |v_i - v_j|^2 >= (R - eps)^2 - D^2 / 3 with D = sqrt(3) h the
    diameter of a cell, and |x| <= R + eps by convexity.  So the surface lies between the spheres of radius sqrt((R - eps)^2 - h^2) and
    R + eps, and a closed surface of one component and Euler characteristic 2 between them encloses the inner ball and lies in the outer one."""
    eps = h * h / (8.0 * (R - h))
    r_in, r_out = np.sqrt((R - eps) ** 2 - h * h), R + eps
    return 4.0 / 3.0 * np.pi * r_in ** 3, 4.0 / 3.0 * np.pi * r_out ** 3


def torus_volume_bounds(R, r, h=1.0):
    """the same for f = r - dist(x, C), C the circle of radius R; D = sqrt(3) h is a cell's diameter.
    Vertices: the second derivative of the distance to C along a line is at most 1 / min(delta, R - delta) at tube distance delta, so a
    vertex has |dist - r| <= eps = h^2 / (8 min(r - h, R - r - h)).
    Inner tube radius.  For a point x of a triangle let c be the point of C nearest to x and L the tangent of C at c: dist(x, C) =
    dist(x, L).  The squared distance to a line is a quadratic form, so dist(x, L)^2 = sum l_i dist(v_i, L)^2 - sum_{i<j} l_i l_j
    |P (v_i - v_j)|^2 >= min_i dist(v_i, L)^2 - D^2 / 3.  A vertex is within D of x, so its coordinate s along L is at most D, and the
    circle leaves its tangent by R - sqrt(R^2 - s^2) <= s^2 / R there: dist(v_i, C) <= dist(v_i, L) + D^2 / R.  Hence
    dist(x, C) >= sqrt((r - eps - D^2 / R)^2 - D^2 / 3).
    Outer tube radius.  Every point of a triangle with sides <= D is within D / sqrt(3) = h of a vertex and the distance to C is
    1-Lipschitz: dist(x, C) <= r + eps + h.
    A closed surface of one component and Euler characteristic 0 between the two tori encloses the inner one and lies in the outer
    one; a torus of tube radius rho has the volume 2 pi^2 R rho^2."""
    eps = h * h / (8.0 * min(r - h, R - r - h))
    lo, hi = np.sqrt((r - eps - 3.0 * h * h / R) ** 2 - h * h), r + eps + h
    return 2.0 * np.pi ** 2 * R * lo ** 2, 2.0 * np.pi ** 2 * R * hi ** 2


def last_cell_volume(shape=(5, 6, 7)):
    """the only crossing cell is the last one in every axis: one corner — the last grid point — is inside"""
    vol = np.full(shape, OUTSIDE, F32)
    vol[-1, -1, -1] = 0.75
    return vol


def sphere_mesh(centre, R, n=16):
    """a closed sphere mesh (the numpy marching cubes of a ball), shifted: building block of the component tests"""
    v, f = marching_cubes(sphere_volume(n, (n / 2 - 0.3,) * 3, R), 0.0)
    return v + np.asarray(centre, F32), f


# ---------------------------------------------------------------------------------------------- the scalar volume from the oracle
VOLUME_VOXEL = [0.029, 0.029, 0.029]        # about 2 * 10^4 grid points on the synthetic body's bounds; no axis a multiple of a tile or a wave
VOLUME_SEED = 0
ULP = 2.0 ** -23


def volume_inputs(mode, seed=VOLUME_SEED, voxel=VOLUME_VOXEL):
    """(body, axes, verts) of a mode: the T-pose bounds and template vertices for canonical / tpose, the world ones for posed"""
    import torch
    from relightableavatar_amd import data_utils, synthetic
    body = synthetic.make_body(seed, posed=True)
    if mode == 'posed':
        verts = body['pverts'][0] @ body['R'][0].T + body['Th'].reshape(1, 3)          # ppts = (x - Th) @ R, inverted
        bounds = body['wbounds'][0]
    else:
        verts, bounds = body['tverts'][0], body['tbounds'][0]
    return body, data_utils.mesh_grid_axes(bounds, voxel), verts.float().contiguous()


def oracle_filter(axes, verts, K):
    """t of every grid point, float32 as the reference computes it (mesh_renderer.py:44-45): sample_blend_K_closest_points without
    values — the K nearest vertices' PLAIN distances (cast_knn_points takes the root, sample_utils.py:609), weighted by 1 / (d + 1e-8)"""
    import torch
    from oracle import ra_oracle as O
    pts = torch.stack(torch.meshgrid(*axes, indexing='ij'), dim=-1).float().reshape(-1, 3)
    d = O.knn3(pts, verts, K)[0].sqrt()
    w = 1 / (d + 1e-8)
    w = w / w.sum(dim=-1, keepdim=True)
    return pts, (d * w).sum(dim=-1)


def borderline(t, dist_th):
    """cells whose own t lies within 4 float32 roundings of dist_th: left out of the decision and the value checks"""
    return (t.double() - dist_th).abs() <= 4 * ULP * max(abs(dist_th), 1e-30)


def oracle_volume(mode, sd, cfg, dist_th, emulate=None, fill=-10.0, pad=10):
    """dict(t, kept, values = -sdf of the kept points, volume = the padded (nx + 2 pad, ...) float32 array) from the oracle alone"""
    import torch
    from oracle import ra_oracle as O
    body, axes, verts = volume_inputs(mode)
    pts, t = oracle_filter(axes, verts, cfg.sample_vert_cnt)
    kept = t < dist_th
    net, fr, x = O.OracleNet(sd, cfg, emulate=emulate), O._frame(body), pts[kept]
    if mode == 'canonical':
        sdf = net.sdf_feat(x)[0]
    elif mode == 'tpose':
        sdf = O.observed_sdf(net, x, fr)
    else:
        sdf = O.hdq_sdf(net, x, fr, dist_th, smooth_transition=False)
    values = -sdf.reshape(-1)
    shape = tuple(len(a) for a in axes)
    cube = torch.full((pts.shape[0],), fill, dtype=values.dtype)
    cube[kept] = values
    cube = torch.nn.functional.pad(cube.reshape(shape), (pad,) * 6, value=fill)
    return dict(t=t, kept=kept, values=values, volume=cube, shape=shape, axes=axes, verts=verts, body=body)

"""References and seeded inputs of the frame set-up, image and compositing stages (helper of test_oracle_frame_stages.py /
test_gpu_frame_stages.py; not a test, no fixture, reads no file).

Every stage has ONE reference, a dtype-generic torch function: run in float64 it is the truth, run in float32 it is what the reference
project computes, and its distance from the float64 run is the error a float32 implementation is entitled to (DESIGN.md section 10's rule,
`parity` below).  oracle/ra_oracle.py is reused where it already restates the operation in the dtype of its arguments (get_near_far_aabb,
microfacet_brdf, verts_normals, inverse_3x3, sample_envmap_image, probe_axes, volume renderer, blend_output_); what is restated here is
what the oracle fixes to float32 (torch.linspace / arange / ones without a dtype) or does not have:
    ray_frame          get_rays + get_full_near_far + the box mask of every pixel (synthetic.rays_within_bounds before its mask is applied)
    generate_image     Visualizer.generate_image with the Depth rank clamped to the hit count (csrc/ra_image.hip's documented deviation)
The places where the reference itself rounds to float32 are kept in both runs, they are part of the operation: the Rodrigues entries of
batch_rodrigues, the bone matrices the data pipeline hands on as float32, the ray direction rounded once.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ra_oracle as O

F32, F64 = torch.float32, torch.float64
ULP = 2.0 ** -23


# ------------------------------------------------------------------------------------------------ the parity rule
def parity(label, got, ref32, ref64, keep=None, relative=False, arithmetic=True):
    """max and median |got - ref64|, normalised by max |ref64| (relative: per element by max(|ref64|, 1)), may be
    at most 10 x the float32 reference's own; where that is exactly 0 the floor is 10 * 2^-23 (of max |ref|).  Outputs without arithmetic
    must be bit-equal to the float32 reference.  Prints kernel error, float32 error and ratio; returns the worst ratio."""
    got, r32, r64 = (torch.as_tensor(t).detach().cpu() for t in (got, ref32, ref64))
    assert got.shape == r32.shape == r64.shape, (label, got.shape, r32.shape, r64.shape)
    if not arithmetic:
        same = bool(torch.equal(got, r32.to(got.dtype)))
        print(f'{label}: bit-equal {same} ({got.numel()} values)')
        assert same, label
        return 0.0
    got, r32, r64 = got.double(), r32.double(), r64.double()
    if keep is not None:
        keep = torch.as_tensor(keep).cpu()
        got, r32, r64 = got[keep], r32[keep], r64[keep]
    if got.numel() == 0:
        print(f'{label}: no element to compare')
        return 0.0
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(got).all()), f'{label}: non-finite values'
    scale = r64.abs().clamp(min=1.0) if relative else max(float(r64.abs().max()), 1e-30)
    ek, e32 = (got - r64).abs() / scale, (r32 - r64).abs() / scale
    worst = 0.0
    for name, fn in (('max', torch.max), ('median', torch.median)):
        k, f = float(fn(ek)), float(fn(e32))
        allowed = 10 * f if f > 0 else 10 * ULP
        ratio = k / (f if f > 0 else ULP)
        worst = max(worst, ratio)
        print(f'{label}: {name} kernel {k:.3e}  float32 {f:.3e}  ratio {ratio:.2f}' + ('' if f > 0 else ' (of one ulp: float32 error 0)'))
        assert k <= allowed, f'{label}: {name} |kernel - float64| {k:.3e} > 10 x float32 reference {f:.3e}'
    return worst


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


# ------------------------------------------------------------------------------------------------ a. body state
def rodrigues_cv(rvec):
    """cv2.Rodrigues (base_dataset.py: R = cv2.Rodrigues(Rh)): float64 inside, identity below |r| = 1e-12, float32 out"""
    r = torch.as_tensor(rvec).double().reshape(3)
    th = float(r.norm())
    R = torch.eye(3, dtype=F64)
    if th >= 1e-12:
        k = r / th
        K = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=F64)
        R = R + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    return R


def rigid_transforms64(poses, joints, parents):
    """O.rigid_transforms before its rounding to float32: the per-bone 4 x 4 and the posed joints in float64 (Rodrigues entries rounded
    to float32 as batch_rodrigues returns them)"""
    J = joints.shape[0]
    R = O.rodrigues(poses).double()
    jt = joints.double()
    rel = jt.clone()
    rel[1:] -= jt[parents[1:]]
    T = torch.zeros(J, 4, 4, dtype=F64)
    T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = R, rel, 1.0
    chain = [T[0]]
    for i in range(1, J):
        chain.append(chain[int(parents[i])] @ T[i])
    tr = torch.stack(chain)
    posed = tr[:, :3, 3].clone()
    jh = torch.cat([jt, torch.zeros(J, 1, dtype=F64)], dim=1)
    tr[:, :, 3] = tr[:, :, 3] - (tr * jh[:, None]).sum(-1)
    return tr, posed


def pose_frame(c, dtype, padding=0.05):
    """O.pose_frame in `dtype`.  dtype float32 returns what the reference computes (A, joints, R rounded from float64; the vertex stages in
    float32); dtype float64 keeps A / joints / R unrounded as OUTPUTS and feeds the vertex stages the float32 matrices the pipeline hands on."""
    T_ = lambda a: torch.as_tensor(np.asarray(a))
    parents = T_(c.parents).long()
    A64, J64 = rigid_transforms64(T_(c.poses).float(), T_(c.tjoints).float(), parents)
    R64 = rodrigues_cv(c.Rh)
    A, R = A64.float().to(dtype), R64.float().to(dtype)                       # what the vertex stages read
    w, bigA, tv, Th = T_(c.weights).to(dtype), T_(c.big_A).float().to(dtype), T_(c.tverts).float().to(dtype), T_(c.Th).float().to(dtype)
    Abig = torch.einsum('nj,jab->nab', w, bigA)
    t = tv - Abig[:, :3, 3]
    txyz = (O.inverse_3x3(Abig[:, :3, :3]) * t[:, None]).sum(-1)
    Abw = torch.einsum('nj,jab->nab', w, A)
    pxyz = (Abw[:, :3, :3] * txyz[:, None]).sum(-1) + Abw[:, :3, 3]
    wxyz = pxyz @ R.mT + Th
    bnd = lambda x: torch.stack([x.min(0)[0] - padding, x.max(0)[0] + padding])
    out = O.odict(A=A64.to(dtype) if dtype == F64 else A64.float(), joints=J64.to(dtype) if dtype == F64 else J64.float(),
                  R=R64.to(dtype) if dtype == F64 else R64.float(), tverts=txyz, pverts=pxyz, wverts=wxyz,
                  pnorm=O.verts_normals(pxyz, T_(c.faces).long()), pbounds=bnd(pxyz), wbounds=bnd(wxyz))
    out.bigdet = torch.linalg.det(Abig[:, :3, :3].double())
    return out


def make_tree(J, kind, r):
    p = np.zeros(J, dtype=np.int64)
    for j in range(1, J):
        p[j] = j - 1 if kind == 'chain' else (0 if kind == 'star' else r.integers(0, j))
    return p


def tree_depth(parents):
    d = np.zeros(len(parents), dtype=np.int64)
    for j in range(1, len(parents)):
        d[j] = d[parents[j]] + 1
    return int(d.max()) + 1


def make_poses(J, kind, r):
    axis = r.standard_normal((J, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    if kind == 'zero':
        p = np.zeros((J, 3))
    elif kind == 'tiny':
        p = np.full((J, 3), 1e-7)
    elif kind == 'random':
        p = r.standard_normal((J, 3)) * 0.25
    elif kind == 'near_pi':
        p = axis * (math.pi - 1e-3 * r.uniform(0.1, 1.0, (J, 1)))
    elif kind == 'over_2pi':
        p = axis * (2 * math.pi + r.uniform(0.2, 2.5, (J, 1)))
    else:
        raise KeyError(kind)
    return p.astype(np.float32)


def make_weights(N, J, kind, r):
    w = np.zeros((N, J), dtype=np.float32)
    if kind == 'onehot':
        w[np.arange(N), r.integers(0, J, N)] = 1.0
    elif kind == 'uniform':
        w[:] = np.float32(1.0 / J)
    elif kind == 'four':
        n = min(4, J)
        for v in range(N):
            idx = r.choice(J, n, replace=False)
            x = r.uniform(0.1, 1.0, n)
            w[v, idx] = (x / x.sum()).astype(np.float32)
    else:
        raise KeyError(kind)
    return w


def _hull_faces(pts):
    from scipy.spatial import ConvexHull
    faces = ConvexHull(pts).simplices.astype(np.int64)
    c = np.cross(pts[faces[:, 1]] - pts[faces[:, 0]], pts[faces[:, 2]] - pts[faces[:, 0]])
    flip = (c * pts[faces].mean(1)).sum(-1) < 0
    faces[flip] = faces[flip][:, [0, 2, 1]]
    return faces


def make_mesh(N, kind, r):
    """-> tverts (N,3) float32, faces (F,3) int64.
    hull: closed convex hull of N points on an ellipsoid (N = 3: one triangle).  isolated: the last 5 vertices belong to no face.
    degenerate: hull + one face with a repeated index (zero area, and 3F odd).  fan: vertex 0 is the apex of N - 2 triangles (valence
    N - 1 >= 200 for N >= 201; 3F odd for odd N)."""
    d = r.standard_normal((N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tv = d * np.array([0.35, 0.25, 0.45])
    if kind == 'fan':
        ang = np.linspace(0, 2 * math.pi, N - 1, endpoint=False)
        tv = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([0.4 * np.cos(ang), 0.3 * np.sin(ang), 0.02 * np.sin(5 * ang)], 1)])
        faces = np.stack([np.zeros(N - 2, dtype=np.int64), np.arange(1, N - 1), np.arange(2, N)], 1)
    elif N < 4:
        faces = np.array([[0, 1, 2]], dtype=np.int64)
    elif kind == 'hull':
        faces = _hull_faces(tv)
    elif kind == 'isolated':
        faces = _hull_faces(tv[:N - 5])
    elif kind == 'degenerate':
        faces = _hull_faces(tv)
        faces = np.concatenate([faces, [[faces[0, 0], faces[0, 0], faces[0, 1]]]])
    else:
        raise KeyError(kind)
    return tv.astype(np.float32), faces


#         name               J    tree      pose        Rh       N     weights    big_A       mesh         padding
BODY_CASES = {
    'j1_n3':               (1,   'chain',  'zero',     'zero',  3,    'onehot',  'identity', 'hull',       0.0),
    'j2_n255':             (2,   'star',   'tiny',     'tiny',  255,  'uniform', 'identity', 'hull',       0.05),
    'j24_n256_isolated':   (24,  'random', 'random',   'random', 256, 'four',    'posed',    'isolated',   0.05),
    'j52_n257_fan':        (52,  'random', 'near_pi',  'random', 257, 'four',    'posed',    'fan',        0.05),
    'j65_n1023_degen':     (65,  'chain',  'random',   'random', 1023, 'four',   'posed',    'degenerate', 0.0),
    'j65_n1025_zero':      (65,  'random', 'zero',     'tiny',  1025, 'uniform', 'posed',    'hull',       0.05),
    'j256_n1025_chain':    (256, 'chain',  'over_2pi', 'random', 1025, 'onehot', 'identity', 'hull',       0.05),
    'j256_n6890_star':     (256, 'star',   'random',   'zero',  6890, 'four',    'posed',    'hull',       0.05),
    'j256_n257_random':    (256, 'random', 'random',   'random', 257, 'uniform', 'posed',    'hull',       0.05),
}


def body_case(name):
    """-> the inputs of Engine.pose_frame / pose_frame() as numpy arrays.  big_A 'posed': a real big pose, the transforms of a first
    pose of the same skeleton (kept small along deep trees, so that the blended 3 x 3 stays well conditioned: asserted in the CPU tests)"""
    J, tree, pose, rh, N, wk, big, mesh, padding = BODY_CASES[name]
    r = np.random.default_rng(_seed(name))
    c = O.odict(name=name, padding=padding)
    c.parents = make_tree(J, tree, r)
    c.tjoints = r.uniform(-0.25, 0.25, (J, 3)).astype(np.float32)
    c.poses = make_poses(J, pose, r)
    c.Rh = {'zero': np.zeros(3), 'tiny': np.full(3, 1e-13), 'random': np.array([0.4, -1.1, 0.7])}[rh].astype(np.float32)
    c.Th = np.array([0.03, -0.02, 0.05], dtype=np.float32)
    c.tverts, c.faces = make_mesh(N, mesh, r)
    c.weights = make_weights(N, J, wk, r)
    if big == 'identity':
        c.big_A = np.tile(np.eye(4, dtype=np.float32), (J, 1, 1))
    else:
        c.big_poses = (r.standard_normal((J, 3)) * 0.3 / math.sqrt(tree_depth(c.parents))).astype(np.float32)
        c.big_A = rigid_transforms64(torch.from_numpy(c.big_poses), torch.from_numpy(c.tjoints), torch.from_numpy(c.parents))[0].float().numpy()
    return c


def face_pair(N=256):
    """two face arrays of equal F and N that differ in one index (the adjacency cache is keyed by content)"""
    r = np.random.default_rng(77)
    tv, f1 = make_mesh(N, 'hull', r)
    f2 = f1.copy()
    used = set(f2[3].tolist())
    f2[3, 1] = next(v for v in range(N) if v not in used)
    return tv, f1, f2


# ------------------------------------------------------------------------------------------------ b. ray generation
def ray_frame(H, W, K, R, T, bounds, dtype):
    """data_utils.py:827-845 (get_rays), :860-875 (get_full_near_far) for EVERY pixel, mask not applied: ray_o, ray_d (H*W,3) as the
    float32 values the reference stores (direction computed in float64 from the float64 camera and rounded once), near, far (H*W) and the
    box mask in `dtype`"""
    K, R, T = (torch.as_tensor(np.asarray(a, dtype=np.float64)) for a in (K, R, T))
    T = T.reshape(3, 1)
    o = -(R.mT @ T).ravel()
    i, j = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing='ij')
    xy1 = torch.stack([j, i, torch.ones_like(i)], dim=2)
    pw = (xy1 @ torch.inverse(K).mT - T.ravel()) @ R
    d = pw - o[None, None]
    d = (d / d.norm(dim=2, keepdim=True)).reshape(-1, 3).float()
    o32 = o.float()[None].expand(H * W, 3)
    dd, oo, b = d.to(dtype), o32.to(dtype), torch.as_tensor(np.asarray(bounds, dtype=np.float32)).to(dtype)
    nd = dd.norm(dim=-1, keepdim=True)
    v = dd / nd
    v[(v < 1e-5) & (v > -1e-10)] = 1e-5
    v[(v > -1e-5) & (v < 1e-10)] = -1e-5
    tmin, tmax = (b[:1] - oo) / v, (b[1:2] - oo) / v
    near, far = torch.minimum(tmin, tmax).max(-1)[0], torch.maximum(tmin, tmax).min(-1)[0]
    mask = near < far
    return O.odict(ray_o=o32, ray_d=d, near=near / nd[:, 0] / nd[:, 0], far=far / nd[:, 0] / nd[:, 0], mask=mask)


def decided(rf64, bounds):
    """pixels whose float64 interval is longer than 1e-4 of the box diagonal in either direction: float32 cannot flip their mask"""
    b = np.asarray(bounds, dtype=np.float64)
    return (rf64.far - rf64.near).abs() > 1e-4 * float(np.linalg.norm(b[1] - b[0]))


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


def make_camera(H, W, kind):
    """'tilted': tilted and rolled, fx != fy, off-centre principal point.  'axis': looking along +z, integer principal point inside the
    image: column cx and row cy have a direction component of exactly 0.  -> K, R (world to camera), T (3,1), float64"""
    if kind == 'axis':
        cx, cy = W // 2, H // 2
        K = np.array([[32.0, 0, cx], [0, 64.0, cy], [0, 0, 1]])              # powers of two: (x - cx) / fx is exact
        R = np.eye(3)
    else:
        K = np.array([[0.9 * max(H, W) + 3.3, 0, 0.43 * W + 0.21], [0, 0.8 * max(H, W) + 1.7, 0.58 * H - 0.13], [0, 0, 1]])
        R = _rot(0.21, -0.17, 0.4)
    origin = np.array([0.05, -0.1, -2.0])
    return K, R, -(R @ origin.reshape(3, 1))


def make_box(kind, H, W, K, R, T):
    """(2,3) float32 box by placement"""
    o = -(R.T @ T).ravel()
    pix = lambda x, y, t: (t * (np.linalg.inv(K) @ np.array([x, y, 1.0])) - T.ravel()) @ R     # the point of pixel (x, y) at camera depth t
    if kind == 'inside':                                                       # the camera sits in the box: near < 0
        lo, hi = o - np.array([0.7, 0.9, 0.5]), o + np.array([1.1, 0.6, 3.0])
    elif kind == 'covering':                                                   # in front, wider than the view
        c = pix(W / 2, H / 2, 2.0)
        lo, hi = c - np.array([30, 30, 0.4]), c + np.array([30, 30, 0.6])
    elif kind == 'one_pixel':
        c = pix(W // 3 + 0.1, H // 2 + 0.2, 2.0)
        s = 2.0 / K[0, 0] * 0.3
        lo, hi = c - s, c + s
    elif kind == 'behind':                                                     # straight behind: the line hits it at negative t
        c = pix(W / 2, H / 2, -3.0)
        lo, hi = c - 0.4, c + 0.4
    elif kind == 'off':                                                        # no ray
        lo, hi = np.array([10.0, 10.0, -9.0]), np.array([11.0, 11.0, -8.0])
    elif kind == 'body':
        c = pix(0.45 * W, 0.55 * H, 2.0)
        lo, hi = c - np.array([0.3, 0.25, 0.2]), c + np.array([0.3, 0.25, 0.2])
    else:
        raise KeyError(kind)
    return np.stack([lo, hi]).astype(np.float32)


RAY_CASES = [(1, 1, 'tilted', 'inside'), (1, 1, 'tilted', 'covering'), (1, 37, 'tilted', 'body'), (1, 37, 'axis', 'covering'),
             (37, 53, 'tilted', 'inside'), (37, 53, 'tilted', 'one_pixel'), (37, 53, 'axis', 'body'), (37, 53, 'tilted', 'behind'),
             (48, 80, 'tilted', 'body'), (48, 80, 'axis', 'inside'), (48, 80, 'tilted', 'off'), (80, 48, 'tilted', 'body'),
             (80, 48, 'axis', 'covering'), (80, 48, 'tilted', 'one_pixel')]


def ray_case(H, W, cam, box):
    K, R, T = make_camera(H, W, cam)
    return K, R, T, make_box(box, H, W, K, R, T)


# ------------------------------------------------------------------------------------------------ c. AABB clip
AABB_SPECIAL = [0.0, 1e-9, 1e-8, -1e-17, -1e-16, -1e-9]
AABB_BOX = np.array([[-0.4, -0.3, -0.5], [0.5, 0.6, 0.45]], dtype=np.float32)


def aabb_case(n):
    """origins inside the box, on a face and outside; every special direction component in each axis, mixed with ordinary ones"""
    r = np.random.default_rng(300 + n)
    d = r.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for i in range(n):
        if i % 2 == 0:
            d[i, (i // 2) % 3] = AABB_SPECIAL[(i // 6) % 6]
        if i % 14 == 0:
            d[i, (i // 2 + 1) % 3] = AABB_SPECIAL[(i // 14) % 6]
    o = r.uniform(-0.3, 0.3, (n, 3))
    o[1::3] = r.uniform(-2.0, 2.0, o[1::3].shape)
    face = o[2::3]
    face[:, 0] = AABB_BOX[0, 0]
    face[1::2, 2] = AABB_BOX[1, 2]
    return torch.from_numpy(o.astype(np.float32)), torch.from_numpy(d.astype(np.float32))


def aabb(o, d, dtype):
    return O.get_near_far_aabb(torch.from_numpy(AABB_BOX).to(dtype), o.to(dtype), d.to(dtype))


# ------------------------------------------------------------------------------------------------ d. BRDF
BRDF_SIZES = [(1, 1), (3, 85), (512, 5)]
ROUGH = [0.09, 0.3, 0.99]
V_DOT_N = [1.0, 1e-4, 0.0, -0.5]


def brdf_case(L, N):
    """p2l (L,N,3), p2c, normal, albedo (N,3), rough (N).  The normal is a world axis (every v.n of V_DOT_N is then exact in both
    precisions); per point: v.n, roughness, albedo 0 / 1 / random cycle; per (light, point): l = v, l = -v (once), l perpendicular to n,
    else random over the sphere.  3 x 85 also has one zero-length normal."""
    r = np.random.default_rng(400 + L * 7 + N)
    n = np.zeros((N, 3)); v = np.zeros((N, 3))
    for p in range(N):
        ax = p % 3
        n[p, ax] = 1.0
        c = V_DOT_N[p % 4] if (L, N) != (1, 1) else 0.6
        phi = r.uniform(0, 2 * math.pi)
        s = math.sqrt(max(0.0, 1 - c * c))
        v[p, ax], v[p, (ax + 1) % 3], v[p, (ax + 2) % 3] = c, s * math.cos(phi), s * math.sin(phi)
    v *= r.uniform(0.5, 3.0, (N, 1))                                           # un-normalised on purpose
    l = r.standard_normal((L, N, 3))
    for p in range(N):
        ax = p % 3
        if p % 4 == 2 and (L, N) != (1, 1):
            continue                                                           # v.n = 0: l = v or l in the tangent plane would put h there too (cos_m = 0, a switch)
        l[0, p] = v[p] * 0.7                                                   # l = v
        if L > 2:
            l[2, p, ax] = 0.0                                                  # l perpendicular to n
    if L > 1:
        l[1, 0] = -v[0]                                                        # l = -v: the half vector is exactly 0
    if (L, N) == (3, 85):
        n[84] = 0.0
    rough = np.array([ROUGH[(p + p // 3) % 3] for p in range(N)])
    alb = r.uniform(0, 1, (N, 3))
    alb[0::3] = 0.0
    alb[1::3] = 1.0
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return O.odict(p2l=f(l), p2c=f(v), normal=f(n), albedo=f(alb), rough=f(rough))


def brdf(c, dtype, lambert_only=False, glossy_only=False):
    """O.microfacet_brdf on (L,N,3) light directions -> (L,N,3)"""
    g = lambda t: t.to(dtype).clone()
    return O.microfacet_brdf(g(c.p2l).permute(1, 0, 2).contiguous(), g(c.p2c), g(c.normal), g(c.albedo), g(c.rough)[:, None], f0=0.02,
                             lambert_only=lambert_only, glossy_only=glossy_only).permute(1, 0, 2)


def brdf_near_switch(c):
    """(L,N) bool: |cos_m| or |h.v / cos_v| below 1e-6 in float64: the step functions of D and G may fall either way in float32"""
    l, v, n = (F.normalize(t.double(), dim=-1, eps=1e-7) for t in (c.p2l, c.p2c, c.normal))
    h = F.normalize(l + v[None], dim=-1, eps=1e-7)
    cos_m = (h * n[None]).sum(-1)
    cos_v = (n * v).sum(-1)
    cos_v = torch.where(cos_v.abs() < 1e-8, torch.where(cos_v >= 0, 1e-8, -1e-8).double(), cos_v)      # safe_divide's clamp
    div = (h * v[None]).sum(-1) / cos_v[None]
    return (cos_m.abs() < 1e-6) | (div.abs() < 1e-6)


# ------------------------------------------------------------------------------------------------ e. envmap
ENV_SHAPES = [(1, 2, 3), (7, 13, 1), (16, 32, 3), (32, 64, 4)]
ENV_SHIFTS = lambda W: [0.0, 1e-3, 0.5, -0.25, float(W), float(-W), 3 * W + 0.75]


def env_image(H, W, C, seed=0):
    return torch.from_numpy(np.random.default_rng(500 + seed + H * W + C).uniform(0.0, 2.0, (H, W, C)).astype(np.float32))


def shift_envmap(image, shift):
    """O.shift_envmap in the image's dtype"""
    H, W = image.shape[:2]
    i, j = torch.meshgrid(torch.arange(0, H), torch.arange(0, W), indexing='ij')
    gx = (j.to(image.dtype) + 0.5 + shift) % W
    grid = torch.stack([gx / W * 2 - 1, (i.to(image.dtype) + 0.5) / H * 2 - 1], dim=-1)[None]
    return F.grid_sample(image.permute(2, 0, 1)[None], grid, align_corners=False, mode='bilinear', padding_mode='border')[0].permute(1, 2, 0)


def gen_light_dirs(env_h, env_w, dtype):
    """normalize(O.gen_light_xyz(env_h, env_w, r)[0]) in dtype (the radius cancels up to rounding; the kernel never multiplies by it)"""
    lat_half, lng_half = math.pi / env_h / 2, 2 * math.pi / env_w / 2
    lats = torch.linspace(math.pi / 2 - lat_half, -math.pi / 2 + lat_half, env_h, dtype=dtype)
    lngs = torch.linspace(math.pi - lng_half, -math.pi + lng_half, env_w, dtype=dtype)
    lngs, lats = torch.meshgrid(lngs, lats, indexing='xy')
    return O.normalize(torch.stack((torch.cos(lats) * torch.cos(lngs), torch.cos(lats) * torch.sin(lngs), torch.sin(lats)), dim=-1))


def add_light_probe(rgb, probe, H, W, cam_R, uH, uW):
    """O.add_light_probe for a given inset size, in rgb's dtype; an empty inset leaves the image as it is"""
    out = rgb.reshape(H, W, 3).clone()
    if uH * uW > 0:
        dt = rgb.dtype
        out[:uH, :uW] = O.sample_envmap_image(probe.to(dt), gen_light_dirs(uH, uW, dt) @ O.probe_axes(cam_R.to(dt)).mT)
    return out.reshape(H * W, 3)


PROBE_IMAGE = (24, 40)
PROBE_INSETS = [(0, 0), (1, 1), (1, 2), (5, 9), (24, 40)]
PROBE_SIZES = [(1, 1), (16, 32), (32, 64)]


def probe_cams():
    """cam_R with cam_R[1][2] (flat index 5) positive, and the same camera rolled half a turn: negative"""
    R = torch.from_numpy(_rot(0.35, -0.6, 0.15).astype(np.float32))
    R2 = R * torch.tensor([[-1.0], [-1.0], [1.0]])
    a, b = (R, R2) if float(R[1, 2]) > 0 else (R2, R)
    assert float(a[1, 2]) > 0 > float(b[1, 2])
    return a, b


# ------------------------------------------------------------------------------------------------ f. visualiser
KINDS = ('Surface', 'Residual', 'Depth', 'Alpha', 'Normal', 'Specular', 'Albedo', 'Roughness', 'Shading', 'Rendering')


def kth(v, k):
    """"a simple version of percentile" (base_visualizer.py:108-109): the k-th smallest and the k-th largest, with torch.topk's NaN rules"""
    v = v.ravel()
    return v.topk(k, largest=False)[0].max(), v.topk(k, largest=True)[0].min()


def generate_image(maps, kind, cfg, H, W, pix, cam_R=None, tbounds=None, dtype=F32, clamp=True):
    """O.generate_image (maps un-batched, the scatter through explicit pixel indices `pix`, no probe inset) in `dtype`.
    clamp: the Depth rank k = int(0.01 P) is clamped to [1, hit count] and an image without a hit is stretched between 0 and 1
    (csrc/ra_image.hip:38-42); k = 0 raises like the reference's topk(0).max()"""
    m = {k: v.to(dtype) for k, v in maps.items()}
    acc = m['acc_map']
    P = acc.shape[0]
    if kind == 'Normal':
        n = O.normalize(m['norm_map']) @ cam_R.to(dtype).mT
        rgb = (n * torch.tensor([1.0, -1.0, -1.0], dtype=dtype) * 0.5 + 0.5) * acc[:, None]
    elif kind == 'Alpha':
        rgb = acc[:, None].expand(-1, 3)
    elif kind == 'Depth':
        d = m['depth_map']
        hit = d[acc != 0]
        k = int(0.01 * d.numel())
        if k < 1:
            raise ValueError('too few rays for the percentile')
        if clamp:
            k = min(k, hit.numel())
        lo, hi = kth(hit, k) if k > 0 else (torch.tensor(0.0, dtype=dtype), torch.tensor(1.0, dtype=dtype))
        lo = lo.clip(None, cfg.min_clip)
        rgb = ((d - lo) / (hi - lo)).clip(0, 1)[:, None].expand(-1, 3)
    elif kind in ('Shading', 'Specular'):
        rgb = m['shade_map' if kind == 'Shading' else 'spec_map']
        if cfg.normalize_shading if kind == 'Shading' else cfg.normalize_specular:
            rgb = rgb / kth(rgb, int(0.005 * rgb.numel()))[1]
    elif kind == 'Albedo':
        rgb = O.linear2srgb(m['albedo_map']) if cfg.tonemapping_albedo else m['albedo_map']
    elif kind == 'Roughness':
        rgb = m['roughness_map'][:, None].expand(-1, 3)
    elif kind == 'Surface':
        tb = tbounds.to(dtype)
        rgb = acc[:, None] * ((m['cpts_map'] - tb[0:1]) / (tb[1:2] - tb[0:1]))
    elif kind == 'Residual':
        d = m['cpts_map'] - m['bpts_map']
        rgb = acc[:, None] * (d / kth(d, int(0.005 * d.numel()))[1])
    elif kind == 'Rendering':
        rgb = m['rgb_map']
    else:
        raise NotImplementedError(kind)
    img = torch.full((H * W, 3), float(cfg.bg_brightness), dtype=dtype)
    img[pix] = rgb
    alpha = torch.zeros(H * W, 1, dtype=dtype)
    alpha[pix] = acc[:, None]
    return torch.cat([img, alpha], dim=-1).reshape(H, W, 4)


IMAGE_P = [100, 101, 199, 200, 257, 4097]


def image_size(P):
    """a non-square H x W with room for P rays and some background"""
    H = max(7, int(math.sqrt(P * 1.3) * 0.8))
    return H, -(-int(P * 1.3) // H)


def image_case(P, seed=0):
    """maps of P rays (un-batched, float32), their H x W and the ascending pixel list; acc is 0 on ~1/8 of the rays"""
    r = np.random.default_rng(600 + P + seed)
    H, W = image_size(P)
    pix = np.sort(r.choice(H * W, P, replace=False))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    acc = r.uniform(0.2, 1.0, P)
    acc[r.choice(P, max(1, P // 8), replace=False)] = 0.0
    bp = r.uniform(-0.5, 0.5, (P, 3))
    maps = O.odict(acc_map=f(acc), depth_map=f(r.uniform(0.5, 3.0, P)), norm_map=f(r.standard_normal((P, 3))), shade_map=f(r.uniform(0, 4, (P, 3))),
                   spec_map=f(r.uniform(0, 0.3, (P, 3))), albedo_map=f(r.uniform(0, 1, (P, 3)) ** 3), roughness_map=f(r.uniform(0.1, 1, P)),
                   rgb_map=f(r.uniform(0, 1, (P, 3))), bpts_map=f(bp), cpts_map=f(bp + r.normal(0, 0.01, (P, 3))))
    tb = torch.tensor([[-0.6, -0.7, -0.8], [0.7, 0.6, 0.9]])
    return maps, H, W, torch.from_numpy(pix), tb


def nan32(negative):
    return torch.tensor([0xFFC00000 - (1 << 32) if negative else 0x7FC00000], dtype=torch.int32).view(F32)[0]


def depth_variants(maps):
    """name -> (depth_map, acc_map) of the Depth edge inputs"""
    P = maps.acc_map.shape[0]
    d0, a0 = maps.depth_map, maps.acc_map
    hits = a0.nonzero()[:, 0]
    out = {}
    a = torch.zeros_like(a0)
    a[hits[:1]] = 0.7
    out['one_hit'] = (d0, a)                                                   # fewer hits than k wherever k >= 2
    out['no_hit'] = (d0, torch.zeros_like(a0))
    d = d0.clone()
    d[hits[1]], d[hits[-2]] = nan32(False), nan32(True)
    out['nans'] = (d, a0)
    d = d0.clone()
    d[hits[2]] = nan32(True)
    out['one_negative_nan'] = (d, a0)
    d = d0.clone()
    d[hits[0]] = float('inf')
    out['plus_inf'] = (d, a0)
    d = d0.clone()
    d[hits[3]] = float('-inf')
    out['minus_inf'] = (d, a0)
    out['all_equal_low'] = (torch.full_like(d0, 0.5), a0)                      # below min_clip: lo = hi, 0 / 0
    out['all_equal_high'] = (torch.full_like(d0, 2.0), a0)                     # lo is clipped to min_clip: 1 everywhere
    return out


# ------------------------------------------------------------------------------------------------ h. data movement
def blend_ground(ground, human, inds, acc, F_, C_):
    """O.blend_output_'s arithmetic for one map, float32: ground * acc + scatter(human) * (1 - acc); ground None: base 0"""
    g = torch.zeros(F_, C_) if ground is None else ground.reshape(F_, C_)
    sc = torch.zeros(F_, C_)
    if human is not None and human.shape[0] > 0:
        sc[inds] = human.reshape(-1, C_)
    ag = acc[:, None]
    return g * ag + sc * (1 - ag) if ground is not None else sc * (1 - ag)

"""The project's own restatement of the garment model that ra_cloth_create / ra_cloth_energy / ra_cloth_inertia compute
(include/relightableavatar.h), in float64 numpy with analytic gradients, the material spaces and planar patches the cloth tests share,
and the same energies in torch operations (what tools/bench_cloth.py times the kernels against).

Written from the rules (csrc/ra_cloth_rules.hpp), not from the reference's program text:
  - rest area |(c - a) x (b - a)| / 2; Dm = [m0 - m2 | m1 - m2], Dm_inv = adj(Dm) / (det + 2^-23);
  - vertex mass: the sum of density area / 3 over a vertex's faces;
  - stretch: F = [x0 - x2 | x1 - x2] Dm_inv, G = (F^T F - I) / 2, S = mu G + lambda / 2 tr(G) I, E = area thickness sum(S G);
  - bending per manifold edge: n = r / (|r| + 1e-8) with r = (p1 - p0) x (p2 - p1), e = v1 - v0, theta = atan2((e / |e|) . (n0 x n1), n0 . n1),
    E = coeff |e|^2 / (4 (area0 + area1)) theta^2 / 2;
  - gravity g mass y; inertia (d . d) mass / (2 dt^2) with d = x_next - (x_curr + dt v (+ dt^2 a)).
"""
import numpy as np

import topology_ref as T

EPS = 2.0 ** -23
FIXTURE_MESHES = ('octa', 'sphere66', 'sphere258', 'patch5', 'fin', 'two', 'fan40', 'unref')


def material(density=426 * 0.00047, thickness=0.00047, young_modulus=0.7e5, poisson_ratio=0.485, bending_multiplier=50.0, stretch_multiplier=1.0,
             material_multiplier=1.0):
    """the derived coefficients in float64: dict with A, stretch_coeff, bending_coeff, lame_mu, lame_lambda and the parameters"""
    A = young_modulus / (1.0 - poisson_ratio ** 2)
    sc = A * (stretch_multiplier * material_multiplier)
    bc = A / 12.0 * (thickness ** 3) * (bending_multiplier * material_multiplier)
    return dict(density=density, thickness=thickness, young_modulus=young_modulus, poisson_ratio=poisson_ratio, A=A, stretch_coeff=sc, bending_coeff=bc,
                lame_mu=0.5 * sc * (1.0 - poisson_ratio), lame_lambda=sc * poisson_ratio)


# ---------------------------------------------------------------------------------------------- material spaces and meshes
def flatten_faces(v, f):
    """every face flattened isometrically on its own: vm (3F,2), fm = arange(3F).reshape(F,3).  Corner 2 at the origin, corner 0 on +x."""
    v = np.asarray(v, dtype=np.float64)
    a, b = v[f[:, 0]] - v[f[:, 2]], v[f[:, 1]] - v[f[:, 2]]
    la = np.linalg.norm(a, axis=1)
    ux = a / la[:, None]
    bx = (b * ux).sum(1)
    by = np.linalg.norm(b - bx[:, None] * ux, axis=1)
    vm = np.zeros((len(f), 3, 2))
    vm[:, 0, 0] = la
    vm[:, 1, 0], vm[:, 1, 1] = bx, by
    return vm.reshape(-1, 2), np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3)


def grid_patch(nx, ny, drop=0, extra_verts=0):
    """a planar (z = 0) grid of nx x ny vertices with unit-free spacing 0.1, two triangles per cell, the last `drop` faces removed and
    `extra_verts` unused vertices appended: (verts (V,3), faces (F,3))"""
    ys, xs = np.meshgrid(np.arange(ny), np.arange(nx), indexing='ij')
    v = np.stack([0.1 * xs.ravel(), 0.1 * ys.ravel(), np.zeros(nx * ny)], axis=1).astype(np.float64)
    f = []
    for y in range(ny - 1):
        for x in range(nx - 1):
            a, b, c, d = y * nx + x, y * nx + x + 1, (y + 1) * nx + x, (y + 1) * nx + x + 1
            f += [[a, b, d], [a, d, c]]
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    if drop:
        f = f[:-drop]
    if extra_verts:
        v = np.vstack([v, np.full((extra_verts, 3), 0.5)])
    return v, f


def patch_counts(nx, ny, drop=0):
    """(F, H, V) of grid_patch(nx, ny, drop)"""
    v, f = grid_patch(nx, ny, drop)
    t = T.halfedge_build(f, len(v))
    return len(f), int((t['edge_counts'] == 2).sum()), len(v)


def perturbed(v, seed, B, amp=0.02):
    rng = np.random.default_rng(seed)
    return v[None] + rng.uniform(-amp, amp, (B,) + v.shape)


# ---------------------------------------------------------------------------------------------- the garment
def face_areas(v, f):
    return np.linalg.norm(np.cross(v[f[:, 2]] - v[f[:, 0]], v[f[:, 1]] - v[f[:, 0]]), axis=1) / v.dtype.type(2.0)


def garment(v, f, vm, fm, mat=None, topo=None, dtype=np.float64):
    """dict: f, f_area, v_mass, inv_mass, Dm, Dm_inv (F,2,2), f_connectivity (H,2), f_connectivity_edges (H,2), material.  dtype:
    the inputs are rounded to it and every array is computed in it (float32: what a float32 run starts from)"""
    v, vm = np.asarray(v, dtype=dtype), np.asarray(vm, dtype=dtype)
    mat = mat or material()
    topo = topo or T.halfedge_build(f, len(v))
    area = face_areas(v, f)
    mass = np.zeros(len(v), dtype=dtype)
    np.add.at(mass, f.reshape(-1), np.repeat((dtype(mat['density']) * area / dtype(3.0)).astype(dtype), 3))
    tm = vm[fm]
    Dm = np.stack([tm[:, 0] - tm[:, 2], tm[:, 1] - tm[:, 2]], axis=-1)
    a, b, c, d = Dm[:, 0, 0], Dm[:, 0, 1], Dm[:, 1, 0], Dm[:, 1, 1]
    det = (a * d - b * c) + dtype(EPS)
    Dm_inv = np.stack([np.stack([d, -b], -1), np.stack([-c, a], -1)], -2) / det[:, None, None]
    ev, ef = T.face_connectivity(topo)
    with np.errstate(divide='ignore'):
        inv = dtype(1.0) / mass
    return dict(f=np.asarray(f), f_area=area, v_mass=mass, inv_mass=inv, Dm=Dm, Dm_inv=Dm_inv, f_connectivity=ef, f_connectivity_edges=ev, material=mat)


# ---------------------------------------------------------------------------------------------- energies with analytic gradients
def stretch(x, g):
    """x (B,V,3) -> (energy (B,), grad (B,V,3)): per-row sums, NOT divided by B"""
    x = np.asarray(x, dtype=np.float64)
    f, m, mat = g['f'], g['Dm_inv'], g['material']
    mu, lam = mat['lame_mu'], mat['lame_lambda']
    tri = x[:, f]                                                       # B,F,3,3
    Ds = np.stack([tri[:, :, 0] - tri[:, :, 2], tri[:, :, 1] - tri[:, :, 2]], axis=-1)      # B,F,3,2
    Fm = Ds @ m[None]
    G = 0.5 * (np.swapaxes(Fm, -1, -2) @ Fm - np.eye(2))
    tr = G[..., 0, 0] + G[..., 1, 1]
    S = mu * G + 0.5 * lam * tr[..., None, None] * np.eye(2)
    k = g['f_area'][None] * mat['thickness']
    e = k * (S * G).sum((-1, -2))
    H = (2.0 * Fm @ S) @ np.swapaxes(m, -1, -2)[None] * k[..., None, None]      # B,F,3,2: d E / d Ds
    grad = np.zeros_like(x)
    for b in range(len(x)):
        np.add.at(grad[b], f[:, 0], H[b, :, :, 0])
        np.add.at(grad[b], f[:, 1], H[b, :, :, 1])
        np.add.at(grad[b], f[:, 2], -(H[b, :, :, 0] + H[b, :, :, 1]))
    return e.sum(1), grad


def _normal(p0, p1, p2):
    p, q = p1 - p0, p2 - p1
    r = np.cross(p, q)
    ln = np.linalg.norm(r, axis=-1, keepdims=True)
    d = ln + 1e-8
    return p, q, r, r / d, ln, d


def _normal_back(p, q, r, n, ln, d, gn):
    w = (gn * r).sum(-1, keepdims=True) / ln
    gr = (gn - n * w) / d
    gp, gq = np.cross(q, gr), np.cross(gr, p)
    return -gp, gp - gq, gq


def bending(x, g):
    """x (B,V,3) -> (energy (B,), grad (B,V,3)), the signed form"""
    x = np.asarray(x, dtype=np.float64)
    ef, ev, f, mat = g['f_connectivity'], g['f_connectivity_edges'], g['f'], g['material']
    grad = np.zeros_like(x)
    if len(ef) == 0:
        return np.zeros(len(x)), grad
    fa, fb = f[ef[:, 0]], f[ef[:, 1]]                                    # H,3
    A = _normal(x[:, fa[:, 0]], x[:, fa[:, 1]], x[:, fa[:, 2]])
    Bn = _normal(x[:, fb[:, 0]], x[:, fb[:, 1]], x[:, fb[:, 2]])
    n0, n1 = A[3], Bn[3]
    e = x[:, ev[:, 1]] - x[:, ev[:, 0]]
    l = np.linalg.norm(e, axis=-1, keepdims=True)
    en = e / l
    nx = np.cross(n0, n1)
    cs, sn = (n0 * n1).sum(-1), (en * nx).sum(-1)
    theta = np.arctan2(sn, cs)
    a4 = 4.0 * (g['f_area'][ef[:, 0]] + g['f_area'][ef[:, 1]])[None]
    c = mat['bending_coeff']
    scale = l[..., 0] ** 2 / a4
    energy = c * scale * theta ** 2 / 2.0
    gth = c * scale * theta
    gl = c * theta ** 2 * l[..., 0] / a4
    r2 = sn * sn + cs * cs
    gsn, gcs = (gth * cs / r2)[..., None], (-gth * sn / r2)[..., None]
    gn0 = gcs * n1 + gsn * np.cross(n1, en)
    gn1 = gcs * n0 + gsn * np.cross(en, n0)
    gen = gsn * nx
    ge = (gen - en * (gen * en).sum(-1, keepdims=True)) / l + gl[..., None] * en
    ga, gb = _normal_back(*A, gn0), _normal_back(*Bn, gn1)
    for b in range(len(x)):
        for k in range(3):
            np.add.at(grad[b], fa[:, k], ga[k][b])
            np.add.at(grad[b], fb[:, k], gb[k][b])
        np.add.at(grad[b], ev[:, 0], -ge[b])
        np.add.at(grad[b], ev[:, 1], ge[b])
    return energy.sum(1), grad


def gravity(x, mass, g=9.81):
    x = np.asarray(x, dtype=np.float64)
    grad = np.zeros_like(x)
    grad[:, :, 1] = g * mass[None]
    return (g * mass[None] * x[:, :, 1]).sum(1), grad


def inertia(x_next, x_curr, v_curr, mass, dt, accel=None):
    """-> (per-row sums (rows,), g_next, g_curr, g_vel): inertia_term, or dynamic_term with accel (3,)"""
    pred = x_curr + dt * v_curr
    if accel is not None:
        pred = pred + dt * dt * np.asarray(accel, dtype=np.float64)
    d = x_next - pred
    val = (d ** 2).sum(-1) * mass[None] / (2 * dt ** 2)
    gn = d * mass[None, :, None] / dt ** 2
    return val.sum(1), gn, -gn, -dt * gn


def sequence_parts(x, dt):
    """inertia_term_sequence's slicing of x (B,T,V,3): (x_next, x_curr, v_curr), each (B (T-1), V, 3)"""
    B, Tn, V, _ = x.shape
    xn, xc = x[:, 1:], x[:, :-1]
    vn = (xn - xc) / dt
    vc = np.concatenate([np.zeros((B, 1, V, 3), dtype=x.dtype), vn[:, :-1]], axis=1)
    return xn.reshape(-1, V, 3), xc.reshape(-1, V, 3), vc.reshape(-1, V, 3)


def finite_difference(fun, x, h=1e-6, n=24, seed=0):
    """central differences of the summed energy fun(x)[0].sum() at n random coordinates: (indices, values)"""
    rng = np.random.default_rng(seed)
    idx = [tuple(rng.integers(0, s) for s in x.shape) for _ in range(n)]
    out = []
    for i in idx:
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        out.append((fun(xp)[0].sum() - fun(xm)[0].sum()) / (2 * h))
    return idx, np.asarray(out)


# ---------------------------------------------------------------------------------------------- the same energies in torch operations
def torch_garment(g, device, dtype):
    import torch
    t = lambda a, dt=dtype: torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=dt)
    return dict(f=t(g['f'], torch.int64), ef=t(g['f_connectivity'], torch.int64), ev=t(g['f_connectivity_edges'], torch.int64), f_area=t(g['f_area']),
                Dm_inv=t(g['Dm_inv']), v_mass=t(g['v_mass']), material=g['material'])


def torch_energy(x, tg, stretch=True, bending=True, gravity=False, g=9.81):
    """x (B,V,3) tensor -> the selected energies' sum / B, in torch operations with autograd"""
    import torch
    mat, f = tg['material'], tg['f']
    total = x.new_zeros(())
    if stretch:
        tri = x[:, f]
        Ds = torch.stack([tri[:, :, 0] - tri[:, :, 2], tri[:, :, 1] - tri[:, :, 2]], dim=-1)
        Fm = Ds @ tg['Dm_inv'][None]
        G = 0.5 * (Fm.mT @ Fm - torch.eye(2, dtype=x.dtype, device=x.device))
        tr = G.diagonal(dim1=-1, dim2=-2).sum(-1)
        S = mat['lame_mu'] * G + 0.5 * mat['lame_lambda'] * tr[..., None, None] * torch.eye(2, dtype=x.dtype, device=x.device)
        total = total + (tg['f_area'][None] * mat['thickness'] * (S * G).sum((-1, -2))).sum()
    if bending and len(tg['ef']):
        def normals(fi):
            t = x[:, f[fi]]
            r = torch.cross(t[:, :, 1] - t[:, :, 0], t[:, :, 2] - t[:, :, 1], dim=-1)
            return r / (r.norm(dim=-1, keepdim=True) + 1e-8)
        n0, n1 = normals(tg['ef'][:, 0]), normals(tg['ef'][:, 1])
        e = x[:, tg['ev'][:, 1]] - x[:, tg['ev'][:, 0]]
        l = e.norm(dim=-1, keepdim=True)
        theta = torch.atan2(((e / l) * torch.cross(n0, n1, dim=-1)).sum(-1), (n0 * n1).sum(-1))
        a = (tg['f_area'][tg['ef'][:, 0]] + tg['f_area'][tg['ef'][:, 1]])[None]
        total = total + (mat['bending_coeff'] * (l[..., 0] ** 2 / (4 * a)) * theta ** 2 / 2).sum()
    if gravity:
        total = total + (g * tg['v_mass'][None] * x[:, :, 1]).sum()
    return total / x.shape[0]

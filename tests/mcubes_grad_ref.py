"""Host restatements for the marching-cubes backward tests, on top of tests/mesh_extract_ref.py.

The rule (relightableavatar_amd/csrc/ra_mcubes_grad_rules.hpp), for a crossed edge owned by grid point p along `axis`, q its other end,
a = vol[p], b = vol[q], v its vertex index:  d = b - a;  t = (iso - a) / d;  attr[v] = (1 - t) A[p] + t A[q];
gt = dverts[v][axis] + sum_c dattr[v][c] (A[q][c] - A[p][c]);  s = gt / d;  dvolume[p] += (t - 1) s;  dvolume[q] += -(t s);
dA[p] += (1 - t) dattr[v];  dA[q] += t dattr[v].  A grid point adds its own +x, +y, +z edges, then those arriving from -x, -y, -z.

Three statements of it:
    backward(..., F32) / attrs_forward(..., F32)    numpy float32 in the kernel's order of operations: what the device must equal bit for bit
    backward(..., F64) / attrs_forward(..., F64)    the same closed forms in float64
    torch_forward(...)                              plain torch at fixed topology, for autograd (float64: the truth; float32: the baseline
                                                    of the 10 x rule)
and the case table shared by the CPU and the GPU tests."""
import functools

import numpy as np
import torch

import mesh_extract_ref as R

F32, F64 = np.float32, np.float64


def topology(vol, iso):
    """the crossed edges of a float32 volume in vertex order: owning point p, axis, other end q (all linear indices)"""
    vol = np.ascontiguousarray(vol, F32)
    nx, ny, nz = vol.shape
    c = R.crossed_edges(vol, iso).reshape(-1, 3)
    p, axis = np.nonzero(c)
    q = p + np.array([ny * nz, nz, 1])[axis]
    return dict(p=p, axis=axis, q=q, n_verts=len(p), shape=vol.shape, crossed=c)


def _edges(vol, iso, topo, F):
    flat = np.asarray(vol).reshape(-1).astype(F)          # a float64 volume keeps its values under F64 (the fitting loop)
    a, b = flat[topo['p']], flat[topo['q']]
    with np.errstate(all='ignore'):
        d = b - a
        t = (F(F32(iso)) - a) / d
    return a, b, d, t, np.isfinite(a) & np.isfinite(b)


def attrs_forward(vol, iso, attrs, F=F32):
    """(n_verts, C): (1 - t) A[p] + t A[q], two products and one add"""
    topo = topology(vol, iso)
    A = np.asarray(attrs).reshape(np.asarray(vol).size, -1).astype(F)
    _, _, _, t, _ = _edges(vol, iso, topo, F)
    with np.errstate(all='ignore'):
        return ((F(1) - t)[:, None] * A[topo['p']]) + (t[:, None] * A[topo['q']])


def backward(vol, iso, dverts=None, attrs=None, dattr=None, F=F32, with_s=False):
    """(dvolume (nx,ny,nz), dattrs (n,C) or None) in the kernel's order of operations, every step one rounding of F"""
    topo = topology(vol, iso)
    p, q, axis, V = topo['p'], topo['q'], topo['axis'], topo['n_verts']
    n = int(np.prod(topo['shape']))
    a, b, d, t, live = _edges(vol, iso, topo, F)
    gt = np.zeros(V, F) if dverts is None else np.asarray(dverts).reshape(V, 3)[np.arange(V), axis].astype(F)
    dA = None
    with np.errstate(all='ignore'):
        if attrs is not None:
            A = np.asarray(attrs).reshape(n, -1).astype(F)
            g = np.asarray(dattr).reshape(V, A.shape[1]).astype(F)
            for c in range(A.shape[1]):
                gt = gt + g[:, c] * (A[q, c] - A[p, c])
            dA = np.zeros_like(A)
        s = gt / d
        ca, cb = (t - F(1)) * s, -(t * s)
        dvol = np.zeros(n, F)
        for k in range(3):              # the own edges towards +x, +y, +z: a grid point owns one edge per axis at most
            e = live & (axis == k)
            dvol[p[e]] = dvol[p[e]] + ca[e]
            if dA is not None:
                dA[p[e]] = dA[p[e]] + (F(1) - t[e])[:, None] * g[e]
        for k in range(3):              # then the edges arriving from -x, -y, -z
            e = live & (axis == k)
            dvol[q[e]] = dvol[q[e]] + cb[e]
            if dA is not None:
                dA[q[e]] = dA[q[e]] + t[e][:, None] * g[e]
    dvol = dvol.reshape(topo['shape'])
    return (dvol, dA, np.where(live, s, 0)) if with_s else (dvol, dA)


def torch_forward(vol, iso, topo, attrs=None):
    """(verts (V,3) in index coordinates, vattrs (V,C) or None) as plain torch in vol's dtype, the topology held fixed"""
    flat = vol.reshape(-1)
    p, q, axis = (torch.as_tensor(topo[k]) for k in ('p', 'q', 'axis'))
    a, b = flat[p], flat[q]
    t = (iso - a) / (b - a)
    base = torch.from_numpy(np.stack(np.unravel_index(topo['p'], topo['shape']), 1)).to(vol.dtype)
    verts = base + torch.nn.functional.one_hot(axis, 3).to(vol.dtype) * t[:, None]
    if attrs is None:
        return verts, None
    A = attrs.reshape(flat.numel(), -1)
    return verts, (1 - t)[:, None] * A[p] + t[:, None] * A[q]


def autograd(vol, iso, dverts=None, attrs=None, dattr=None, dtype=torch.float64):
    """(dvolume, dattrs or None, vattrs or None) by torch autograd through torch_forward; non-finite ends are not supported here"""
    topo = topology(vol, iso)
    v = torch.from_numpy(np.ascontiguousarray(vol, F32)).to(dtype).requires_grad_()
    A = None if attrs is None else torch.from_numpy(np.ascontiguousarray(attrs, F32)).to(dtype).reshape(v.numel(), -1).requires_grad_()
    verts, va = torch_forward(v, float(F32(iso)), topo, A)
    loss = verts.sum() * 0
    if dverts is not None:
        loss = loss + (verts * torch.from_numpy(np.asarray(dverts, F32)).to(dtype)).sum()
    if A is not None:
        loss = loss + (va * torch.from_numpy(np.asarray(dattr, F32)).to(dtype)).sum()
    loss.backward()
    return v.grad.numpy(), None if A is None else A.grad.numpy(), None if A is None else va.detach().numpy()


# ---------------------------------------------------------------------------------------------- the cases
def edge_sized_volume(shape, seed):
    """a smooth blob plus noise, with a border of outside: crossings in every part of an oddly sized grid"""
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing='ij'), -1)
    vol = (0.8 - np.linalg.norm(g, axis=-1) + 0.3 * np.random.default_rng(seed).uniform(-1, 1, shape)).astype(F32)
    for ax in range(3):
        idx = [slice(None)] * 3
        for side in (0, -1):
            idx[ax] = side
            vol[tuple(idx)] = R.OUTSIDE
    return vol


@functools.lru_cache(None)
def volume(name):
    """(volume, iso): the volumes of tests/test_gpu_mesh_extract.py, rebuilt"""
    if name == 'patterns':
        return R.all_patterns_volume(), 0.0
    if name == 'sphere':
        return R.sphere_volume(), 0.0
    if name == 'torus':
        return R.torus_volume(), 0.0
    if name == 'random':                # interior grid points have all six edges crossed now and then
        return R.random_volume(), 0.0
    if name == 'exact_iso':
        return R.exact_iso_volume(), 0.0
    if name == '33x17x65':              # more points than one workgroup's, no axis a multiple of 64
        return edge_sized_volume((33, 17, 65), 1), 0.05
    if name == '2x2x2':
        return R.pattern_volume(0b10010110)[1:3, 1:3, 1:3].copy(), 0.0
    if name == '2x3x65':
        return np.random.default_rng(2).uniform(-1, 1, (2, 3, 65)).astype(F32), 0.1
    if name == 'last_cell':
        return R.last_cell_volume(), 0.0
    if name == 'all_outside':
        return np.full((3, 4, 5), R.OUTSIDE, F32), 0.0
    raise KeyError(name)


VOLUMES = ('patterns', 'sphere', 'random', 'exact_iso', '33x17x65', '2x2x2', '2x3x65', 'last_cell', 'all_outside')
CPU_VOLUMES = ('random', 'sphere', 'torus', 'exact_iso', 'patterns', 'last_cell')
CHANNELS = (0, 1, 3, 4, 5, 64)


@functools.lru_cache(None)
def case(name, C):
    """dict(vol, iso, dverts, attrs (n,C) or None, dattr or None, n_verts): the inputs of one backward, seeded by the name"""
    vol, iso = volume(name)
    topo = topology(vol, iso)
    rng = np.random.default_rng(sum(map(ord, name)) * 100 + C)
    V = topo['n_verts']
    out = dict(vol=vol, iso=iso, n_verts=V, dverts=rng.standard_normal((V, 3)).astype(F32), attrs=None, dattr=None, topo=topo)
    if C:
        out['attrs'] = rng.uniform(-1, 1, (vol.size, C)).astype(F32)
        out['dattr'] = rng.standard_normal((V, C)).astype(F32)
    return out


@functools.lru_cache(None)
def reference(name, C, F=F32):
    """(dvolume, dattrs, vattrs) of a case in F: computed once, shared, never written to"""
    c = case(name, C)
    dvol, dA = backward(c['vol'], c['iso'], c['dverts'], c['attrs'], c['dattr'], F)
    va = attrs_forward(c['vol'], c['iso'], c['attrs'], F) if C else None
    for x in (dvol, dA, va):
        if x is not None:
            x.setflags(write=False)
    return dvol, dA, va


def nonfinite_volume():
    """the random volume with a NaN, +inf and -inf at interior points whose neighbours cross"""
    vol = R.random_volume().copy()
    vol[3, 4, 5], vol[5, 5, 5], vol[4, 6, 3] = np.nan, np.inf, -np.inf
    return vol, 0.0, [(3, 4, 5), (5, 5, 5), (4, 6, 3)]


# ---------------------------------------------------------------------------------------------- end to end (a): the radius fit
RADIUS_FIT = dict(target=6.0, steps=40, lr=0.05)


def radius_loss_grad(verts, centre, target):
    """mean((|v - c| - target)^2) and its gradient in the vertices, float64"""
    diff = np.asarray(verts, F64) - np.asarray(centre, F64)
    r = np.linalg.norm(diff, axis=1)
    return float(np.mean((r - target) ** 2)), (2.0 * (r - target) / (r * len(r)))[:, None] * diff


def radius_fit_reference():
    """plain gradient steps on the sphere volume with the float64 restatement: the losses before every step and after the last.  The loss
    reported is the mean; a step is lr times the gradient of the SUM over the vertices (the mean's times the vertex count), so that a
    vertex moves by the same amount whatever the mesh's size: 3.9797 -> 0.4295 in 40 steps, a factor of 9.27"""
    vol = R.sphere_volume().astype(F64)
    losses = []
    for _ in range(RADIUS_FIT['steps'] + 1):
        verts = torch_forward(torch.from_numpy(vol), 0.0, topology(vol, 0.0))[0].numpy()
        loss, g = radius_loss_grad(verts, R.SPHERE['centre'], RADIUS_FIT['target'])
        losses.append(loss)
        vol = vol - RADIUS_FIT['lr'] * len(verts) * backward(vol, 0.0, g, F=F64)[0]
    return losses


# ---------------------------------------------------------------------------------------------- the two rules of differentiable_marching_cubes
def normal_rule_grads(decoder, params, verts, g):
    """the reference's RegisterSDFGradient (lib/utils/mesh_utils.py:70-91) restated: d / d params of sum(-(n . g) sdf(verts)) with
    n = normalize(d sdf / d x) held constant"""
    x = verts.detach().clone().requires_grad_()
    sdf = decoder(x).reshape(-1)
    n = torch.nn.functional.normalize(torch.autograd.grad(sdf.sum(), x, retain_graph=True)[0], dim=-1).detach()
    return torch.autograd.grad((-(n * g).sum(-1) * sdf).sum(), params, allow_unused=True)


def grid_rule_grads(decoder, params, points, dvolume):
    """the exact gradient of the computed vertices: dvolume (of volume = -sdf) pushed through the decoder on the grid"""
    sdf = decoder(points.reshape(-1, 3)).reshape(-1)
    return torch.autograd.grad((-torch.as_tensor(dvolume, dtype=sdf.dtype).reshape(-1) * sdf).sum(), params, allow_unused=True)

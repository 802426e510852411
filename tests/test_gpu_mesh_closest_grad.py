"""ra_mesh_closest_backward, Mesh.closest_backward and the differentiable distances of mesh_utils on the device.
Run with `-m gpu` on an MI355X.

Bit equality is the main check: dpts, dverts and dattr equal the float32 restatement (tests/mesh_closest_grad_ref.py: backward32) fed
the kernel's own forward outputs, two calls agree, forwards taken default and RA_MESH_BRUTE give the same gradients, any subset of the
outputs gives the same bits, and dpts' rows keep their bits under any permutation or prefix of the rows (NOT dverts: the order of the rows
is the order of summation).  Parity is the project's 10 x float32 rule (frame_stage_ref.parity's statistics): the kernel's error against
the float64 closed form evaluated at the KERNEL's returned faces (ties differ legitimately from the float64 argmin) may be at most 10 x
the error of the float32 restatement on its own numpy forward against the closed form at its own faces (never below one rounding).  On a
face of no area the barycentrics are not unique, so there the float64 closed form takes the returned ones (mesh_closest_grad_ref.flat_faces).
Every test prints its figures before it asserts."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import mesh_closest_grad_ref as G
import mesh_distance_ref as M
import test_gpu_mesh_distance as D
from frame_stage_ref import parity
from relightableavatar_amd import _lib, mesh_utils
from relightableavatar_amd._lib import RaError
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.evaluators import mesh_evaluator

pytestmark = pytest.mark.gpu
U = 2.0 ** -23
KEYS = ('dpts', 'dverts', 'dattr')
TRI_N = (0, 1, 63, 64, 65, 257)


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from relightableavatar_amd.engine import Engine
    return Engine(make_cfg('relight'), device='cuda:0')          # any context will do: no weights are read


def T(a, dev='cuda:0'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(None)
def case(name):
    """(verts, faces, points): one triangle with n points around it (three runs of n slots), 33 faces of the hull, and the mesh-distance
    tests' hull, two-copies and degenerate meshes with their near sets"""
    if name.startswith('tri_'):
        n = int(name[4:])
        rng = np.random.default_rng(100 + n)
        v = np.float32([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.3]])
        w = rng.uniform(-0.4, 1.2, (n, 3))                      # affine weights past the edges: face, edge and vertex regions
        w /= w.sum(1, keepdims=True)
        p = w @ v.astype(np.float64) + 0.1 * rng.standard_normal((n, 3))
        return v, np.array([[0, 1, 2]]), p.astype(np.float32)
    if name == 'f33':
        v, f = D.hull()
        f = f[:33]
        rng = np.random.default_rng(33)
        tri = v.astype(np.float64)[f]
        p = np.repeat(tri.mean(1), 4, axis=0) + 0.03 * rng.standard_normal((4 * len(f), 3))
        return v, f, p.astype(np.float32)
    v, f = D.mesh_case(name)
    return v, f, D.point_sets(name)['near']


@functools.lru_cache(None)
def upstream(name, Cn):
    n = len(case(name)[2])
    rng = np.random.default_rng(7 + Cn)
    return rng.standard_normal(n).astype(np.float32), rng.standard_normal((n, Cn)).astype(np.float32)


@functools.lru_cache(None)
def float32_floor(name, Cn):
    """the error of the float32 restatement on its own numpy forward against the float64 closed form at its own faces, per output:
    (|error| array, max |reference|)"""
    v, f, p = case(name)
    g, ga = upstream(name, Cn)
    _, q, face, bary = M.closest_point(p, v, f, np.float32)
    r32, r64 = G.backward32(p, q, face, bary, f, len(v), g, ga), G.backward64(p, v, f, face, g, ga, flat_bary=bary)
    return {k: np.abs(r32[k].astype(np.float64) - r64[k]) for k in KEYS}


def ten_times_rule(label, got, ref64, e32):
    """frame_stage_ref.parity's rule with the float32 error given: max and median |got - ref64| normalised by max |ref64| may be at most
    10 x the float32 restatement's own, and that is never taken below one rounding, 2^-23 of max |ref64| (tests/test_gpu_fit.py's
    10 x max(error, eps): a float32 result is not held closer than its format, however lucky the few values of the restatement —
    three per channel on a single triangle — happen to be)"""
    if got.size == 0:
        print(f'{label}: no element to compare')
        return
    assert np.isfinite(ref64).all() and np.isfinite(got).all(), f'{label}: non-finite values'
    scale = max(float(np.abs(ref64).max()), 1e-30)
    ek, e32 = np.abs(got.astype(np.float64) - ref64) / scale, e32 / scale
    for name, fn in (('max', np.max), ('median', np.median)):
        k, f = float(fn(ek)), float(fn(e32))
        print(f'{label}: {name} kernel {k:.3e}  float32 {f:.3e}  ratio {k / max(f, U):.2f}' + ('' if f >= U else ' (of one rounding: the float32 error is below it)'))
        assert k <= 10 * max(f, U), f'{label}: {name} |kernel - float64| {k:.3e} > 10 x float32 restatement {f:.3e}'


def same_bits(tag, a, b, keys=KEYS):
    for k in keys:
        x, y = a[k], b[k]
        x, y = (x if torch.is_tensor(x) else T(x)), (y if torch.is_tensor(y) else T(y))
        same = x.shape == y.shape and bool(torch.equal(x.contiguous().view(torch.int32).cpu(), y.contiguous().view(torch.int32).cpu()))
        print(f'{tag}: {k} bit-equal {same} ({tuple(x.shape)})')
        assert same, f'{tag}: {k}'


def restate(out, v, f, p, g, ga):
    return G.backward32(p, N(out.closest), N(out.face), N(out.bary), f, len(v), g, ga)


# ------------------------------------------------------------------------------------------------ bits and parity
CASES = [(f'tri_{n}', 3) for n in TRI_N] + [('f33', 3), ('hull', 3), ('two', 3), ('degenerate', 3)] + \
        [(name, Cn) for name in ('tri_65', 'hull') for Cn in (0, 1, 64)]


@pytest.mark.parametrize('name,Cn', CASES)
def test_bits_and_parity(eng, name, Cn):
    v, f, p = case(name)
    g, ga = upstream(name, Cn)
    n = len(p)
    mesh = eng.mesh(T(v), T(f))
    tp, tg, tga = T(p), T(g), T(ga)
    out = mesh.closest(tp)
    r = mesh.closest_backward(tp, out, tg, tga)
    assert r.dpts.shape == (n, 3) and r.dverts.shape == (len(v), 3) and r.dattr.shape == (len(v), Cn)
    slots = np.bincount(f[N(out.face)[N(out.face) >= 0]].reshape(-1), minlength=len(v)) if n else np.zeros(len(v), int)
    print(f'{name} C {Cn}: {n} rows, {len(v)} vertices, slots per vertex {slots.min()} .. {slots.max()}, {int((slots == 0).sum())} vertices without one')
    same_bits(f'{name} C {Cn}: kernel = float32 restatement on the kernel\'s forward', r, restate(out, v, f, p, g, ga))
    same_bits(f'{name}: second call', r, mesh.closest_backward(tp, out, tg, tga))
    same_bits(f'{name}: forward taken RA_MESH_BRUTE', r, mesh.closest_backward(tp, mesh.closest(tp, brute=True), tg, tga))
    for k in range(1, 3):
        for want in itertools.combinations(KEYS, k):
            sub = mesh.closest_backward(tp, out, tg if set(want) & {'dpts', 'dverts'} else None, tga if 'dattr' in want else None, want=want)
            assert tuple(sub.keys()) == want
            same_bits(f'{name}: want = {want}', r, sub, keys=want)
    if n > 1:
        perm = np.random.default_rng(1).permutation(n)
        tperm = T(perm)
        pick = lambda rows: type(out)(closest=out.closest[rows], face=out.face[rows], bary=out.bary[rows])
        rp = mesh.closest_backward(tp[tperm], pick(tperm), tg[tperm], want=('dpts',))
        same_bits(f'{name}: dpts rows under a permutation', dict(dpts=r.dpts[tperm]), rp, keys=('dpts',))
        half = slice(0, n // 2)
        rh = mesh.closest_backward(tp[half], pick(half), tg[half], want=('dpts',))
        same_bits(f'{name}: dpts rows of a prefix', dict(dpts=r.dpts[half]), rh, keys=('dpts',))
    assert int(G.flat_faces(v, f).sum()) == (2 if name == 'degenerate' else 0), 'only the degenerate mesh has faces of no area'
    if n:
        # the closed form at the KERNEL's faces; on a face of no area float64 has no barycentrics of its own (G.flat_faces): the kernel's
        r64 = G.backward64(p, v, f, N(out.face), g, ga, flat_bary=N(out.bary))
        floor = float32_floor(name, Cn)
        for k in KEYS:
            ten_times_rule(f'{name} C {Cn} {k}', N(r[k]), r64[k], floor[k])
    mesh.close()


# ------------------------------------------------------------------------------------------------ dead rows and bad values
@pytest.mark.parametrize('n', [64, 130])
def test_dead_rows_and_non_finite_values_stay_where_they_are(eng, n):
    v, f = D.hull()
    p = G.generic_points()[:n].copy()
    rng = np.random.default_rng(n)
    g, ga = rng.standard_normal(n).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    mesh = eng.mesh(T(v), T(f))
    clean_out = mesh.closest(T(p))
    clean = mesh.closest_backward(T(p), clean_out, T(g), T(ga))
    bad = p.copy()
    bad[17] = [np.nan, 0.1, 0.2]
    bad[40, 2] = np.inf
    bad[41] = -np.inf
    rows, others = [17, 40, 41], np.setdiff1d(np.arange(n), [17, 40, 41])
    out = mesh.closest(T(bad))
    r = mesh.closest_backward(T(bad), out, T(g), T(ga))
    print(f'n = {n}: faces of the non-finite points {out.face[rows].tolist()}, their dpts {N(r.dpts[rows]).tolist()}')
    assert out.face[rows].tolist() == [-1, -1, -1] and not N(r.dpts[rows]).view(np.uint32).any()
    same_bits(f'n = {n}: dpts of the finite rows beside dead rows', dict(dpts=clean.dpts[T(others)]), dict(dpts=r.dpts[T(others)]), keys=('dpts',))
    same_bits(f'n = {n}: with dead rows, kernel = restatement', r, restate(out, v, f, bad, g, ga))
    assert bool(torch.isfinite(r.dverts).all()) and bool(torch.isfinite(r.dattr).all())
    # a NaN upstream gradient reaches its own row and its three vertices only
    gn = g.copy()
    gn[5] = np.nan
    rn = mesh.closest_backward(T(p), clean_out, T(gn), T(ga))
    hit = f[int(clean_out.face[5])]
    rest_v, rest_r = np.setdiff1d(np.arange(len(v)), hit), np.setdiff1d(np.arange(n), [5])
    print(f'n = {n}: NaN g in row 5 (face {int(clean_out.face[5])}, vertices {hit.tolist()}): dpts[5] {N(rn.dpts[5]).tolist()}, dverts there {N(rn.dverts[T(hit)]).tolist()}')
    assert bool(torch.isnan(rn.dpts[5]).all()) and bool(torch.isnan(rn.dverts[T(hit)]).all())
    same_bits(f'n = {n}: NaN g, every other row and vertex', dict(dpts=clean.dpts[T(rest_r)], dverts=clean.dverts[T(rest_v)], dattr=clean.dattr),
              dict(dpts=rn.dpts[T(rest_r)], dverts=rn.dverts[T(rest_v)], dattr=rn.dattr))
    # every row dead: zeros
    dead = np.full_like(p, np.nan)
    out = mesh.closest(T(dead))
    r0 = mesh.closest_backward(T(dead), out, T(g), T(ga))
    assert all(not N(r0[k]).view(np.uint32).any() for k in KEYS)
    mesh.close()


# ------------------------------------------------------------------------------------------------ autograd
def _torch_distance_loss(p, v, f, face, bary, w, dtype):
    """sum w |p - sum_k b_k v[f[face][k]]| in torch, the face and the barycentrics given: gather by the returned face, index_add_ backwards"""
    p, v, b, w = (torch.as_tensor(a).to(dtype) for a in (p, v, bary, w))
    v.requires_grad_()
    q = (v[torch.as_tensor(f).long()[torch.as_tensor(face).long()]] * b[..., None]).sum(1)
    (w * (p - q).norm(dim=-1)).sum().backward()
    return v.grad.numpy()


def test_autograd_reaches_verts_and_values(eng):
    v, f = D.hull()
    p = G.generic_points()
    n = len(p)
    rng = np.random.default_rng(23)
    w, W = rng.uniform(0.5, 1.5, n).astype(np.float32), rng.standard_normal((n, 5)).astype(np.float32)
    vals = rng.standard_normal((len(v), 5)).astype(np.float32)
    tp, tv, tf, tw = T(p), T(v), T(f), T(w)
    # the engine call the autograd functions must equal, bit for bit
    mesh = eng.mesh(tv, tf)
    out = mesh.closest(tp)
    d = out.d2.sqrt()
    g_d2 = torch.where(d > 0, tw / (2 * d), torch.zeros_like(d))
    want = mesh.closest_backward(tp, out, g_d2, T(W))
    mesh.close()
    grads = {}
    # point_mesh_distance
    vv, pp = tv.clone().requires_grad_(), tp.clone().requires_grad_()
    dist, face = mesh_utils.point_mesh_distance(pp, vv, tf, engine=eng)
    (tw * dist).sum().backward()
    assert face.dtype == torch.int64 and torch.equal(face, out.face.long()) and torch.equal(dist.detach(), d)
    assert vv.grad is not None and pp.grad is not None
    grads['point_mesh_distance'] = vv.grad
    same_bits('point_mesh_distance: verts.grad / points.grad = the engine call', dict(dverts=vv.grad, dpts=pp.grad), want, keys=('dverts', 'dpts'))
    # bvh_distance, its own mesh and a given one
    for given in (False, True):
        vv = tv.clone().requires_grad_()
        m = eng.mesh(tv, tf) if given else None
        dist = mesh_utils.bvh_distance(tp, vv, tf, engine=eng, mesh=m)
        (tw * dist).sum().backward()
        assert torch.equal(dist.detach(), d) and vv.grad is not None
        same_bits(f'bvh_distance (mesh given: {given}): verts.grad = the engine call', dict(dverts=vv.grad), want, keys=('dverts',))
        if given:
            m.close()
    # sample_closest_points_on_surface: verts through the distance, values through the interpolation
    vv, va = tv.clone().requires_grad_(), T(vals).requires_grad_()
    interp, dist = mesh_utils.sample_closest_points_on_surface(tp[None], vv[None], tf[None], va[None], engine=eng)
    ((tw * dist.view(-1)).sum() + (T(W) * interp[0]).sum()).backward()
    assert vv.grad is not None and va.grad is not None
    same_bits('sample_closest_points_on_surface: verts.grad, values.grad = the engine call', dict(dverts=vv.grad, dattr=va.grad), want, keys=('dverts', 'dattr'))
    # winding_distance: the distance factor carries the gradient to verts
    vv = tv.clone().requires_grad_()
    mesh_utils.winding_distance(tp, vv, tf, engine=eng).sum().backward()
    assert vv.grad is not None and bool(torch.isfinite(vv.grad).all()) and float(vv.grad.abs().max()) > 0
    # without requires_grad: today's calls, today's bits — also as the forward of the calls above
    plain = mesh_utils.bvh_distance(tp, tv, tf, engine=eng)
    i0, d0 = mesh_utils.sample_closest_points_on_surface(tp[None], tv[None], tf[None], T(vals)[None], engine=eng)
    today = (T(vals)[tf.long()[out.face.long().clamp_min(0)]] * out.bary[..., None]).sum(1)
    assert not plain.requires_grad and torch.equal(plain, d) and torch.equal(d0.view(-1), d) and torch.equal(i0[0], today) and torch.equal(interp[0].detach(), today)
    # the float64 torch expression of the same loss at the returned faces, under the 10 x rule
    face_np, bary_np = N(out.face), N(out.bary)
    g64 = _torch_distance_loss(p, v, f, face_np, bary_np, w, torch.float64)
    g32 = _torch_distance_loss(p, v, f, face_np, bary_np, w, torch.float32)
    parity('verts.grad of sum w d against torch float64 (gather by the returned face, index_add_)', N(grads['point_mesh_distance']), g32, g64)
    a64 = np.zeros((len(v), 5))
    for k in range(3):
        np.add.at(a64, f[face_np, k], bary_np[:, k, None].astype(np.float64) * W)
    a32 = N(torch.zeros(len(v), 5).index_add_(0, torch.as_tensor(f[face_np]).reshape(-1), (torch.as_tensor(bary_np)[..., None] * torch.as_tensor(W)[:, None]).reshape(-1, 5)))
    parity('values.grad against float64 (index_add_ of b_k W)', N(va.grad), a32, a64)


def test_losses_are_the_evaluators_arithmetic(eng):
    v, f = D.hull()
    dv, _ = D.displaced_hull()
    gen = torch.Generator().manual_seed(3)
    tgt_pts, _ = mesh_utils.sample_surface(torch.from_numpy(v), torch.from_numpy(f), 500, gen)
    src_pts, src_face = mesh_utils.sample_surface(torch.from_numpy(dv), torch.from_numpy(f), 400, gen)
    tri = torch.from_numpy(dv)[torch.from_numpy(f)[src_face]].double()
    bary = torch.linalg.solve(tri.mT, src_pts.double()[..., None])[..., 0].float()       # the samples' barycentrics in their faces
    moving = T(dv).requires_grad_()
    src, tgt = eng.mesh(T(dv), T(f)), eng.mesh(T(v), T(f))
    p2s = mesh_utils.point_to_surface_loss(moving, T(f), tgt_pts.cuda(), engine=eng)
    assert p2s.dtype == torch.float64 and torch.equal(p2s.detach(), mesh_evaluator.mean_distance(src, tgt_pts.cuda()))
    sq = mesh_utils.point_to_surface_loss(moving, T(f), tgt_pts.cuda(), squared=True, engine=eng)
    assert torch.equal(sq.detach(), src.closest(tgt_pts.cuda(), want=('d2',)).d2.double().mean())
    ch = mesh_utils.chamfer_loss(moving, T(f), T(v), T(f), (src_face, bary), tgt_pts.cuda(), engine=eng)
    moved = (T(dv)[T(f).long()[src_face.cuda()]] * bary.cuda()[..., None]).sum(1)
    ref = mesh_evaluator.chamfer_and_p2s(src, tgt, moved, tgt_pts.cuda(), moved)[0]
    print(f'p2s {float(p2s.detach()):.6e}, squared {float(sq.detach()):.6e}, chamfer {float(ch.detach()):.6e} (evaluator {float(ref):.6e})')
    assert torch.equal(ch.detach(), ref)
    (ga,) = torch.autograd.grad(ch, moving)
    (gb,) = torch.autograd.grad(mesh_utils.chamfer_loss(moving, T(f), T(v), T(f), (src_face, bary), tgt_pts.cuda(), engine=eng), moving)
    assert torch.equal(ga, gb) and bool(torch.isfinite(ga).all()) and float(ga.abs().max()) > 0
    # one small step against the gradient lowers the loss (a condition, not a measure)
    stepped = (moving - 1e-3 * ga / ga.abs().max()).detach()
    after = mesh_utils.chamfer_loss(stepped, T(f), T(v), T(f), (src_face, bary), tgt_pts.cuda(), engine=eng)
    print(f'chamfer after a 1 mm step against its gradient: {float(after):.6e}')
    assert float(after) < float(ch.detach())
    src.close(), tgt.close()


# ------------------------------------------------------------------------------------------------ fitting
FIT_POINTS, FIT_ITERS, FIT_LR = 300, 8, 3e-4      # 8 steps x 0.3 mm at most per coordinate against a displacement of 3 mm: no overshoot


@functools.lru_cache(None)
def fit_inputs():
    v, f = D.hull()
    dv, _ = D.displaced_hull()
    pts, _ = mesh_utils.sample_surface(torch.from_numpy(v), torch.from_numpy(f), FIT_POINTS, torch.Generator().manual_seed(5))
    return dv, f, pts.numpy()


@functools.lru_cache(None)
def fit_truth():
    dv, f, pts = fit_inputs()
    w64 = G.fit(dv, f, pts, 29, FIT_ITERS, FIT_LR)
    w32 = G.fit(dv, f, pts, 29, FIT_ITERS, FIT_LR, dtype=np.float32)
    return w64, w32


def test_point_cloud_fitting(eng):
    dv, f, pts = fit_inputs()
    before = float(mesh_utils.point_to_surface_loss(T(dv), T(f), T(pts), engine=eng))
    runs = [mesh_utils.point_cloud_fitting(T(dv), T(f), T(pts), 29, FIT_ITERS, None, FIT_LR, engine=eng) for _ in range(2)]
    got = runs[0]
    after = float(mesh_utils.point_to_surface_loss(got, T(f), T(pts), engine=eng))
    chunked = [mesh_utils.point_cloud_fitting(T(dv), T(f), T(pts), 29, 4, 300, FIT_LR, generator=torch.Generator().manual_seed(9), engine=eng) for _ in range(2)]
    (w64, l64), (w32, l32) = fit_truth()
    loss_dev, loss64, loss32 = G.mean_d2(pts, N(got), f), G.mean_d2(pts, w64, f), G.mean_d2(pts, w32, f)
    start = G.mean_d2(pts, dv, f)
    floor = max(abs(loss32 - loss64), U * loss64)
    print(f'point-to-surface loss {before:.6e} -> {after:.6e}; mean d2 {start:.6e} -> device {loss_dev:.9e}, float64 loop {loss64:.9e}, float32 loop {loss32:.9e}; '
          f'|device - float64| {abs(loss_dev - loss64):.3e}, |float32 - float64| {abs(loss32 - loss64):.3e} (ratio {abs(loss_dev - loss64) / floor:.2f}); '
          f'the float64 loop\'s losses {l64[0]:.6e} -> {l64[-1]:.6e}')
    assert got.shape == (len(dv), 3) and got.dtype == torch.float32 and got.is_cuda
    assert after < before
    assert torch.equal(runs[0], runs[1]) and torch.equal(chunked[0], chunked[1])
    assert abs(loss_dev - loss64) <= 10 * floor


# ------------------------------------------------------------------------------------------------ errors and memory
def test_argument_errors(eng):
    v, f, p = case('hull')
    mesh = eng.mesh(T(v), T(f))
    tp = T(p[:8])
    out = mesh.closest(tp)
    g, ga = torch.ones(8, device='cuda:0'), torch.ones(8, 3, device='cuda:0')
    dp, dv, da = torch.empty(8, 3, device='cuda:0'), torch.empty(len(v), 3, device='cuda:0'), torch.empty(len(v), 3, device='cuda:0')
    L, P = eng.lib, lambda t: None if t is None else C.c_void_p(t.data_ptr())
    fd = mesh.faces_device()

    def call(F=len(f), V=len(v), n=8, g=g, ga=ga, Cn=3, outs=(dp, dv, da)):
        rc = L.ra_mesh_closest_backward(eng.ctx, P(fd), F, V, P(tp), P(out.closest), P(out.face), P(out.bary), n, P(g), P(ga), Cn, *[P(o) for o in outs], eng.stream)
        return rc, L.ra_last_error()

    assert call()[0] == 0
    for kw in (dict(n=-1), dict(n=1 << 30), dict(V=0), dict(F=0), dict(F=(1 << 24) + 1), dict(Cn=-1), dict(Cn=65)):
        rc, msg = call(**kw)
        print(kw, rc, msg)
        assert rc == 1 and b'bad sizes' in msg, kw
    for kw in (dict(outs=(None, None, None)), dict(g=None), dict(g=None, outs=(dp, None, None)), dict(g=None, outs=(None, dv, None)), dict(ga=None),
               dict(ga=None, outs=(None, None, da))):
        rc, msg = call(**kw)
        print({k: (v if not isinstance(v, tuple) else [o is not None for o in v]) for k, v in kw.items()}, rc, msg)
        assert rc == 1 and b'null argument' in msg, kw
    assert call(g=None, outs=(None, None, da))[0] == 0 and call(ga=None, outs=(dp, dv, None))[0] == 0       # each output needs its own upstream gradient only
    # n == 0: zeros in the vertex-sized outputs, no row pointer read
    dv.fill_(7.0), da.fill_(7.0)
    rc = L.ra_mesh_closest_backward(eng.ctx, P(fd), len(f), len(v), None, None, None, None, 0, None, None, 3, None, P(dv), P(da), eng.stream)
    assert rc == 0 and not N(dv).view(np.uint32).any() and not N(da).view(np.uint32).any()
    with pytest.raises(ValueError, match='want'):
        mesh.closest_backward(tp, out, g, ga, want=('dpts', 'dfaces'))
    mesh.close()
    with pytest.raises(RaError, match='closed'):
        mesh.closest_backward(tp, out, g, ga)
    torch.cuda.synchronize()


def test_a_hundred_calls_leave_free_memory_where_the_first_left_it(eng):
    v, f, p = case('hull')
    mesh = eng.mesh(T(v), T(f))
    tp = T(p)
    g, ga = torch.ones(len(p), device='cuda:0'), torch.ones(len(p), 3, device='cuda:0')
    out = mesh.closest(tp)
    keep = mesh.closest_backward(tp, out, g, ga)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(100):
        r = mesh.closest_backward(tp, out, g, ga)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print(f'free memory: {free0} after the first backward, {free1} after 100 more')
    assert free1 >= free0
    same_bits('the 101st call', keep, r)
    mesh.close()

"""ra_mesh_winding_grad, Mesh.winding_grad, the autograd of mesh_utils' winding and distance functions and isosurface_fitting on the
device.  Run with `-m gpu` on an MI355X.

No tolerance is chosen here.  The gradient is held to the project's 10 x float32 rule (frame_stage_ref.parity, relative to max |g| of
the case): max and median |kernel - float64 oracle| are at most 10 x the error of the float32 restatement of the kernel's operations
on the same inputs (tests/winding_grad_ref.py; the oracle is pinned to the reference's float64 autograd by
tests/test_oracle_winding_grad.py).  The reference's own float32 autograd is printed beside, not used as a ceiling: it is off by up
to several times max |g|.  Exactness is bit equality: the value is Mesh.winding's, and a row does not depend on n, on the order or the
subset of the points, or on the launch shape.  Every test prints its figures before it asserts.

isosurface_fitting (30 iterations, the hull scaled by 1.15 onto the opened hull, sum of squares over all 301 vertices; figures of the
run that DESIGN.md section 24 records): f = winding_number at 0.5: loss 75.506958 -> 75.442108 (outside a hull the winding number is all but flat: only the vertices near
the hole move); f = winding_distance at 0: 0.851211 -> 0.704670."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import fit_ref as FR
import mesh_distance_ref as M
import winding_grad_ref as G
import winding_ref as W
from frame_stage_ref import parity
from relightableavatar_amd import largesteps, mesh_utils
from relightableavatar_amd._lib import RaError
from relightableavatar_amd.config import make_cfg

pytestmark = pytest.mark.gpu
STRIDE = {'near': 1, 'grid': 5}
F32 = np.float32


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from relightableavatar_amd.engine import Engine
    return Engine(make_cfg('relight'), device='cuda:0')          # any context will do: no weights are read


@functools.lru_cache(None)
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'winding_grad.npz'))


def points(name, group):
    return W.point_sets(name)[group][::STRIDE[group]]


@functools.lru_cache(None)
def large():
    """test_gpu_winding.large(): the hull at 10 001 vertices (19 998 faces) and points 1 cm inside and outside it; here the 129 in the
    middle of its 256: 65 outside, 64 inside"""
    v, f = W.hull(10001)
    tri = v.astype(np.float64)[f[::157][:128]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    p = np.concatenate([tri.mean(1) + 1e-2 * nrm, tri.mean(1) - 1e-2 * nrm]).astype(np.float32)
    return v, f, np.ascontiguousarray(p[63:192])


@functools.lru_cache(None)
def large_refs(n_faces):
    v, f, p = large()
    return G.winding_grad(p, v, f[:n_faces])[1], G.winding_grad_kernel32(p, v, f[:n_faces])[1]


def T(a, dev='cuda:0'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same_bits(tag, a, b):
    same = bool(torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu()))
    print(f'{tag}: bit-equal {same} ({a.numel()} values)')
    assert same, tag


def same_rows(tag, got, want):
    same_bits(f'{tag}: winding', got[0], want[0])
    same_bits(f'{tag}: gradient', got[1], want[1])


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('group', W.SETS)
@pytest.mark.parametrize('name', W.MESHES)
def test_parity(eng, name, group):
    v, f = W.mesh_case(name)
    p = points(name, group)
    r64, r32 = G.winding_grad(p, v, f)[1], G.winding_grad_kernel32(p, v, f)[1]
    mesh = eng.mesh(T(v), T(f))
    w, g = mesh.winding_grad(T(p))
    tag = f'{name}/{group} ({len(f)} faces, {len(p)} points)'
    scale = np.abs(r64).max()
    own = np.abs(golden()[f'{name}/{group}/g32'] - r64).max() / scale
    print(f'{tag}: max |kernel - oracle| / max |g| {np.abs(g.cpu().numpy() - r64).max() / scale:.3e}; the reference\'s float32 autograd, for the record: {own:.3e}')
    parity(tag, g.cpu().numpy(), r32, r64)
    same_bits(f'{tag}: the value is Mesh.winding\'s', w, mesh.winding(T(p)))
    same_rows(f'{tag} twice', mesh.winding_grad(T(p)), (w, g))
    mesh.close()


# ------------------------------------------------------------------------------------------------ shapes, exactness
def face_counts(eng):
    leaf, tile, chunk = eng.lib.ra_mesh_tile(0), eng.lib.ra_winding_tile(0), eng.lib.ra_winding_tile(1)
    assert (leaf, tile, chunk) == (32, 64, W.CHUNK)
    return [1, leaf - 1, leaf, leaf + 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, len(large()[1])]


@pytest.mark.parametrize('k', range(9))
def test_point_and_face_counts_at_tile_and_chunk_edges_and_both_launch_shapes(eng, k):
    """prefixes of the large hull's faces at the leaf, tile and chunk edges and all of them, 1, 63, 64, 65 and 129 points: the default
    launch, the one-pass kernel and the split launch agree bit for bit, and all hold the 10 x rule"""
    v, f, p = large()
    n_faces = face_counts(eng)[k]
    assert n_faces in (1, 31, 32, 33, 1023, 1024, 1025, 2049, 19998) and len(p) == 129
    r64, r32 = large_refs(n_faces)
    mesh = eng.mesh(T(v), T(f[:n_faces]))
    tp = T(p)
    w, g = mesh.winding_grad(tp)
    parity(f'{n_faces} faces, {len(p)} points', g.cpu().numpy(), r32, r64)
    same_bits(f'{n_faces} faces: the value is Mesh.winding\'s', w, mesh.winding(tp))
    one, split = mesh.winding_grad(tp, shape='one_pass'), mesh.winding_grad(tp, shape='split')
    same_rows(f'{n_faces} faces: default = one pass', (w, g), one)
    same_rows(f'{n_faces} faces: split = one pass', split, one)
    for n in (1, 63, 64, 65):
        for shape in (None, 'one_pass', 'split'):
            same_rows(f'{n_faces} faces: the first {n} points, {shape}', mesh.winding_grad(tp[:n], shape=shape), (w[:n], g[:n]))
        same_rows(f'{n_faces} faces: the last {n} points', mesh.winding_grad(tp[-n:]), (w[-n:], g[-n:]))
    mesh.close()


def test_any_order_any_subset_and_the_one_pass_default(eng):
    v, f = W.mesh_case('opened')
    p = T(W.point_sets('opened')['near'])
    mesh = eng.mesh(T(v), T(f))
    base = mesh.winding_grad(p)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(p))).cuda()
    same_rows('permuted points', mesh.winding_grad(p[perm]), (base[0][perm], base[1][perm]))
    pick = torch.from_numpy(np.sort(np.random.default_rng(4).choice(len(p), 97, replace=False))).cuda()
    same_rows('a subset of 97', mesh.winding_grad(p[pick]), (base[0][pick], base[1][pick]))
    same_rows('twice', mesh.winding_grad(p), base)
    mesh.close()
    # past the split threshold the default is the one-pass kernel: the same rows
    v, f, q = large()
    mesh = eng.mesh(T(v), T(f))
    one = mesh.winding_grad(T(q), shape='one_pass')
    reps = eng.lib.ra_winding_tile(2) * eng.lib.ra_winding_tile(0) // len(q) + 1
    many = T(q).repeat(reps, 1)
    same_rows(f'{len(many)} points, default (one pass) = the 129 alone, repeated', mesh.winding_grad(many), (one[0].repeat(reps), one[1].repeat(reps, 1)))
    mesh.close()


# ------------------------------------------------------------------------------------------------ rules
@pytest.mark.parametrize('shape', [None, 'one_pass', 'split'])
def test_nan_rules(eng, shape):
    v, f, _ = large()
    gv, gf, mid = G.edge_gadget()
    v2, f2 = np.concatenate([v, gv]), np.concatenate([f, gf + len(v)])
    base = W.point_sets('hull')['near'][:130].copy()
    p = base.copy()
    bad = {3: [np.nan, 0, 0], 64: [0, np.inf, 0], 65: [0, 0, -np.inf], 70: v[f[1234, 1]], 100: mid, 129: v[f[7, 0]]}
    for i, x in bad.items():
        p[i] = x
    mesh = eng.mesh(T(v2), T(f2))
    (w, g), (w0, g0) = mesh.winding_grad(T(p), shape=shape), mesh.winding_grad(T(base), shape=shape)
    rows = np.array(sorted(bad))
    others = torch.from_numpy(np.setdiff1d(np.arange(len(p)), rows)).cuda()
    print(f'shape {shape}: rows {rows} -> winding {w[rows].cpu().numpy()}, gradient {g[rows].cpu().numpy().tolist()}')
    assert bool((~torch.isfinite(g[rows])).any(1).all()) and bool(torch.isfinite(g[others]).all()) and bool(torch.isfinite(w[others]).all())
    assert bool(torch.isnan(w[[3, 64, 65, 70, 129]]).all()) and bool(torch.isfinite(w[100]))          # on an edge the value is Mesh.winding's
    same_bits('the value', w, mesh.winding(T(p), shape=shape))
    same_rows('every other point as alone', (w[others], g[others]), (w0[others], g0[others]))
    mesh.close()


def test_dropped_faces_contribute_nothing(eng):
    v, f = W.hull()
    p = T(W.point_sets('hull')['near'])
    bad = v.copy()
    bad[int(f[3, 0])] = np.nan
    keep = ~(f == f[3, 0]).any(1)
    a, b = eng.mesh(T(bad), T(f)), eng.mesh(T(v), T(f[keep]))
    # the Morton order of the kept faces is the same, so are the sums
    same_rows(f'{(~keep).sum()} faces dropped', a.winding_grad(p), b.winding_grad(p))
    a.close(), b.close()


def test_flat_pairs_contribute_zero(eng):
    """det == 0: points in the plane of a lone triangle outside it, and a face of three equal vertices beside the hull's faces"""
    tri = np.float32([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]])
    mesh = eng.mesh(T(tri), T(np.array([[0, 1, 2]])))
    w, g = mesh.winding_grad(T(np.float32([[1, 1, 0], [-0.25, 0.125, 0], [2, -1, 0]])))
    print(f'in the plane of one triangle: winding {w.cpu().numpy()}, gradient {g.cpu().numpy().tolist()}')
    assert bool((w == 0).all()) and bool((g == 0).all())
    mesh.close()
    # the `degenerate` mesh of the parity test carries a collinear face and a face of three equal vertices; here the latter alone
    point = np.float32([[0.25, 0.5, 0.125]] * 3)
    mesh = eng.mesh(T(point), T(np.array([[0, 1, 2]])))
    w, g = mesh.winding_grad(T(W.point_sets('hull')['near'][:70]))
    assert bool((w == 0).all()) and bool((g == 0).all())
    mesh.close()


def test_empty_query_and_errors(eng):
    v, f = W.hull()
    L = eng.lib
    mesh = eng.mesh(T(v), T(f))
    p = T(W.point_sets('hull')['near'][:10])
    out, grad = torch.empty(10, device='cuda:0'), torch.empty(10, 3, device='cuda:0')
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert L.ra_mesh_winding_grad(eng.ctx, mesh._handle, None, 0, 0, None, None, eng.stream) == 0                   # n == 0: no pointer is read
    w0, g0 = mesh.winding_grad(torch.empty(0, 3))
    assert w0.shape == (0,) and g0.shape == (0, 3)
    assert L.ra_mesh_winding_grad(eng.ctx, mesh._handle, ptr(p), 10, 0, None, ptr(grad), eng.stream) == 0           # the value is optional
    same_bits('without the value', grad, mesh.winding_grad(p)[1])
    for args, word in (((None, mesh._handle, ptr(p), 10, 0, ptr(out), ptr(grad)), 'null argument'), ((eng.ctx, None, ptr(p), 10, 0, ptr(out), ptr(grad)), 'null argument'),
                       ((eng.ctx, mesh._handle, None, 10, 0, ptr(out), ptr(grad)), 'null argument'), ((eng.ctx, mesh._handle, ptr(p), 10, 0, ptr(out), None), 'null argument'),
                       ((eng.ctx, mesh._handle, ptr(p), -1, 0, ptr(out), ptr(grad)), 'bad sizes'), ((eng.ctx, mesh._handle, ptr(p), 1 << 30, 0, ptr(out), ptr(grad)), 'bad sizes'),
                       ((eng.ctx, mesh._handle, ptr(p), 10, 4, ptr(out), ptr(grad)), 'unknown flag'), ((eng.ctx, mesh._handle, ptr(p), 10, 3, ptr(out), ptr(grad)), 'unknown flag'),
                       ((eng.ctx, C.c_void_p(out.data_ptr()), ptr(p), 10, 0, ptr(out), ptr(grad)), 'not a mesh of this ctx')):
        assert L.ra_mesh_winding_grad(*args, eng.stream) != 0
        msg = L.ra_last_error().decode()
        print(f'{word}: {msg}')
        assert word in msg and 'ra_mesh_winding_grad' in msg
    other = eng.mesh(T(v), T(f))
    other.close()
    with pytest.raises(RaError, match='closed'):
        other.winding_grad(p)
    with pytest.raises(ValueError):
        mesh.winding_grad(p, shape='both')
    # the context works afterwards
    q = points('hull', 'near')
    parity('after the errors', mesh.winding_grad(T(q))[1].cpu().numpy(), G.winding_grad_kernel32(q, v, f)[1], G.winding_grad(q, v, f)[1])
    mesh.close()


# ------------------------------------------------------------------------------------------------ autograd
@functools.lru_cache(None)
def autograd_refs(name):
    """a mesh with both of its point sets — and, for the opened hull, 96 points around the middle of its hole, where the winding number
    lies between the shift's thresholds: winding and distance, value and gradient, in float64 and in float32 restatements"""
    v, f = W.mesh_case(name)
    p = [points(name, 'near'), points(name, 'grid')]
    if name == 'opened':
        top = v[int(np.argmax(v[:, 2]))].astype(np.float64)          # its faces are the hole
        p.append((top + np.random.default_rng(6).normal(0, 0.02, (96, 3))).astype(F32))
    p = np.concatenate(p)
    d2_32, c32 = M.closest_point(p, v, f, np.float32)[:2]
    d32 = np.sqrt(d2_32)
    with np.errstate(all='ignore'):
        gd32 = np.where((d32 > 0)[:, None], (p - c32) / d32[:, None], F32(0)).astype(F32)
    return p, G.winding_grad(p, v, f), G.winding_grad_kernel32(p, v, f), G.distance_grad(p, v, f), (d32, gd32)


def backward_of(fn, p, weights):
    tp = T(p).requires_grad_()
    out = fn(tp)
    (out * T(weights)).sum().backward()
    return out.detach(), tp.grad


def test_winding_number_and_distance_backward(eng):
    v, f = W.hull()
    p, (w64, gw64), (w32, gw32), (d64, gd64), (d32, gd32) = autograd_refs('hull')
    c = np.random.default_rng(5).uniform(0.5, 1.5, len(p)).astype(F32)
    tv, tf = T(v), torch.from_numpy(f)
    mesh = eng.mesh(tv, tf)
    for fn in (mesh_utils.winding_number, lambda *a, **k: mesh_utils.winding_number_nooom(*a, quota_GB=0.001, **k)):
        w, g = backward_of(lambda x: fn(x, tv, tf, engine=eng), p, c)
        parity('winding_number: backward', g.cpu().numpy(), c[:, None] * gw32, c[:, None].astype(np.float64) * gw64)
        same_bits('winding_number: forward with requires_grad', w, mesh.winding(T(p)))
        same_bits('winding_number: backward = upstream x Mesh.winding_grad', g, T(c)[:, None] * mesh.winding_grad(T(p))[1])
    d, g = backward_of(lambda x: mesh_utils.bvh_distance(x, tv, tf, engine=eng), p, c)
    parity('bvh_distance: backward', g.cpu().numpy(), c[:, None] * gd32, c[:, None].astype(np.float64) * gd64)
    same_bits('bvh_distance: forward with requires_grad', d, mesh.closest(T(p), want=('d2',)).d2.sqrt())
    # host points: the gradient comes back where the points are
    hp = torch.from_numpy(p[:70].copy()).requires_grad_()
    mesh_utils.winding_number(hp, tv, tf, engine=eng).sum().backward()
    assert hp.grad.device.type == 'cpu' and hp.grad.shape == (70, 3)
    same_bits('host points', hp.grad, mesh.winding_grad(T(p[:70]))[1])
    # a mesh that is already built serves the call and stays open
    w, g = backward_of(lambda x: mesh_utils.winding_number(x, None, None, mesh=mesh), p[:70], c[:70])
    same_bits('mesh=', g, T(c[:70])[:, None] * mesh.winding_grad(T(p[:70]))[1])
    mesh.close()


@pytest.mark.parametrize('th', W.THRESHOLDS)
def test_winding_distance_backward(eng, th):
    """backward against the oracle composed in float64, on the rows whose float64 winding number is further from a threshold than the
    measured winding error (at most 1 % are not); in the snapped zone the winding term is exactly 0: the gradient is +-grad(d).  On
    the opened hull: a closed one has no point between the thresholds"""
    v, f = W.mesh_case('opened')
    p, (w64, gw64), (w32, gw32), dg64, (d32, gd32) = autograd_refs('opened')
    tv, tf = T(v), torch.from_numpy(f)
    got, g = backward_of(lambda x: mesh_utils.winding_distance(x, tv, tf, winding_th=th, engine=eng), p, np.ones(len(p), dtype=F32))
    mesh = eng.mesh(tv, tf)
    w = mesh.winding(T(p)).cpu().numpy()
    _, gd = backward_of(lambda x: mesh_utils.bvh_distance(x, None, None, mesh=mesh), p, np.ones(len(p), dtype=F32))
    mesh.close()
    err = np.abs(w.astype(np.float64) - w64).max()
    margin = W.threshold_margin(w64, 0.5, th)
    keep = margin > err
    print(f'th {th}: measured winding error {err:.3e}; {(~keep).sum()} of {len(p)} points within it of a threshold (at most 1 %)')
    assert (~keep).sum() <= 0.01 * len(p)
    val64, grad64, _ = G.winding_distance_grad(p, v, f, th, wg=(w64, gw64), dg=dg64)
    s32 = W.winding_shift(w32, 0.5, th)
    grad32 = ((G.shift_slope(w32, 0.5, th).astype(F32) * d32)[:, None] * gw32 + s32[:, None] * gd32).astype(F32)          # float32 throughout
    parity(f'th {th}: winding_distance backward', g.cpu().numpy(), grad32, grad64, keep=np.repeat(keep[:, None], 3, 1))
    state = W.shift_state(w64, 0.5, th)
    snapped = keep & (state != 0)
    print(f'th {th}: clamped low {(state == -1).sum()}, free {(state == 0).sum()}, clamped high {(state == 1).sum()}')
    assert snapped.sum() > 1000 and (keep & (state == 0)).sum() > 30
    rows = torch.from_numpy(np.nonzero(snapped)[0]).cuda()
    exact = bool(torch.equal(g[rows], T(state[snapped].astype(F32))[:, None] * gd[rows]))          # as values: a zero component may come out as -0
    print(f'th {th}: {int(snapped.sum())} snapped rows: the gradient is exactly shift x grad(d): {exact}')
    assert exact
    same_bits(f'th {th}: forward with requires_grad', got, mesh_utils.winding_distance(T(p), tv, tf, winding_th=th, engine=eng))


def test_without_requires_grad_the_calls_and_bits_are_the_plain_ones(eng, monkeypatch):
    from relightableavatar_amd.engine import Mesh
    v, f = W.mesh_case('opened')
    p = T(W.point_sets('opened')['near'])
    tv, tf = T(v), torch.from_numpy(f)
    mesh = eng.mesh(tv, tf)
    w, d = mesh.winding(p), mesh.closest(p, want=('d2',)).d2.sqrt()
    calls = []
    plain = Mesh.winding_grad
    monkeypatch.setattr(Mesh, 'winding_grad', lambda self, *a, **k: (calls.append(1), plain(self, *a, **k))[1])
    same_bits('winding_number', mesh_utils.winding_number(p, tv, tf, engine=eng), w)
    same_bits('bvh_distance', mesh_utils.bvh_distance(p, tv, tf, engine=eng), d)
    same_bits('winding_distance', mesh_utils.winding_distance(p, tv, tf, engine=eng), mesh_utils.winding_shift(w, 0.5, 0.45) * d)
    with torch.no_grad():
        same_bits('winding_number under no_grad', mesh_utils.winding_number(p.clone().requires_grad_(), tv, tf, engine=eng), w)
    assert not calls, 'the gradient kernel ran without requires_grad'
    out = mesh_utils.winding_number(p.clone().requires_grad_(), tv, tf, engine=eng)
    assert len(calls) == 1 and out.requires_grad
    same_bits('winding_number with requires_grad', out.detach(), w)
    mesh.close()


# ------------------------------------------------------------------------------------------------ isosurface_fitting
FIT = dict(param_lambda=29, opt_iter=30, lr=1e-3)


@functools.lru_cache(None)
def fit_case():
    """source: the hull scaled by 1.15 about its centroid; target: the opened hull"""
    v, f = W.hull()
    c = v.mean(0, dtype=np.float64)
    return (c + 1.15 * (v.astype(np.float64) - c)).astype(F32), f, *W.mesh_case('opened')


def fit_loss(eng, f, verts, tv, tf, thresh):
    return float((f(verts, tv, tf, engine=eng) - thresh).pow(2).sum())


def run_fit(eng, f, thresh, seed=7):
    sv, sf, tv, tf = fit_case()
    gen = torch.Generator(device='cuda:0')
    gen.manual_seed(seed)
    return mesh_utils.isosurface_fitting(T(sv), torch.from_numpy(sf), T(tv), torch.from_numpy(tf), f=f, thresh=thresh, chunk_size=len(sv), generator=gen,
                                         engine=eng, **FIT)


def test_isosurface_first_gradient(eng):
    """the parameter's gradient after the first backward: the oracle's gradient of sum (w - 0.5)^2 pushed through a dense float64 solve
    of M = I + lambda L, and the float32 restatement's pushed through the same solve, under the 10 x rule"""
    sv, sf, tv, tf = fit_case()
    Mx = largesteps.compute_matrix(T(sv), torch.from_numpy(sf), FIT['param_lambda'], engine=eng)
    param = largesteps.to_differential(Mx, T(sv)).detach().requires_grad_()
    verts = largesteps.from_differential(Mx, param, 'Cholesky', x0=T(sv))
    gen = torch.Generator(device='cuda:0')
    gen.manual_seed(7)
    query = verts[torch.randperm(len(verts), device='cuda:0', generator=gen)]
    (mesh_utils.winding_number(query, T(tv), torch.from_numpy(tf), engine=eng) - 0.5).pow(2).sum().backward()
    at = verts.detach().cpu().numpy()
    (w64, g64), (w32, g32) = G.winding_grad(at, tv, tf), G.winding_grad_kernel32(at, tv, tf)
    dense = FR.truth_matrix(sf, len(sv), FIT['param_lambda']).toarray()
    r64 = np.linalg.solve(dense, (2 * (w64 - 0.5))[:, None] * g64)
    r32 = np.linalg.solve(dense, ((F32(2) * (w32 - F32(0.5)))[:, None] * g32).astype(np.float64)).astype(F32)
    parity('the parameter\'s first gradient', param.grad.cpu().numpy(), r32, r64)


def test_isosurface_fitting_on_the_winding_number(eng):
    sv, sf, tv, tf = fit_case()
    out = run_fit(eng, mesh_utils.winding_number, 0.5)
    before = fit_loss(eng, mesh_utils.winding_number, T(sv), T(tv), torch.from_numpy(tf), 0.5)
    after = fit_loss(eng, mesh_utils.winding_number, out, T(tv), torch.from_numpy(tf), 0.5)
    print(f'isosurface_fitting, f = winding_number, thresh 0.5, {FIT["opt_iter"]} iterations: loss over all {len(sv)} vertices {before:.6f} -> {after:.6f}; '
          f'largest move {(out - T(sv)).norm(dim=-1).max().item():.4f}')
    assert out.shape == (len(sv), 3) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    assert after < before
    same_bits('the same seed twice', run_fit(eng, mesh_utils.winding_number, 0.5), out)


def test_isosurface_fitting_on_the_winding_distance(eng):
    sv, sf, tv, tf = fit_case()
    out = run_fit(eng, mesh_utils.winding_distance, 0.0)
    before = fit_loss(eng, mesh_utils.winding_distance, T(sv), T(tv), torch.from_numpy(tf), 0.0)
    after = fit_loss(eng, mesh_utils.winding_distance, out, T(tv), torch.from_numpy(tf), 0.0)
    print(f'isosurface_fitting, f = winding_distance, thresh 0.0, {FIT["opt_iter"]} iterations: loss over all {len(sv)} vertices {before:.6f} -> {after:.6f}')
    assert bool(torch.isfinite(out).all()) and after < before
    same_bits('the same seed twice', run_fit(eng, mesh_utils.winding_distance, 0.0), out)

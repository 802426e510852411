"""ra_topo_diffuse_apply / _solve, ra_mesh_normals, ra_icp_residual, ra_adam_uniform_step, relightableavatar_amd.largesteps and the
fitting functions of mesh_utils on the device.  Run with `-m gpu` on an MI355X.

Two kinds of check.  Bit for bit: every result equals the numpy restatement in the kernels' operation order (tests/fit_ref.py, which
tests/test_oracle_icp.py pins to the reference's outputs and to the plain definitions), from run to run, and a channel solved beside
others equals the same channel solved alone.  The 10 x float32 rule: against a float64 truth (scipy's spsolve, the reference's float64
golden, the float64 fitting loop) the error is at most 10 x the error of the same computation run in float32 (float32 spsolve, the
reference's float32 golden, the float32 fitting loop).  Every test prints its figures before it asserts."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import fit_ref as Ft
import topology_ref as T
from relightableavatar_amd import _lib, largesteps, mesh_utils
from relightableavatar_amd._lib import RaError
from relightableavatar_amd.config import make_cfg

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -23
APPLY_MESHES = ('octa', 'unref', 'repeat', 'fan40', 'v255', 'v256', 'v257')
SOLVE_MESHES = ('octa', 'unref', 'repeat', 'sphere66', 'sphere258', 'sphere1026', 'patch5', 'fin', 'two', 'fan40', 'v255', 'v257')
NORMAL_MESHES = ('octa', 'sphere66', 'patch5', 'fin', 'two', 'fan40', 'unref', 'repeat')
ICP_CASES = ('s66_on_258', 's258_on_66', 'patch_on_fin')
ANGLE_TH = float(np.cos(np.deg2rad(45.0)))


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from relightableavatar_amd.engine import Engine
    return Engine(make_cfg('relight'), device='cuda:0')          # any context will do: no weights are read


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(REPO, 'tests', 'golden', 'icp.npz'))


def D(a, dev='cuda:0'):
    return torch.from_numpy(np.array(a, order='C')).to(dev)       # a copy: the shared arrays are read-only


def N(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)) if a.size else 0.0


def make(eng, name):
    v, f = T.mesh(name)
    return eng.topology(D(f.astype(np.int32)), len(v))


@functools.lru_cache(None)
def values(name, Cn):
    v, _ = T.mesh(name)
    extra = np.random.default_rng(23).standard_normal((len(v), max(Cn - 3, 0)))
    out = np.ascontiguousarray(np.concatenate([v, extra], axis=1)[:, :Cn], dtype=np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(None)
def rhs(name, lam):
    """a smooth right-hand side, as the fitting has: M v in float32"""
    out = Ft.apply(values(name, 3), T.topo(name), lam)
    out.setflags(write=False)
    return out


@functools.lru_cache(None)
def want_solve(name, lam):
    return Ft.solve(rhs(name, lam), T.topo(name), lam)


def test_tile_is_the_restatements(eng):
    assert eng.lib.ra_fit_tile(0) == Ft.TILE and eng.lib.ra_fit_tile(1) == Ft.TILE


@pytest.mark.parametrize('name', APPLY_MESHES)
def test_apply_equals_the_restatement_bit_for_bit(eng, name):
    topo = make(eng, name)
    for Cn in (1, 3, 4, 64):
        x = values(name, Cn)
        src = D(x)
        got = topo.diffuse_apply(src, 29.0)
        want = Ft.apply(x, T.topo(name), 29.0)
        ok = same_bits(N(got), want)
        print(f'{name}: V {topo.V} C {Cn}: bit-equal {ok}, max |diff| {np.abs(N(got).astype(np.float64) - want).max():.3e}')
        assert got.shape == (topo.V, Cn) and got.dtype == torch.float32 and ok
        assert torch.equal(src, D(x)), 'the input is not modified'
    if name == 'unref':
        got = N(topo.diffuse_apply(D(values(name, 3)), 29.0))
        assert same_bits(got[[3, 7]], values(name, 3)[[3, 7]]), 'an isolated vertex has the row out = x'
    if name == 'octa':
        flat = topo.diffuse_apply(D(values(name, 1)).reshape(-1), 9.0)
        assert flat.shape == (topo.V,) and same_bits(N(flat), Ft.apply(values(name, 1), T.topo(name), 9.0).reshape(-1))
        assert same_bits(N(topo.diffuse_apply(D(values(name, 3)), 0.0)), values(name, 3)), 'lambda = 0 is the identity'
    topo.close()


@pytest.mark.parametrize('name', SOLVE_MESHES)
def test_solve_bits_and_parity(eng, name):
    topo = make(eng, name)
    v, f = T.mesh(name)
    for lam in (0, 9, 29):
        if name in ('v255', 'v257') and lam != 29:
            continue
        b = rhs(name, lam)
        want, w_it, w_stop, w_res = want_solve(name, lam)
        got, info = topo.diffuse_solve(D(b), lam, info=True)
        again = topo.diffuse_solve(D(b), lam)
        g = N(got)
        ok = same_bits(g, want)
        truth = Ft.truth_solve(f, len(v), lam, b.astype(np.float64))
        f32 = Ft.truth_solve(f, len(v), lam, b, np.float32)
        err, ref = rel(g, truth), rel(f32, truth)
        print(f'{name} lambda {lam}: iterations {N(info.iters).tolist()} (restatement {w_it.tolist()}) residual {N(info.residual).max():.3e}; bit-equal {ok}; '
              f'error {err:.3e}, float32 spsolve {ref:.3e}')
        assert ok and same_bits(N(again), g), 'the restatement\'s bits, twice'
        assert np.array_equal(N(info.iters), w_it) and np.array_equal(N(info.stop), w_stop) and same_bits(N(info.residual), w_res)
        assert err <= 10 * max(ref, EPS32), 'the 10 x float32 rule against spsolve'
        # each channel alone: the same bits
        for ch in range(3):
            alone = topo.diffuse_solve(D(b[:, ch]), lam)
            assert alone.shape == (topo.V,) and same_bits(N(alone), g[:, ch]), ch
    topo.close()


def test_solve_control_cases(eng):
    name, lam = 'sphere258', 29
    topo = make(eng, name)
    b = rhs(name, lam)
    x, it, stop, res = want_solve(name, lam)
    x0 = values(name, 3)
    got, info = topo.diffuse_solve(D(b), lam, x0=D(x0), max_iter=0, info=True)
    assert same_bits(N(got), x0) and not N(info.iters).any() and not N(info.stop).any(), 'max_iter = 0 returns x0'
    got, info = topo.diffuse_solve(D(b), lam, max_iter=5, info=True)
    w = Ft.solve(b, T.topo(name), lam, max_iter=5)
    print(f'max_iter 5: iterations {N(info.iters).tolist()} stop {N(info.stop).tolist()} residual {N(info.residual).tolist()}')
    assert same_bits(N(got), w[0]) and (N(info.iters) == 5).all() and (N(info.stop) == Ft.STOP_NONE).all() and (N(info.residual) > 1e-9).all()
    assert same_bits(N(info.residual), w[3])
    # the float32 rounding of the solution leaves a residual of about cond x 2^-24 |x|: a warm start passes a tolerance above that
    got, info = topo.diffuse_solve(D(b), lam, x0=D(x), tol=1e-3, info=True)
    print(f'warm start: residual {N(info.residual).max():.3e}')
    assert same_bits(N(got), x) and not N(info.iters).any() and (N(info.stop) == Ft.STOP_CONVERGED).all()
    # ... and at the default tolerance it takes fewer iterations than a cold start, to the restatement's bits
    got, info = topo.diffuse_solve(D(b), lam, x0=D(x), info=True)
    w = Ft.solve(b, T.topo(name), lam, x0_32=x)
    print(f'warm start at 1e-9: iterations {N(info.iters).tolist()} against {it.tolist()} cold')
    assert same_bits(N(got), w[0]) and np.array_equal(N(info.iters), w[1]) and (N(info.iters) < it).all()
    got, info = topo.diffuse_solve(D(np.zeros_like(b)), lam, x0=D(x), info=True)
    assert not N(got).any() and (N(info.stop) == Ft.STOP_ZERO).all(), 'b = 0 gives x = 0'
    for where in ('b', 'x0'):
        bad_b, bad_x = b.copy(), np.zeros_like(b)
        (bad_b if where == 'b' else bad_x)[7, 1] = np.nan if where == 'b' else np.inf
        got, info = topo.diffuse_solve(D(bad_b), lam, x0=D(bad_x), info=True)
        g = N(got)
        assert np.isnan(g[:, 1]).all() and N(info.stop)[1] == Ft.STOP_NAN and same_bits(g[:, [0, 2]], x[:, [0, 2]]), f'a non-finite {where} stays in its channel'
    topo.close()


def test_solve_and_apply_errors(eng):
    topo = make(eng, 'octa')
    L, ctx, h, s = eng.lib, eng.ctx, topo._handle, eng.stream
    x = D(values('octa', 3))
    out = torch.empty_like(x)
    p = lambda t: C.c_void_p(t.data_ptr())

    def fails(rc, what):
        assert rc != 0 and what.encode() in L.ra_last_error(), (what, L.ra_last_error())
    fails(L.ra_topo_diffuse_apply(ctx, None, p(x), 6, 3, 1.0, p(out), s), 'null argument')
    fails(L.ra_topo_diffuse_apply(ctx, h, None, 6, 3, 1.0, p(out), s), 'null argument')
    fails(L.ra_topo_diffuse_apply(ctx, h, p(x), 5, 3, 1.0, p(out), s), 'bad sizes')
    fails(L.ra_topo_diffuse_apply(ctx, h, p(x), 6, 65, 1.0, p(out), s), 'bad sizes')
    fails(L.ra_topo_diffuse_apply(ctx, h, p(x), 6, 3, -1.0, p(out), s), 'bad lambda')
    fails(L.ra_topo_diffuse_apply(ctx, h, p(x), 6, 3, float('nan'), p(out), s), 'bad lambda')
    fails(L.ra_topo_diffuse_apply(ctx, C.c_void_p(p(x).value), p(x), 6, 3, 1.0, p(out), s), 'not a topology of this ctx')
    fails(L.ra_topo_diffuse_solve(None, h, p(x), 6, 3, 1.0, None, 1e-9, 8, p(out), None, s), 'null argument')
    fails(L.ra_topo_diffuse_solve(ctx, h, None, 6, 3, 1.0, None, 1e-9, 8, p(out), None, s), 'null argument')
    fails(L.ra_topo_diffuse_solve(ctx, h, p(x), 6, 0, 1.0, None, 1e-9, 8, p(out), None, s), 'bad sizes')
    fails(L.ra_topo_diffuse_solve(ctx, h, p(x), 6, 3, 1.0, None, 1e-9, -1, p(out), None, s), 'bad sizes')
    fails(L.ra_topo_diffuse_solve(ctx, h, p(x), 6, 3, float('nan'), None, 1e-9, 8, p(out), None, s), 'bad lambda')
    fails(L.ra_topo_diffuse_solve(ctx, h, p(x), 6, 3, -2.0, None, 1e-9, 8, p(out), None, s), 'bad lambda')
    fails(L.ra_topo_diffuse_solve(ctx, h, p(x), 6, 3, 1.0, None, float('nan'), 8, p(out), None, s), 'bad tol')
    fails(L.ra_topo_diffuse_solve(ctx, h, p(x), 6, 3, 1.0, None, -1e-3, 8, p(out), None, s), 'bad tol')
    fails(L.ra_topo_diffuse_solve(ctx, C.c_void_p(p(x).value), p(x), 6, 3, 1.0, None, 1e-9, 8, p(out), None, s), 'not a topology of this ctx')
    fails(L.ra_mesh_normals(ctx, h, p(x), 6, None, None, None, s), 'null argument')
    fails(L.ra_mesh_normals(ctx, h, p(x), 7, p(out), None, None, s), 'bad sizes')
    with pytest.raises(ValueError):
        topo.diffuse_apply(torch.zeros(5, 3), 1.0)
    with pytest.raises(ValueError):
        topo.diffuse_solve(x, 1.0, x0=torch.zeros(6, 2))
    with pytest.raises(RaError, match='bad lambda'):
        topo.diffuse_solve(x, -1.0)
    topo.close()


def test_parameterisation_round_trip_and_gradient(eng):
    name, lam = 'sphere258', 29
    v, f = T.mesh(name)
    v32 = values(name, 3)
    M = largesteps.compute_matrix(D(v32), D(f), lam, engine=eng)
    u = largesteps.to_differential(M, D(v32))
    assert same_bits(N(u), rhs(name, lam))
    u = u.detach().requires_grad_()
    back = largesteps.from_differential(M, u, 'Cholesky')
    err = rel(N(back), v32.astype(np.float64))
    f32 = Ft.truth_solve(f, len(v), lam, rhs(name, lam), np.float32)
    ref = rel(f32, Ft.truth_solve(f, len(v), lam, rhs(name, lam).astype(np.float64)))
    print(f'from_differential(to_differential(v)) - v: {err:.3e}; float32 spsolve on the same system {ref:.3e}')
    assert same_bits(N(back), want_solve(name, lam)[0]) and err <= 10 * max(ref, EPS32)
    g = np.random.default_rng(31).standard_normal(v32.shape).astype(np.float32)
    back.backward(D(g))
    assert same_bits(N(u.grad), N(M.solve(D(g)))), 'the backward of the solve is the forward solve of the gradient, bit for bit'
    assert same_bits(N(u.grad), Ft.solve(g, T.topo(name), lam)[0])
    w = D(v32).requires_grad_()
    largesteps.to_differential(M, w).backward(D(g))
    assert same_bits(N(w.grad), Ft.apply(g, T.topo(name), lam)), 'the backward of the apply is the apply'
    with pytest.raises(ValueError, match='method'):
        largesteps.from_differential(M, u, 'LU')


@pytest.mark.parametrize('name', NORMAL_MESHES)
def test_normals(eng, golden, name):
    v, f = T.mesh(name)
    v32 = v.astype(np.float32)
    topo = make(eng, name)
    got = topo.normals(D(v32))
    wfn, war, wvn = Ft.normals(v32, f, T.topo(name))
    fn, ar, vn = N(got.face_normal), N(got.face_area), N(got.vert_normal)
    tn, ta, tvn = Ft.normals64(v32.astype(np.float64), f, T.topo(name))
    en, ea, evn = rel(fn, tn), rel(ar, ta), rel(vn, tvn)
    rn, ra = rel(golden[f'{name}/face_normals32'], tn), rel(golden[f'{name}/face_areas32'], ta)
    oks = same_bits(fn, wfn), same_bits(ar, war), same_bits(vn, wvn)
    print(f'{name}: bit-equal {oks}; face normals {en:.3e} (reference float32 {rn:.3e}), areas {ea:.3e} ({ra:.3e}), vertex normals {evn:.3e}')
    assert all(oks)
    assert en <= 10 * max(rn, EPS32) and ea <= 10 * max(ra, EPS32) and evn <= 10 * EPS32
    assert np.isfinite(fn).all() and np.isfinite(ar).all() and np.isfinite(vn).all(), 'a degenerate face and an unreferenced vertex stay finite through the eps rules'
    only = topo.normals(D(v32), want=('vert_normal',))
    assert set(only) == {'vert_normal'} and same_bits(N(only.vert_normal), vn)
    assert same_bits(N(mesh_utils.face_normals(D(v32), D(f), engine=eng)), fn) and same_bits(N(mesh_utils.get_face_areas(D(v32), D(f), engine=eng)), ar)
    e = T.topo(name)['edges']
    el = N(mesh_utils.get_edge_length(D(v32), D(e)))
    assert rel(el, Ft.edge_length(v32.astype(np.float64), e)) <= 10 * max(rel(golden[f'{name}/edge_length32'], golden[f'{name}/edge_length64']), EPS32)
    topo.close()


def _icp_inputs(golden, name):
    p, n0, tv, tf = (golden[f'{name}/{k}'] for k in ('points', 'point_normals', 'verts', 'faces'))
    return p.astype(np.float32), n0.astype(np.float32), tv.astype(np.float32), tf, float(golden[f'{name}/dist_th'])


@pytest.mark.parametrize('name', ICP_CASES)
def test_icp_residual(eng, golden, name):
    p, n0, tv, tf, dist_th = _icp_inputs(golden, name)
    topo = eng.topology(D(tf.astype(np.int32)), len(tv))
    n1 = topo.normals(D(tv), want=('face_normal',)).face_normal
    mesh = eng.mesh(D(tv), torch.from_numpy(tf.copy()))
    got = mesh.icp_residual(D(p), D(n0), n1, dist_th, ANGLE_TH, want_keep=True)
    q = mesh.closest(D(p), want=('d2', 'closest', 'face'))
    sums, grad, keep = Ft.icp_residual(p, n0, N(n1), N(q.d2), N(q.closest), N(q.face), dist_th, ANGLE_TH)
    mask_ok = np.array_equal(N(got.keep), golden[f'{name}/keep'])
    l64, l32 = float(golden[f'{name}/loss64']), float(golden[f'{name}/loss32'])
    g64, g32 = golden[f'{name}/grad64'], golden[f'{name}/grad32']
    loss = float(got.loss)
    el, rl, eg, rg = abs(loss - l64) / l64, abs(l32 - l64) / l64, rel(N(got.grad), g64), rel(g32, g64)
    print(f'{name}: kept {int(N(got.sums)[1])} of {len(p)}, mask equal {mask_ok}; sums bit-equal {same_bits(N(got.sums), sums)}; loss {el:.3e} (reference float32 {rl:.3e}); '
          f'gradient {eg:.3e} ({rg:.3e})')
    assert mask_ok and np.array_equal(keep, golden[f'{name}/keep']), 'the kept mask equals the reference\'s, no row excused'
    assert same_bits(N(got.sums), sums) and same_bits(N(got.grad), grad)
    assert el <= 10 * max(rl, EPS32) and eg <= 10 * max(rg, EPS32)
    # the autograd op: the same loss and gradient; the triangles of the reference's signature build their own mesh
    for target in (mesh, D(tv)[D(tf)]):
        pt = D(p).requires_grad_()
        out = mesh_utils.icp_loss(pt, target, D(n0), n1, dist_th, ANGLE_TH, engine=eng)
        out.backward()
        assert out.dtype == torch.float32 and float(out.detach()) == float(np.float32(sums[0] / sums[1])) and same_bits(N(pt.grad), grad)
    mesh.close(), topo.close()


def test_icp_residual_edges(eng, golden):
    p, n0, tv, tf, _ = _icp_inputs(golden, 's258_on_66')
    topo = eng.topology(D(tf.astype(np.int32)), len(tv))
    n1 = topo.normals(D(tv), want=('face_normal',)).face_normal
    mesh = eng.mesh(D(tv), torch.from_numpy(tf.copy()))
    # nothing kept: NaN loss, zero gradient (the reference's empty mean)
    g = golden['none_kept/points'].astype(np.float32), golden['none_kept/point_normals'].astype(np.float32)
    m2 = eng.mesh(D(golden['none_kept/verts'].astype(np.float32)), torch.from_numpy(golden['none_kept/faces'].copy()))
    t2 = eng.topology(D(golden['none_kept/faces'].astype(np.int32)), len(golden['none_kept/verts']))
    none = m2.icp_residual(D(g[0]), D(g[1]), t2.normals(D(golden['none_kept/verts'].astype(np.float32)), want=('face_normal',)).face_normal,
                           float(golden['none_kept/dist_th']), ANGLE_TH, want_keep=True)
    assert np.isnan(float(none.loss)) and not N(none.grad).any() and not N(none.keep).any() and N(none.sums).tolist() == [0.0, 0.0]
    assert np.isnan(golden['none_kept/loss64']) and not golden['none_kept/grad64'].any()
    m2.close(), t2.close()
    empty = mesh.icp_residual(torch.zeros(0, 3), torch.zeros(0, 3), n1)
    assert N(empty.sums).tolist() == [0.0, 0.0] and empty.grad.shape == (0, 3) and np.isnan(float(empty.loss))
    tile = eng.lib.ra_fit_tile(1)
    assert len(p) > tile + 1
    full = None
    for n in (tile - 1, tile, tile + 1):
        got = mesh.icp_residual(D(p[:n]), D(n0[:n]), n1, 0.1, ANGLE_TH, want_keep=True)
        q = mesh.closest(D(p[:n]), want=('d2', 'closest', 'face'))
        sums, grad, keep = Ft.icp_residual(p[:n], n0[:n], N(n1), N(q.d2), N(q.closest), N(q.face), 0.1, ANGLE_TH)
        print(f'n {n}: kept {int(sums[1])}, sums bit-equal {same_bits(N(got.sums), sums)}')
        assert same_bits(N(got.sums), sums) and same_bits(N(got.grad), grad) and np.array_equal(N(got.keep), keep)
        full = got if n == tile + 1 else full
    # one NaN point among them: not kept, and every other row as before
    bad = p[:tile + 1].copy()
    row = int(np.flatnonzero(N(full.keep))[3])
    bad[row, 1] = np.nan
    got = mesh.icp_residual(D(bad), D(n0[:tile + 1]), n1, 0.1, ANGLE_TH, want_keep=True)
    want_keep = N(full.keep).copy()
    want_keep[row] = False
    q = mesh.closest(D(bad), want=('d2', 'closest', 'face'))
    sums, grad, keep = Ft.icp_residual(bad, n0[:tile + 1], N(n1), N(q.d2), N(q.closest), N(q.face), 0.1, ANGLE_TH)
    assert np.array_equal(N(got.keep), want_keep) and N(got.sums)[1] == N(full.sums)[1] - 1 and np.isfinite(N(got.sums)).all()
    assert same_bits(N(got.sums), sums) and same_bits(N(got.grad), grad) and not N(got.grad)[row].any()
    with pytest.raises(ValueError):
        mesh.icp_residual(D(p), D(n0[:5]), n1)
    L = eng.lib
    assert L.ra_icp_residual(eng.ctx, mesh._handle, None, None, 4, None, 0.1, 0.7, C.c_void_p(got.sums.data_ptr()), None, None, eng.stream) != 0
    assert b'null argument' in L.ra_last_error()
    mesh.close(), topo.close()


def test_adam_uniform_three_steps(eng):
    rng = np.random.default_rng(41)
    shape = (777, 3)          # more than one workgroup, no multiple of it
    p0 = rng.standard_normal(shape).astype(np.float32)
    param = D(p0).requires_grad_()
    opt = largesteps.AdamUniform([param], lr=3e-2, engine=eng)
    q, g1, g2 = p0.copy(), np.zeros(shape, dtype=np.float32), np.float32(0)
    for t in range(1, 4):
        g = (rng.standard_normal(shape) * 10.0 ** -t).astype(np.float32)
        param.grad = D(g)
        opt.step()
        q, g1, g2 = Ft.adam_step(q, g, g1, g2, t, 3e-2)
        st = opt.state[param]
        oks = same_bits(N(param), q), same_bits(N(st['g1']), g1), same_bits(N(st['g2']), np.asarray([g2]))
        print(f'step {t}: bit-equal param / g1 / g2 {oks}; g2 {float(st["g2"]):.6e}')
        assert all(oks) and st['step'] == t and st['g2'].numel() == 1
    L = eng.lib
    assert L.ra_adam_uniform_step(eng.ctx, None, None, None, None, 5, 1, 0.1, 0.9, 0.999, eng.stream) != 0 and b'null argument' in L.ra_last_error()
    assert L.ra_adam_uniform_step(eng.ctx, None, None, None, None, 5, 0, 0.1, 0.9, 0.999, eng.stream) != 0 and b'bad sizes' in L.ra_last_error()


@functools.lru_cache(None)
def fit_truth(focus):
    v0, v1, f = Ft.fit_pair()
    sel = Ft.boundary_rows(f, len(v0), 1) if focus else None
    margins = []
    w64 = Ft.fit(v0, f, v1, f, 29, Ft.FIT_ITERS, Ft.FIT_LR, sel, sel, margins=margins)
    w32 = Ft.fit(v0, f, v1, f, 29, Ft.FIT_ITERS, Ft.FIT_LR, sel, sel, dtype=np.float32)
    return w64, w32, min(margins)


@pytest.mark.parametrize('focus', (False, True))
def test_fitting_against_the_float64_loop(eng, focus, capsys):
    v0, v1, f = Ft.fit_pair()
    w64, w32, margin = fit_truth(focus)
    assert margin > 0.05 and w64[2][-1] < 0.5 * w64[2][0] and (np.diff(w64[2]) < 0).all()
    got = mesh_utils.bidirectional_icp_fitting(D(v0.astype(np.float32)), D(f), D(v1.astype(np.float32)), D(f), 29, Ft.FIT_ITERS, 5, Ft.FIT_LR,
                                               boundary_focus=focus, dilate=1, engine=eng)
    printed = capsys.readouterr().out
    errs = [rel(N(got[k]), w64[k]) for k in range(2)]
    refs = [rel(w32[k], w64[k]) for k in range(2)]
    moved = float(np.abs(N(got[0]).astype(np.float64) - v0).max())
    print(f'boundary_focus {focus}: moved {moved:.3e}; loss of the float64 loop {w64[2][0]:.3e} -> {w64[2][-1]:.3e}; error {errs[0]:.3e} {errs[1]:.3e}, '
          f'float32 loop {refs[0]:.3e} {refs[1]:.3e}; margin {margin:.3f}')
    assert got[0].shape == (81, 3) and got[0].dtype == torch.float32 and got[0].is_cuda and moved > 1e-3
    assert printed.count('bidirectional L2 loss') == 4, 'the loss is read every ep_iter iterations only'
    assert all(e <= 10 * max(r, EPS32) for e, r in zip(errs, refs))


def test_fitting_refuses_a_closed_mesh_under_boundary_focus(eng):
    v, f = T.mesh('sphere66')
    with pytest.raises(ValueError, match='boundary'):
        mesh_utils.bidirectional_icp_fitting(D(v.astype(np.float32)), D(f), D(v.astype(np.float32)), D(f), opt_iter=1, engine=eng)

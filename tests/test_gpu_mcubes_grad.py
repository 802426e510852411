"""ra_marching_cubes_backward, ra_marching_cubes_attrs, mesh_utils.marching_cubes and differentiable_marching_cubes on the device
(DESIGN.md section 28).  Run with `-m gpu` on an MI355X.

No tolerance is chosen for the kernels: dvolume, dattrs and the vertex attributes are compared bit for bit with the float32 restatement
in kernel order (tests/mcubes_grad_ref.py), which tests/test_oracle_mcubes_grad.py holds to float64 autograd.  The end-to-end criteria
are the issue's.  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import mcubes_grad_ref as G
import mesh_extract_ref as R
from frame_stage_ref import parity
from relightableavatar_amd import mesh_utils, raster_utils
from relightableavatar_amd.config import make_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from relightableavatar_amd.engine import Engine
    return Engine(make_cfg('relight'), device=DEV)          # any context will do: no weights are read


def T(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a)).to(DEV)          # a copy: the shared references are read-only


def bits(t):
    t = torch.as_tensor(np.array(t) if isinstance(t, np.ndarray) else t).cpu()          # a copy: the shared references are read-only
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(tag, got, want):
    x, y = bits(got), bits(want)
    x, y = x.reshape(-1), y.reshape(-1)
    ok = x.shape == y.shape and bool(torch.equal(x, y))
    print(f'{tag}: bit-equal {ok} ({x.numel()} values, {int((x != y).sum()) if x.shape == y.shape else -1} differ)')
    assert ok, tag


def device_backward(eng, c, **kw):
    return eng.marching_cubes_backward(T(c['vol']), c['iso'], c['n_verts'], dverts=T(c['dverts']), attrs=T(c['attrs']), dattr=T(c['dattr']), **kw)


@pytest.mark.parametrize('C_', G.CHANNELS)
@pytest.mark.parametrize('name', G.VOLUMES)
def test_backward_and_attrs_equal_the_restatement_bit_for_bit(eng, name, C_):
    c = G.case(name, C_)
    want_dvol, want_dA, want_va = G.reference(name, C_)
    v, f = eng.marching_cubes(T(c['vol']), c['iso'])
    block = eng.lib.ra_mcubes_tile(0)
    print(name, c['vol'].shape, f'{c["vol"].size / block:.2f} workgroups, C {C_}, verts {c["n_verts"]}')
    assert v.shape[0] == c['n_verts'] and (name != 'all_outside' or c['n_verts'] == 0)
    out = device_backward(eng, c)
    same(f'{name} C={C_} dvolume', out.dvolume, want_dvol)
    assert tuple(out.dvolume.shape) == c['vol'].shape
    if C_:
        same(f'{name} C={C_} dattrs', out.dattrs, want_dA)
        va = eng.marching_cubes_attrs(T(c['vol']), c['iso'], T(c['attrs']), c['n_verts'])
        assert tuple(va.shape) == (c['n_verts'], C_)
        same(f'{name} C={C_} vertex attributes', va, want_va)
    else:
        assert 'dattrs' not in out
    # a repeat gives the same bits; each half alone equals the full call
    again = device_backward(eng, c)
    same('dvolume again', again.dvolume, out.dvolume)
    same('dvolume alone', device_backward(eng, c, want=('dvolume',)).dvolume, out.dvolume)
    if C_:
        same('dattrs again', again.dattrs, out.dattrs)
        half = device_backward(eng, c, want=('dattrs',))
        assert 'dvolume' not in half
        same('dattrs alone', half.dattrs, out.dattrs)
    # without dverts gt starts at +0
    if name in ('random', '2x2x2'):
        want0 = G.backward(c['vol'], c['iso'], None, c['attrs'], c['dattr'])
        got0 = eng.marching_cubes_backward(T(c['vol']), c['iso'], c['n_verts'], attrs=T(c['attrs']), dattr=T(c['dattr']))
        same('dvolume without dverts', got0.dvolume, want0[0])
        if C_:
            same('dattrs without dverts', got0.dattrs, want0[1])


def test_random_volume_has_grid_points_with_six_crossed_edges():
    c = G.case('random', 0)
    topo = c['topo']
    ends = np.bincount(np.concatenate([topo['p'], topo['q']]), minlength=c['vol'].size)
    print('random: grid points by number of crossed edges', np.bincount(ends).tolist())
    assert int((ends == 6).sum()) > 0


def test_smallest_case_before_and_after_the_largest(eng):
    small, large = G.case('2x2x2', 3), G.case('patterns', 64)
    a = device_backward(eng, small)
    big = device_backward(eng, large)
    b = device_backward(eng, small)
    same('largest dvolume', big.dvolume, G.reference('patterns', 64)[0])
    same('2x2x2 dvolume after the largest', b.dvolume, a.dvolume)
    same('2x2x2 dattrs after the largest', b.dattrs, a.dattrs)
    same('2x2x2 dvolume', a.dvolume, G.reference('2x2x2', 3)[0])


def test_all_outside_zero_fills_the_outputs(eng):
    vol = T(G.volume('all_outside')[0])
    n, Cn = vol.numel(), 3
    dvol, dA, A = torch.ones(n, device=DEV), torch.ones(n, Cn, device=DEV), torch.ones(n, Cn, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = eng.lib.ra_marching_cubes_backward(eng.ctx, p(vol), *vol.shape, 0.0, None, 0, p(A), None, Cn, p(dvol), p(dA), eng.stream)
    assert rc == 0, eng.lib.ra_last_error()
    torch.cuda.synchronize()
    assert not bool(dvol.any()) and not bool(dA.any())
    assert eng.lib.ra_marching_cubes_attrs(eng.ctx, p(vol), *vol.shape, 0.0, p(A), Cn, 0, None, eng.stream) == 0


def test_non_finite_ends_contribute_nothing(eng):
    vol, iso, where = G.nonfinite_volume()
    topo = G.topology(vol, iso)
    flat = vol.reshape(-1)
    dead = ~(np.isfinite(flat[topo['p']]) & np.isfinite(flat[topo['q']]))
    rng = np.random.default_rng(5)
    V = topo['n_verts']
    dverts, attrs, dattr = rng.standard_normal((V, 3)).astype(np.float32), rng.uniform(-1, 1, (vol.size, 3)).astype(np.float32), rng.standard_normal((V, 3)).astype(np.float32)
    dverts[dead], dattr[dead] = np.nan, np.nan           # the forward's vertex there is NaN: whatever arrives for it is not read
    v, _ = eng.marching_cubes(T(vol), iso)
    nan_vertex = torch.isnan(v).any(-1).cpu().numpy()      # an infinite b end alone gives t = 0, not NaN: the rule drops that edge all the same
    assert v.shape[0] == V and int(dead.sum()) >= 6 and nan_vertex.any() and not (nan_vertex & ~dead).any()
    out = eng.marching_cubes_backward(T(vol), iso, V, dverts=T(dverts), attrs=T(attrs), dattr=T(dattr))
    want = G.backward(vol, iso, dverts, attrs, dattr)
    dvol, dA = out.dvolume.cpu(), out.dattrs.cpu()
    print('non-finite: edges with a non-finite end', int(dead.sum()), 'of', V, '; dvolume there', [float(dvol[w]) for w in where])
    assert bool(torch.isfinite(dvol).all()) and bool(torch.isfinite(dA).all())
    for w in where:
        assert float(dvol[w]) == 0.0 and not bool(dA.reshape(vol.shape + (3,))[w].any())
    same('non-finite dvolume', dvol, want[0])
    same('non-finite dattrs', dA, want[1])


def test_argument_errors_are_named(eng):
    L, t = eng.lib, torch.zeros(64, device=DEV)
    p = C.c_void_p(t.data_ptr())
    err = lambda: L.ra_last_error().decode()
    big = 1 << 9            # 2^27 points: legal alone, too many elements with 16 channels
    for (nx, ny, nz, Cn, nv), msg in ((((1, 2, 2, 0, 4)), 'bad sizes'), ((1 << 10, 1 << 10, 1 << 10, 0, 4), 'bad sizes'), ((2, 2, 2, 65, 4), 'bad sizes'),
                                      ((2, 2, 2, -1, 4), 'bad sizes'), ((2, 2, 2, 3, -1), 'bad sizes'), ((big, big, big, 16, 4), 'bad sizes'),
                                      ((2, 2, 2, 3, 1 << 30), 'bad sizes')):
        assert L.ra_marching_cubes_backward(eng.ctx, p, nx, ny, nz, 0.0, p, nv, p, p, Cn, p, p, eng.stream) != 0
        assert 'ra_marching_cubes_backward: ' + msg in err(), (msg, err())
        assert L.ra_marching_cubes_attrs(eng.ctx, p, nx, ny, nz, 0.0, p, Cn, nv, p, eng.stream) != 0
        assert 'ra_marching_cubes_attrs: ' + msg in err(), (msg, err())
    nan = float('nan')
    assert L.ra_marching_cubes_backward(eng.ctx, p, 2, 2, 2, nan, p, 4, p, p, 3, p, p, eng.stream) != 0 and 'ra_marching_cubes_backward: bad iso' in err()
    assert L.ra_marching_cubes_attrs(eng.ctx, p, 2, 2, 2, nan, p, 3, 4, p, eng.stream) != 0 and 'ra_marching_cubes_attrs: bad iso' in err()
    for args in ((None, 2, 2, 2, 0.0, p, 4, p, p, 3, p, p), (p, 2, 2, 2, 0.0, p, 4, p, p, 3, None, None), (p, 2, 2, 2, 0.0, p, 4, None, p, 3, p, p),
                 (p, 2, 2, 2, 0.0, p, 4, p, None, 3, p, p)):
        assert L.ra_marching_cubes_backward(eng.ctx, *args, eng.stream) != 0 and 'ra_marching_cubes_backward: null argument' in err(), args
    for args in ((None, 2, 2, 2, 0.0, p, 3, 4, p), (p, 2, 2, 2, 0.0, None, 3, 4, p), (p, 2, 2, 2, 0.0, p, 3, 4, None)):
        assert L.ra_marching_cubes_attrs(eng.ctx, *args, eng.stream) != 0 and 'ra_marching_cubes_attrs: null argument' in err(), args
    assert L.ra_marching_cubes_backward(None, p, 2, 2, 2, 0.0, p, 4, p, p, 3, p, p, eng.stream) != 0 and 'null argument' in err()
    with pytest.raises(ValueError):
        eng.marching_cubes_backward(torch.zeros(1, 4, 4), 0.0, 0)
    with pytest.raises(ValueError):
        eng.marching_cubes_backward(torch.zeros(2, 2, 2), 0.0, 0, want=('dverts',))
    with pytest.raises(ValueError):
        eng.marching_cubes_backward(torch.zeros(2, 2, 2), 0.0, 0, want=('dattrs',))


def test_backward_between_the_size_query_and_the_writing_call(eng):
    """the backward's scratch is its own: the offsets of a pending ra_marching_cubes size query survive it"""
    vol_np, iso = G.volume('33x17x65')
    vol = T(vol_np)
    rv, rf = R.marching_cubes(vol_np, iso)
    nv, nf = C.c_int(), C.c_int()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert eng.lib.ra_marching_cubes(eng.ctx, ptr(vol), *vol.shape, iso, None, None, C.byref(nv), C.byref(nf), eng.stream) == 0
    assert (nv.value, nf.value) == (len(rv), len(rf))
    big, small = G.case('patterns', 4), G.case('random', 3)            # one larger than the pending volume, one smaller
    device_backward(eng, big)
    eng.marching_cubes_attrs(T(small['vol']), small['iso'], T(small['attrs']), small['n_verts'])
    verts, faces = torch.empty(nv.value, 3, device=DEV), torch.empty(nf.value, 3, dtype=torch.int32, device=DEV)
    assert eng.lib.ra_marching_cubes(eng.ctx, ptr(vol), *vol.shape, iso, ptr(verts), ptr(faces), None, None, eng.stream) == 0, eng.lib.ra_last_error()
    same('vertices after an interleaved backward', verts, rv)
    same('faces after an interleaved backward', faces, rf)


def test_mesh_utils_marching_cubes_is_the_engine_call_with_a_backward(eng):
    c = G.case('sphere', 3)
    vol, attrs = T(c['vol']).requires_grad_(), T(c['attrs']).reshape(c['vol'].shape + (3,)).requires_grad_()
    ev, ef = eng.marching_cubes(vol, c['iso'])
    before = eng.lib.ra_mesh_extract_stats(eng.ctx, 1)
    v, f, va = mesh_utils.marching_cubes(vol, c['iso'], attrs, engine=eng)
    same('verts', v, ev)
    same('faces', f, ef)
    same('vertex attributes', va, G.reference('sphere', 3)[2])
    assert v.requires_grad and va.requires_grad and not f.requires_grad and f.dtype == torch.int32
    dverts, dattr = T(c['dverts']), T(c['dattr'])
    ((v * dverts).sum() + (va * dattr).sum()).backward()
    want = device_backward(eng, c)
    same('volume.grad', vol.grad, want.dvolume)
    same('attrs.grad', attrs.grad, want.dattrs)
    assert vol.grad.shape == vol.shape and attrs.grad.shape == attrs.shape
    # positions alone, and without autograd the plain calls
    vol2 = T(c['vol']).requires_grad_()
    v2, f2 = mesh_utils.marching_cubes(vol2, c['iso'], engine=eng)
    (v2 * dverts).sum().backward()
    same('volume.grad, positions alone', vol2.grad, eng.marching_cubes_backward(T(c['vol']), c['iso'], c['n_verts'], dverts=dverts).dvolume)
    v3, f3 = mesh_utils.marching_cubes(T(c['vol']), c['iso'], engine=eng)
    same('verts without autograd', v3, ev)
    assert not v3.requires_grad and eng.lib.ra_mesh_extract_stats(eng.ctx, 1) == before == 1       # one read-back per forward, none behind it


def test_end_to_end_radius_fit(eng):
    """(a) plain gradient steps on the sphere volume (R = 8) lower mean((|v - c| - 6)^2); the same loop on the float64 restatement sets the mark"""
    ref = G.radius_fit_reference()
    cfg, centre = G.RADIUS_FIT, torch.tensor(R.SPHERE['centre'], device=DEV)
    vol = T(R.sphere_volume())
    losses = []
    for _ in range(cfg['steps'] + 1):
        v = vol.clone().requires_grad_()
        verts, _ = mesh_utils.marching_cubes(v, 0.0, engine=eng)
        loss = ((verts - centre).norm(dim=1) - cfg['target']).pow(2).sum()          # a step is lr times the gradient of the SUM
        losses.append(float(loss.detach()) / verts.shape[0])
        loss.backward()
        vol = vol - cfg['lr'] * v.grad
    factor, ref_factor = losses[0] / losses[-1], ref[0] / ref[-1]
    print(f'radius fit: device {losses[0]:.4f} -> {losses[-1]:.4f} (x {factor:.2f}); float64 restatement {ref[0]:.4f} -> {ref[-1]:.4f} (x {ref_factor:.2f})')
    assert abs(ref[0] - 3.9797) < 1e-3 and ref_factor > 9
    assert factor >= 0.5 * ref_factor


SILHOUETTE = dict(n=12, centre=(5.3, 5.6, 5.45), R=4.2, shift=(0.4, -0.3, 0.0), depth=1.5, lr=0.05)


def _camera(H, W, depth):
    Rt = torch.eye(3, device=DEV)[None]
    Tt = torch.tensor([[[0.0], [0.0], [depth]]], device=DEV)
    K = torch.tensor([[1.6 * W / 2, 0, W / 2], [0, 1.6 * W / 2, H / 2], [0, 0, 1]], device=DEV)
    return Rt, Tt, raster_utils.get_ndc_perspective_matrix(K[None], H, W)


def test_end_to_end_silhouette_chain(eng):
    """(b) volume -> marching_cubes -> render_nvdiffrast(antialias=True) -> squared mask error against the mask of a shifted sphere, at
    64 x 64: the gradient arrives at the ends of crossed edges only, and 20 steps lower the loss (test_gpu_antialias.py::test_end_to_end's
    criterion).  A 12^3 volume, so that a voxel spans about 6 pixels: ra_antialias searches the own pixel's face alone for a silhouette
    edge, and finds one the more often the larger the triangles are.  A step moves the gradient's largest entry by 0.05 volume units
    (a plain gradient step, normalised); the target is 0.5 voxels away."""
    H = W = 64
    cfg = SILHOUETTE
    Rt, Tt, P = _camera(H, W, cfg['depth'])
    n = cfg['n']

    def mask(volume):
        verts, faces = mesh_utils.marching_cubes(volume, 0.0, engine=eng)
        world = (verts - (n - 1) / 2) / (n / 2)
        return raster_utils.render_nvdiffrast(world, faces, torch.ones(verts.shape[0], 1, device=DEV), H=H, W=W, R=Rt, T=Tt, K=P, R_S=1, engine=eng,
                                              antialias=True)[1]

    target = mask(T(R.sphere_volume(n, tuple(np.add(cfg['centre'], cfg['shift'])), cfg['R']))).detach()
    vol = T(R.sphere_volume(n, cfg['centre'], cfg['R']))
    losses = []
    for step in range(21):
        v = vol.clone().requires_grad_()
        loss = ((mask(v) - target) ** 2).sum()
        losses.append(float(loss.detach()))
        loss.backward()
        g = v.grad
        if step == 0:
            ends = torch.from_numpy(R.crossed_edges(vol.cpu().numpy(), 0.0))
            is_end = ends.any(-1)
            for ax in range(3):
                is_end |= torch.roll(ends[..., ax], 1, ax)          # the other end of an edge along ax (no edge leaves the last layer: nothing wraps)
            nz = (g != 0).cpu()
            print(f'silhouette: {int(nz.sum())} grid points with a gradient, {int(is_end.sum())} ends of crossed edges, covered pixels {int((target > 0).sum())}, '
                  f'fractional {int(((target > 0) & (target < 1)).sum())}')
            assert int(nz.sum()) > 0 and not bool((nz & ~is_end).any()) and bool(torch.isfinite(g).all())
        vol = vol - cfg['lr'] * g / g.abs().max().clamp(min=1e-30)
    print(f'silhouette fit: loss {losses[0]:.4f} -> {losses[-1]:.4f}', [round(l, 3) for l in losses])
    assert losses[-1] < losses[0]


class _Sphere(torch.nn.Module):
    def __init__(self, radius, centre, dtype=torch.float32, device='cpu'):
        super().__init__()
        self.radius = torch.nn.Parameter(torch.tensor(radius, dtype=dtype, device=device))
        self.centre = torch.nn.Parameter(torch.tensor(centre, dtype=dtype, device=device))

    def forward(self, x):
        return (x - self.centre).norm(dim=-1) - self.radius


SPHERE_FIT = dict(n=24, radius=0.6123, centre=(0.05, -0.03, 0.02), target=0.45)


def _restated_param_grads(mode, dtype):
    """d loss / d (radius, centre) of loss = mean((|v| - target)^2) by the restated rules (tests/mcubes_grad_ref.py) on the CPU"""
    cfg = SPHERE_FIT
    dec = _Sphere(cfg['radius'], cfg['centre'], dtype)
    pts = torch.stack(torch.meshgrid(*[torch.linspace(-1, 1, cfg['n'], dtype=dtype)] * 3, indexing='ij'), -1)
    with torch.no_grad():
        vol = (-dec(pts.reshape(-1, 3))).reshape(pts.shape[:-1]).float()            # the device's volume is float32
    topo = G.topology(vol.numpy(), 0.0)
    scale = 2.0 / (cfg['n'] - 1)
    idx = G.torch_forward(vol.to(dtype), 0.0, topo)[0]
    verts = (idx * scale - 1).requires_grad_()
    loss = ((verts.norm(dim=-1) - cfg['target']) ** 2).mean()
    g = torch.autograd.grad(loss, verts)[0]
    params = (dec.radius, dec.centre)
    if mode == 'normal':
        gr = G.normal_rule_grads(dec, params, verts.detach(), g)
    else:
        F = G.F64 if dtype == torch.float64 else G.F32
        dvol = G.backward(vol.numpy(), 0.0, (g * scale).numpy(), F=F)[0]
        gr = G.grid_rule_grads(dec, params, pts, dvol)
    return torch.cat([gr[0].reshape(1), gr[1].reshape(3)]).detach(), topo['n_verts']


@pytest.mark.parametrize('mode', ('normal', 'grid'))
def test_end_to_end_differentiable_marching_cubes(eng, mode):
    """(c) a torch sphere with a learnable radius and centre: the parameter gradients of both modes against the float64 restatement under
    the 10 x rule, and plain gradient steps that move the radius towards the target"""
    cfg = SPHERE_FIT
    dec = _Sphere(cfg['radius'], cfg['centre'], device=DEV)
    pts = torch.stack(torch.meshgrid(*[torch.linspace(-1, 1, cfg['n'], device=DEV)] * 3, indexing='ij'), -1)
    loss_of = lambda verts: ((verts.norm(dim=-1) - cfg['target']) ** 2).mean()
    verts, faces = mesh_utils.differentiable_marching_cubes(pts, dec, chunk_size=5000, engine=eng, gradient=mode)
    assert verts.requires_grad and faces.dtype == torch.int32 and verts.is_cuda
    loss_of(verts).backward()
    got = torch.cat([dec.radius.grad.reshape(1), dec.centre.grad.reshape(3)]).cpu()
    (r32, nv32), (r64, nv64) = _restated_param_grads(mode, torch.float32), _restated_param_grads(mode, torch.float64)
    print(mode, 'verts', verts.shape[0], nv32, nv64, 'd loss / d (radius, centre): device', got.tolist(), 'float64', r64.tolist())
    assert verts.shape[0] == nv32 == nv64
    parity(f'differentiable_marching_cubes {mode}', got, r32, r64)
    assert float(r64[0]) > 0            # the radius is above the target: the loss falls with it
    radii = [float(dec.radius.detach())]
    for _ in range(5):
        dec.zero_grad()
        v, _ = mesh_utils.differentiable_marching_cubes(pts, dec, chunk_size=5000, engine=eng, gradient=mode)
        loss_of(v).backward()
        with torch.no_grad():
            dec.radius -= 0.2 * dec.radius.grad
        radii.append(float(dec.radius.detach()))
    print(mode, 'radius', [round(r, 4) for r in radii], 'target', cfg['target'])
    assert all(abs(b - cfg['target']) < abs(a - cfg['target']) for a, b in zip(radii, radii[1:]))

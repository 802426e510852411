"""ra_cloth_create / ra_cloth_energy / ra_cloth_inertia and relightableavatar_amd.physx_utils on the device.  Run
with `-m gpu` on an MI355X.

Two kinds of check.  The 10 x float32 rule (tests/test_gpu_fit.py): against the reference's float64 golden the error of an energy, and
of a gradient normalised by its largest magnitude, is at most 10 x the error of the reference's own float32 golden, floored at float32
eps; where there is no golden (the edge shapes) the float64 truth is tests/physx_ref.py and the float32 yardstick the same energies in
float32 torch operations on the CPU.  Bit for bit: a row of a batch equals that row alone, two runs are equal, terms evaluated alone
equal the columns of a joint call.  Every test prints its figures before it asserts."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import physx_ref as P
import topology_ref as T
from relightableavatar_amd import _lib, largesteps, mesh_utils, physx_utils
from relightableavatar_amd.config import make_cfg

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -23
CASES = P.FIXTURE_MESHES + ('patch5_shared',)
G = 9.81


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from relightableavatar_amd.engine import Engine
    from relightableavatar_amd.evaluators import mesh_evaluator
    e = Engine(make_cfg('relight'), device='cuda:0')          # any context will do: no weights are read
    mesh_evaluator.Evaluator.engine = e
    return e


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(REPO, 'tests', 'golden', 'physx.npz'))


def D(a, dtype=None, dev='cuda:0'):
    t = torch.from_numpy(np.array(a, order='C'))
    return t.to(dev) if dtype is None else t.to(dev, dtype)


def N(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)) if a.size else 0.0


def check(what, err, ref_err):
    b = 10 * max(ref_err, EPS32)
    print(f'{what}: error {err:.2e}, the float32 reference {ref_err:.2e}, ratio {err / max(ref_err, EPS32):.2f} (bound 10)')
    assert err <= b, (what, err, b)


_garments = {}


def garment(eng, golden, name):
    if name not in _garments:
        v, f, vm, fm = (golden[f'{name}/{k}'] for k in ('v', 'f', 'vm', 'fm'))
        _garments[name] = physx_utils.Garment(D(v, torch.float32), D(f), D(vm, torch.float32), D(fm), physx_utils.StVKMaterial(), engine=eng)
    return _garments[name]


def build(eng, v, f, vm=None, fm=None):
    if vm is None:
        vm, fm = P.flatten_faces(v, f)
    return physx_utils.Garment(D(v, torch.float32), D(f), D(vm, torch.float32), D(fm), physx_utils.StVKMaterial(), engine=eng)


# ---------------------------------------------------------------------------------------------- parity with the reference
@pytest.mark.parametrize('name', CASES)
def test_parity(eng, golden, name):
    g = garment(eng, golden, name)
    x = D(golden[f'{name}/x'], torch.float32)
    B = x.shape[0]
    for term, terms in (('stretch', ('stretch',)), ('bending', ('bending',))):
        e, grad = g.cloth.energy(x, terms=terms)
        col = 0 if term == 'stretch' else 1
        want = float(golden[f'{name}/{term}64'])
        check(f'{name} {term}', abs(float(N(e)[:, col].sum()) / B - want) / abs(want), abs(float(golden[f'{name}/{term}32']) - want) / abs(want))
        check(f'{name} {term} gradient', rel(N(grad) / B, golden[f'{name}/{term}_grad64']), rel(golden[f'{name}/{term}_grad32'], golden[f'{name}/{term}_grad64']))
    e, _ = g.cloth.energy(x, terms=('gravity',), gravity=G)
    want = float(golden[f'{name}/gravity64'])
    check(f'{name} gravity', abs(float(N(e)[:, 2].sum()) / B - want) / abs(want), abs(float(golden[f'{name}/gravity32']) - want) / abs(want))
    got = float(physx_utils.gravity_energy(x, g.v_mass, G))
    check(f'{name} gravity_energy', abs(got - want) / abs(want), abs(float(golden[f'{name}/gravity32']) - want) / abs(want))


@pytest.mark.parametrize('name', CASES)
def test_garment_arrays(eng, golden, name):
    g = garment(eng, golden, name)
    for k in ('f_area', 'v_mass', 'Dm_inv', 'Dm'):
        check(f'{name} {k}', rel(N(g[k]), golden[f'{name}/{k}64']), rel(golden[f'{name}/{k}32'], golden[f'{name}/{k}64']))
    mesh = 'patch5' if name == 'patch5_shared' else name
    ev, ef = T.face_connectivity(T.topo(mesh))
    tev, tef = g.topology.face_connectivity()
    assert np.array_equal(N(g.f_connectivity), ef) and np.array_equal(N(g.f_connectivity_edges), ev)
    assert torch.equal(g.f_connectivity, tef) and torch.equal(g.f_connectivity_edges, tev)
    assert np.array_equal(N(g.f_connected_faces), golden[f'{name}/f'][ef])
    assert np.array_equal(np.isinf(N(g.inv_mass)), np.isinf(golden[f'{name}/inv_mass64']))
    finite = np.isfinite(golden[f'{name}/inv_mass64'])
    check(f'{name} inv_mass', rel(N(g.inv_mass)[finite], golden[f'{name}/inv_mass64'][finite]),
          rel(golden[f'{name}/inv_mass32'][finite], golden[f'{name}/inv_mass64'][finite]))
    m = mesh_utils.get_vertex_mass(D(golden[f'{name}/v'], torch.float32), D(golden[f'{name}/f']), 426 * 0.00047, engine=eng)
    assert same_bits(N(m), N(g.v_mass))
    m2 = mesh_utils.get_vertex_mass(D(golden[f'{name}/v'], torch.float32), D(golden[f'{name}/f']), 426 * 0.00047, areas=g.f_area, engine=eng)
    check(f'{name} get_vertex_mass(areas)', rel(N(m2), golden[f'{name}/v_mass64']), rel(golden[f'{name}/v_mass32'], golden[f'{name}/v_mass64']))


def test_unreferenced_vertex(eng, golden):
    g = garment(eng, golden, 'unref')
    unused = np.flatnonzero(golden['unref/v_mass64'] == 0)
    assert len(unused) == 2
    assert (N(g.v_mass)[unused] == 0).all() and np.isposinf(N(g.inv_mass)[unused]).all()
    _, grad = g.cloth.energy(D(golden['unref/x'], torch.float32), terms=('stretch', 'bending', 'gravity'), gravity=G)
    assert (N(grad)[:, unused] == 0).all() and np.isfinite(N(grad)).all()


# ---------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize('name', ('sphere258', 'two', 'fin'))
def test_rows_terms_and_runs_bit_for_bit(eng, golden, name):
    g = garment(eng, golden, name)
    x = D(P.perturbed(golden[f'{name}/v'], 7, 3), torch.float32)
    all3 = ('stretch', 'bending', 'gravity')
    e, grad = g.cloth.energy(x, terms=all3, gravity=G)
    e2, grad2 = g.cloth.energy(x, terms=all3, gravity=G)
    assert same_bits(N(e), N(e2)) and same_bits(N(grad), N(grad2))
    for b in range(3):
        eb, gb = g.cloth.energy(x[b:b + 1].clone(), terms=all3, gravity=G)
        assert same_bits(N(eb)[0], N(e)[b]) and same_bits(N(gb)[0], N(grad)[b]), b
    both, gboth = g.cloth.energy(x, terms=('stretch', 'bending'))
    es, gs = g.cloth.energy(x, terms=('stretch',))
    ebn, gbn = g.cloth.energy(x, terms=('bending',))
    assert same_bits(N(es)[:, 0], N(both)[:, 0]) and same_bits(N(ebn)[:, 1], N(both)[:, 1]) and same_bits(N(both)[:, :2], N(e)[:, :2])
    assert (N(es)[:, 1:] == 0).all() and (N(ebn)[:, [0, 2]] == 0).all()
    assert same_bits(N(gs + gbn), N(gboth))              # each term accumulated on its own, then added
    no_grad, none = g.cloth.energy(x, terms=all3, gravity=G, grad=False)
    assert none is None and same_bits(N(no_grad), N(e))


# ---------------------------------------------------------------------------------------------- edge shapes
@functools.lru_cache(None)
def patches():
    """planar patches (nx, ny, drop, extra unused vertices) whose face, hinge and vertex counts sit one below, at and one above a
    workgroup's worth.  A one-row strip has an odd hinge count whatever is dropped, so two-row patches are searched as well."""
    tile = _lib.lib().ra_cloth_tile(0)
    assert tile == _lib.lib().ra_cloth_tile(1) == _lib.lib().ra_cloth_tile(2)
    found = {}
    shapes = [(n + 1, 2) for n in range(tile // 2 - 4, tile // 2 + 5)] + [(m + 1, 3) for m in range(tile // 5 - 2, tile // 5 + 4)]
    for nx, ny in shapes:
        for drop in range(0, 3):
            F, H, V = P.patch_counts(nx, ny, drop)
            for which, count in (('F', F), ('H', H)):
                if abs(count - tile) <= 1:
                    found.setdefault((which, count - tile), (nx, ny, drop, 0))
            for extra in (0, 1):
                if abs(V + extra - tile) <= 1:
                    found.setdefault(('V', V + extra - tile), (nx, ny, drop, extra))
    assert len(found) == 9, found
    return found


@pytest.mark.parametrize('which', ('F', 'H', 'V'))
@pytest.mark.parametrize('off', (-1, 0, 1))
def test_edge_shapes(eng, which, off):
    tile = _lib.lib().ra_cloth_tile(0)
    nx, ny, drop, extra = patches()[(which, off)]
    v, f = P.grid_patch(nx, ny, drop, extra)
    ref = P.garment(v, f, *P.flatten_faces(v, f))
    counts = dict(F=len(f), H=len(ref['f_connectivity']), V=len(v))
    assert counts[which] == tile + off
    g = build(eng, v, f)
    assert np.array_equal(N(g.f_connectivity), ref['f_connectivity'])
    x = P.perturbed(v, 31 + off, 2, amp=0.01)            # B = 2: B x count crosses a workgroup boundary inside a row
    x32 = x.astype(np.float32)
    e, grad = g.cloth.energy(D(x32), terms=('stretch', 'bending', 'gravity'), gravity=G)
    es, gs = P.stretch(x, ref)
    eb, gb = P.bending(x, ref)
    eg, gg = P.gravity(x, ref['v_mass'], G)
    # the float32 yardstick: the same garment and energies in float32 on the CPU, from the float32 inputs the device gets (the rest
    # areas of a grid whose coordinates reach 13 at a spacing of 0.1 carry the inputs' rounding, whoever computes them)
    t32 = P.torch_garment(P.garment(v, f, *P.flatten_faces(v, f), dtype=np.float32), 'cpu', torch.float32)
    for col, (term, want, gwant) in enumerate((('stretch', es, gs), ('bending', eb, gb), ('gravity', eg, gg))):
        sel = dict(stretch=term == 'stretch', bending=term == 'bending', gravity=term == 'gravity', g=G)
        a = torch.from_numpy(x32.copy()).requires_grad_()
        y = P.torch_energy(a, t32, **sel)
        y.backward()
        check(f'{which}{off:+d} {term}', rel(N(e)[:, col].sum(), want.sum()), abs(float(y.detach()) * 2 - want.sum()) / abs(want.sum()))
        one, gone = g.cloth.energy(D(x32), terms=(term,), gravity=G)
        check(f'{which}{off:+d} {term} gradient', rel(N(gone), gwant), rel(a.grad.numpy() * 2, gwant))
    assert same_bits(N(e)[0], N(g.cloth.energy(D(x32[:1]), terms=('stretch', 'bending', 'gravity'), gravity=G)[0])[0])


@pytest.mark.parametrize('faces', ([[0, 1, 2]], [[0, 1, 2], [2, 3, 4]]), ids=('one_triangle', 'shared_vertex'))
def test_no_hinges(eng, faces):
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0.2, 0.9, 0.1], [-0.5, 1.5, 0.3], [0.6, 1.7, -0.2]], dtype=np.float64)[:max(max(faces)) + 1]
    f = np.asarray(faces, dtype=np.int64)
    g = build(eng, v, f)
    assert g.f_connectivity.shape == (0, 2) and g.f_connectivity_edges.shape == (0, 2)
    x = P.perturbed(v, 3, 2).astype(np.float32)
    e, grad = g.cloth.energy(D(x), terms=('stretch', 'bending'))
    ref = P.garment(v, f, *P.flatten_faces(v, f))
    es, gs = P.stretch(x.astype(np.float64), ref)
    assert (N(e)[:, 1] == 0).all()
    assert rel(N(e)[:, 0], es) <= 100 * EPS32 and rel(N(grad), gs) <= 100 * EPS32
    eb, gb = g.cloth.energy(D(x), terms=('bending',))
    assert (N(eb) == 0).all() and (N(gb) == 0).all()


def test_no_faces(eng):
    """a topology of vertices without faces is a valid, empty garment: massless vertices, every energy 0 but none a failed launch"""
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0.2, 0.9, 0.1]], dtype=np.float64)
    g = build(eng, v, np.zeros((0, 3), dtype=np.int64))
    assert g.f_area.shape == (0,) and g.Dm_inv.shape == (0, 2, 2) and g.f_connectivity.shape == (0, 2)
    assert (N(g.v_mass) == 0).all() and np.isposinf(N(g.inv_mass)).all()
    e, grad = g.cloth.energy(D(P.perturbed(v, 3, 2), torch.float32), terms=('stretch', 'bending', 'gravity'), gravity=G)
    assert (N(e) == 0).all() and (N(grad) == 0).all()


# ---------------------------------------------------------------------------------------------- invariants
def test_rigid_motion_keeps_the_rest_stretch(eng, golden):
    name = 'sphere66'
    g = garment(eng, golden, name)
    v = golden[f'{name}/v']
    cz, sz, cx, sx = np.cos(0.7), np.sin(0.7), np.cos(-1.1), np.sin(-1.1)
    R = np.asarray([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.asarray([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    moved = v @ R.T + np.asarray([0.3, -0.2, 0.5])
    e_rest = float(N(g.cloth.energy(D(v[None], torch.float32), terms=('stretch',))[0])[0, 0])
    e_moved = float(N(g.cloth.energy(D(moved[None], torch.float32), terms=('stretch',))[0])[0, 0])
    # the rule: the rest value is what the det + 2^-23 of Dm_inv leaves (5e-10 here, not 0); the reference's own float32 run of it is
    # the yardstick, for the moved positions as for the rest ones
    want, ref32 = float(golden[f'{name}/rest_stretch64']), float(golden[f'{name}/rest_stretch32'])
    check(f'{name} rest stretch', abs(e_rest - want) / want, abs(ref32 - want) / want)
    check(f'{name} rest stretch after a rigid motion', abs(e_moved - want) / want, abs(ref32 - want) / want)


def test_flat_patch_has_no_bending(eng):
    v, f = P.grid_patch(9, 7)
    g = build(eng, v, f)
    e, grad = g.cloth.energy(D(np.stack([v, v + 0.25]), torch.float32), terms=('bending',))
    assert (N(e) == 0).all() and (N(grad) == 0).all()


def test_gravity_gradient_is_exact(eng, golden):
    g = garment(eng, golden, 'fan40')
    x = D(golden['fan40/x'], torch.float32)
    _, grad = g.cloth.energy(x, terms=('gravity',), gravity=G)
    want = np.zeros((1, len(golden['fan40/v']), 3), dtype=np.float32)
    want[0, :, 1] = np.float32(G) * N(g.v_mass)
    assert same_bits(N(grad), want)


# ---------------------------------------------------------------------------------------------- inertia
@pytest.mark.parametrize('name', ('sphere66', 'unref'))
def test_inertia_terms(eng, golden, name):
    g = garment(eng, golden, name)
    seq, dt = golden[f'{name}/seq'], float(golden['delta_t'])
    xn, xc, vc = seq[:, 2], seq[:, 1], (seq[:, 1] - seq[:, 0]) / dt
    for term, fun in (('inertia', physx_utils.inertia_term), ('dynamic', physx_utils.dynamic_term)):
        a, b, c = (D(t, torch.float32).requires_grad_() for t in (xn, xc, vc))
        val = fun(a, b, c, g.v_mass, dt, engine=eng)
        val.backward()
        want = float(golden[f'{name}/{term}64'])
        check(f'{name} {term}', abs(float(val.detach()) - want) / want, abs(float(golden[f'{name}/{term}32']) - want) / want)
        for t, key in ((a, 'g_next'), (b, 'g_curr'), (c, 'g_vel')):
            check(f'{name} {term} {key}', rel(N(t.grad), golden[f'{name}/{term}_{key}64']), rel(golden[f'{name}/{term}_{key}32'], golden[f'{name}/{term}_{key}64']))
    # NULL gradient outputs
    value, gn, gc, gv = eng.cloth_inertia(g.v_mass, D(xn, torch.float32), D(xc, torch.float32), D(vc, torch.float32), dt, grads=(False, False, False))
    assert gn is None and gc is None and gv is None
    full = eng.cloth_inertia(g.v_mass, D(xn, torch.float32), D(xc, torch.float32), D(vc, torch.float32), dt)
    assert same_bits(N(value), N(full[0]))
    check(f'{name} inertia rows', rel(N(value), P.inertia(xn, xc, vc, golden[f'{name}/v_mass64'], dt)[0]),
          abs(float(golden[f'{name}/inertia32']) - float(golden[f'{name}/inertia64'])) / float(golden[f'{name}/inertia64']))
    # the sequence: the reference's run at B = 1, and both sequences against the restatement
    s = D(seq[:1], torch.float32).requires_grad_()
    val = physx_utils.inertia_term_sequence(s, g.v_mass, dt)
    val.backward()
    want = float(golden[f'{name}/sequence64'])
    check(f'{name} sequence', abs(float(val.detach()) - want) / want, abs(float(golden[f'{name}/sequence32']) - want) / want)
    check(f'{name} sequence gradient', rel(N(s.grad), golden[f'{name}/sequence_grad64']), rel(golden[f'{name}/sequence_grad32'], golden[f'{name}/sequence_grad64']))
    val2 = physx_utils.inertia_term_sequence(D(seq, torch.float32), g.v_mass, dt)
    parts = P.sequence_parts(seq, dt)
    want2 = P.inertia(*parts, golden[f'{name}/v_mass64'], dt)[0].sum() / len(parts[0])
    check(f'{name} sequence at B = 2', abs(float(val2) - want2) / want2, abs(float(golden[f'{name}/sequence32']) - want) / want)


# ---------------------------------------------------------------------------------------------- autograd and the drape
def test_autograd_scales_the_library_gradient(eng, golden):
    g = garment(eng, golden, 'sphere66')
    x = D(golden['sphere66/x'], torch.float32).requires_grad_()
    physx_utils.stretch_energy(x, g).backward()
    _, grad = g.cloth.energy(x.detach(), terms=('stretch',))
    assert same_bits(N(x.grad), N(grad * torch.tensor(0.5, dtype=torch.float32, device=grad.device)))
    y = D(golden['sphere66/x'], torch.float32).requires_grad_()
    total, per = physx_utils.cloth_energy(y, g, stretch=True, bending=True, gravity=True, per_term=True)
    (2 * total).backward()
    e, grad = g.cloth.energy(y.detach(), terms=('stretch', 'bending', 'gravity'))
    assert same_bits(N(per), N(e)) and same_bits(N(y.grad), N(grad))
    assert abs(float(total.detach()) - float(N(e).sum()) / 2) <= 2 * EPS32 * abs(float(total.detach()))
    b = float(physx_utils.bending_energy(y.detach(), g))
    assert abs(b - float(N(e)[:, 1].sum()) / 2) <= 2 * EPS32 * b


def drape(eng, golden):
    g = garment(eng, golden, 'sphere66')
    x = D(golden['sphere66/x'][:1], torch.float32).clone().requires_grad_()
    opt = largesteps.AdamUniform([x], lr=1e-3, engine=eng)
    pinned = [0, 1, 2]
    first = None
    for _ in range(50):
        opt.zero_grad()
        loss = physx_utils.cloth_energy(x, g, stretch=True, bending=True, gravity=True)
        first = float(loss.detach()) if first is None else first
        loss.backward()
        x.grad[:, pinned] = 0
        opt.step()
    last = float(physx_utils.cloth_energy(x.detach(), g, stretch=True, bending=True, gravity=True))
    return first, last, N(x)


def test_drape_end_to_end(eng, golden):
    first, last, x = drape(eng, golden)
    first2, last2, x2 = drape(eng, golden)
    print(f'drape: energy {first:.6e} -> {last:.6e} after 50 AdamUniform steps')
    assert last < first and np.isfinite(x).all()
    assert same_bits(x, x2) and first == first2 and last == last2
    assert same_bits(x[0, :3], golden['sphere66/x'][0, :3].astype(np.float32))       # the pinned vertices did not move


# ---------------------------------------------------------------------------------------------- argument checks
def test_argument_checks(eng, golden):
    L, ctx, s = eng.lib, eng.ctx, eng.stream
    g = garment(eng, golden, 'octa')
    topo, cloth = g.topology._handle, g.cloth._handle
    v, vm, fm = D(golden['octa/v'], torch.float32), D(golden['octa/vm'], torch.float32), D(golden['octa/fm'], torch.int32)
    x = D(golden['octa/x'], torch.float32)
    energy = torch.full((1, 3), 7.0, dtype=torch.float64, device='cuda:0')
    grad = torch.full_like(x, 7.0)
    mat = _lib.ra_cloth_material(*[d for _, d in _lib.CLOTH_MATERIAL_DEFAULTS])
    out = C.c_void_p()
    P_ = lambda t: C.c_void_p(t.data_ptr())

    def refused(rc, text):
        assert rc != 0 and text in L.ra_last_error().decode(), (rc, L.ra_last_error())
        torch.cuda.synchronize()
        assert (energy == 7.0).all() and (grad == 7.0).all()         # nothing was launched into the outputs

    refused(L.ra_cloth_energy(ctx, None, P_(x), 1, 3, 9.81, P_(energy), P_(grad), s), 'null argument')
    refused(L.ra_cloth_energy(ctx, cloth, P_(x), 0, 3, 9.81, P_(energy), P_(grad), s), 'bad sizes')
    refused(L.ra_cloth_energy(ctx, cloth, P_(x), -2, 3, 9.81, P_(energy), P_(grad), s), 'bad sizes')
    refused(L.ra_cloth_energy(ctx, cloth, P_(x), 1, 8, 9.81, P_(energy), P_(grad), s), 'bad terms')
    refused(L.ra_cloth_energy(ctx, cloth, P_(x), 1, 0, 9.81, P_(energy), P_(grad), s), 'bad terms')
    refused(L.ra_cloth_energy(ctx, cloth, P_(x), 1, 3, float('nan'), P_(energy), P_(grad), s), 'bad gravity')
    refused(L.ra_cloth_energy(ctx, topo, P_(x), 1, 3, 9.81, P_(energy), P_(grad), s), 'not a cloth of this ctx')
    refused(L.ra_cloth_create(ctx, topo, P_(v), v.shape[0] + 1, P_(vm), vm.shape[0], P_(fm), C.byref(mat), C.byref(out), s), 'bad sizes')
    refused(L.ra_cloth_create(ctx, None, P_(v), v.shape[0], P_(vm), vm.shape[0], P_(fm), C.byref(mat), C.byref(out), s), 'null argument')
    refused(L.ra_cloth_create(ctx, topo, P_(v), v.shape[0], P_(vm), vm.shape[0] - 1, P_(fm), C.byref(mat), C.byref(out), s), 'material index')
    bad_fm = fm.clone()
    bad_fm[3, 1] = -1
    refused(L.ra_cloth_create(ctx, topo, P_(v), v.shape[0], P_(vm), vm.shape[0], P_(bad_fm), C.byref(mat), C.byref(out), s), 'material index')
    nan_mat = _lib.ra_cloth_material(*[d for _, d in _lib.CLOTH_MATERIAL_DEFAULTS])
    nan_mat.thickness = float('nan')
    refused(L.ra_cloth_create(ctx, topo, P_(v), v.shape[0], P_(vm), vm.shape[0], P_(fm), C.byref(nan_mat), C.byref(out), s), 'bad material')
    assert not out.value
    refused(L.ra_cloth_array(ctx, cloth, 9, P_(grad), s), 'unknown array')
    refused(L.ra_cloth_inertia(ctx, P_(g.v_mass), P_(x), P_(x), P_(x), 0, 6, 0.03, None, P_(energy), None, None, None, s), 'bad sizes')
    refused(L.ra_cloth_inertia(ctx, P_(g.v_mass), P_(x), P_(x), P_(x), 1, 6, 0.0, None, P_(energy), None, None, None, s), 'bad delta_t')
    refused(L.ra_cloth_inertia(ctx, None, P_(x), P_(x), P_(x), 1, 6, 0.03, None, P_(energy), None, None, None, s), 'null argument')
    refused(L.ra_topo_destroy(ctx, topo), 'still reads this topology')
    with pytest.raises(ValueError):
        g.cloth.energy(x[:, :-1])

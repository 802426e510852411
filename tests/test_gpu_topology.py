"""ra_topo_create, ra_topo_array, ra_mesh_smooth, ra_mesh_subdivide, ra_topo_dilate, Engine.topology and the connectivity helpers of
mesh_utils on the device.  Run with `-m gpu` on an MI355X.

No tolerance is chosen here.  Every integer array equals the numpy restatement (tests/topology_ref.py), which
tests/test_oracle_topology.py pins to the reference's own outputs; the smoothed rows equal the restatement's float32 result BIT FOR
BIT, for 1, 2 and 90 iterations, 1, 3, 4 and 55 channels, with a row subset and without, twice; so do the subdivided rows of up to
three chained Loop steps, given the library's own coefficient table, and the child topologies' arrays equal the restatement's
index arithmetic.  Every test prints its figures before it asserts."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import mesh_extract_ref as X
import topology_ref as T
from relightableavatar_amd import _lib, mesh_utils
from relightableavatar_amd._lib import RaError
from relightableavatar_amd.config import make_cfg

pytestmark = pytest.mark.gpu
NAMES = tuple(T.MESHES)
# (channels, iterations, with a row subset)
SMOOTH = ((3, 1, False), (3, 2, False), (3, 90, False), (3, 90, True), (1, 2, True), (1, 90, False), (4, 1, True), (4, 90, False), (55, 2, False), (55, 90, True))


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from relightableavatar_amd.engine import Engine
    return Engine(make_cfg('relight'), device='cuda:0')          # any context will do: no weights are read


def D(a, dev='cuda:0'):
    return torch.from_numpy(np.array(a, order='C')).to(dev)       # a copy: the shared arrays are read-only


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(None)
def values(name, C):
    """(V, C) float32: the positions, then seeded further channels (or the first C coordinates)"""
    v, _ = T.mesh(name)
    extra = np.random.default_rng(17).uniform(0, 1, (len(v), max(C - 3, 0)))
    out = np.ascontiguousarray(np.concatenate([v, extra], axis=1)[:, :C], dtype=np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(None)
def want_smooth(name, C, iters, sub):
    return T.taubin(values(name, C), T.topo(name), T.smooth_inds(name) if sub else None, 0.33, iters, np.float32)


def make(eng, name):
    v, f = T.mesh(name)
    return eng.topology(D(f.astype(np.int32)), len(v))


@pytest.mark.parametrize('name', NAMES)
def test_arrays_equal_the_restatement(eng, name):
    want, (v, f) = T.topo(name), T.mesh(name)
    topo = make(eng, name)
    print(f'{name}: V {topo.V} F {topo.F} E {topo.E} (want {want["E"]}) valence {topo.max_valence} outgoing {topo.max_outgoing} read-backs {topo.readbacks}')
    assert (topo.F, topo.V, topo.E, topo.HE) == (len(f), len(v), want['E'], 3 * len(f))
    assert (topo.max_valence, topo.max_outgoing, topo.readbacks) == (want['max_valence'], want['max_outgoing'], 1)
    for k in _lib.RA_TOPO_ARRAYS:
        got = topo.array(k)
        assert got.dtype == torch.int64 and got.is_cuda
        same = np.array_equal(got.cpu().numpy(), want[k].reshape(-1))
        print(f'{name}: {k} equal {same} ({got.numel()} entries)')
        assert same, k
    assert topo.array('twin', torch.int32).dtype == torch.int32
    he = topo.halfedge
    assert (he.HE, he.E, he.F, he.V) == (topo.HE, topo.E, topo.F, topo.V) and he.verts is None
    assert np.array_equal(he.twin.cpu().numpy(), want['twin']) and np.array_equal(he.vert.cpu().numpy(), f.reshape(-1)) and np.array_equal(he.edge.cpu().numpy(), want['edge'])
    assert topo.edges.shape == (topo.E, 2) and np.array_equal(topo.edges.cpu().numpy(), want['edges']) and np.array_equal(topo.edge_counts.cpu().numpy(), want['edge_counts'])
    ev, cf = topo.face_connectivity()
    wev, wcf = T.face_connectivity(want)
    assert np.array_equal(ev.cpu().numpy(), wev) and np.array_equal(cf.cpu().numpy(), wcf)
    # a second build of the same faces: the same arrays (the filling order of the lists does not show)
    again = make(eng, name)
    for k in _lib.RA_TOPO_ARRAYS:
        assert torch.equal(again.array(k), topo.array(k)), k
    again.close(), topo.close()


@pytest.mark.parametrize('name', NAMES)
def test_smooth_equals_the_float32_restatement_bit_for_bit(eng, name):
    topo = make(eng, name)
    for Cn, iters, sub in SMOOTH:
        if name == 'sphere1026' and (Cn, iters) not in ((3, 90), (55, 2)):
            continue
        src = D(values(name, Cn))
        keep = src.clone()
        inds = D(T.smooth_inds(name)) if sub else None
        got = topo.smooth(src, inds, 0.33, iters)
        want = torch.from_numpy(want_smooth(name, Cn, iters, sub))
        diff = (got.cpu().double() - want.double()).abs().max().item()
        same = bool(torch.equal(bits(got), bits(want)))
        print(f'{name}: C {Cn} iter {iters} inds {sub}: bit-equal {same}, max |diff| {diff:.3e}')
        assert got.shape == (topo.V, Cn) and got.dtype == torch.float32 and got.data_ptr() != src.data_ptr()
        assert same, (name, Cn, iters, sub)
        assert torch.equal(src, keep), 'the input is not modified'
        assert torch.equal(bits(topo.smooth(src, inds, 0.33, iters)), bits(got)), 'twice'
        if sub and iters == 90:      # a bool mask names the same rows
            mask = torch.zeros(topo.V, dtype=torch.bool, device='cuda:0')
            mask[inds] = True
            assert torch.equal(bits(topo.smooth(src, mask, 0.33, iters)), bits(got))
    if name == 'octa':
        flat = topo.smooth(D(values(name, 1)).reshape(-1), None, 0.33, 2)
        assert flat.shape == (topo.V,) and torch.equal(bits(flat), bits(torch.from_numpy(want_smooth(name, 1, 2, False)).reshape(-1)))
        assert torch.equal(topo.smooth(D(values(name, 3)), None, 0.33, 0), D(values(name, 3)))
        assert torch.equal(topo.smooth(D(values(name, 3)), torch.zeros(0, dtype=torch.long), 0.33, 3), D(values(name, 3))), 'an empty subset moves nothing'
        neg = topo.smooth(D(values(name, 3)), torch.tensor([-1, 0]), 0.33, 2)
        assert torch.equal(bits(neg), bits(torch.from_numpy(T.taubin(values(name, 3), T.topo(name), np.array([5, 0]), 0.33, 2))))
    topo.close()


def test_workgroup_edges(eng):
    """(vertex, channel) counts below, at and above one workgroup of the smoothing kernel, and vertex counts around the build's"""
    L = eng.lib
    sb, bb = L.ra_topo_tile(1), L.ra_topo_tile(0)
    assert sb == 256 and bb == 256 and L.ra_topo_tile(2) == 64
    totals = sorted(len(T.mesh(n)[0]) * c for n in ('v63', 'v64', 'v65') for c in (4,))
    assert totals == [sb - 4, sb, sb + 4]
    assert {len(T.mesh(n)[0]) for n in ('v255', 'v256', 'v257')} == {bb - 1, bb, bb + 1}
    for name in ('v63', 'v64', 'v65', 'v255', 'v256', 'v257'):
        topo = make(eng, name)
        got = topo.smooth(D(values(name, 4)), None, 0.33, 2)
        assert torch.equal(bits(got), bits(torch.from_numpy(want_smooth(name, 4, 2, False)))), name
        topo.close()


def test_dilate(eng):
    for name in ('patch5', 'two', 'unref', 'repeat'):
        want, topo = T.topo(name), make(eng, name)
        V = topo.V
        m0 = np.zeros(V, dtype=bool)
        m0[[0, V // 2]] = True
        for steps in (0, 1, 2, 5, -1, -3):
            m = ~m0 if steps < 0 else m0.copy()
            for _ in range(abs(steps)):
                m = np.array([m[want['nbr'][want['nbr_start'][v]:want['nbr_start'][v + 1]]].any() for v in range(V)])
            m = ~m if steps < 0 else m
            got = topo.dilate(D(m0), steps)
            print(f'{name}: dilate {steps}: {int(got.sum())} set, want {int(m.sum())}')
            assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), m), (name, steps)
        topo.close()


def test_empty_topologies(eng):
    for V in (0, 5):
        topo = eng.topology(torch.zeros(0, 3, dtype=torch.int32), V)
        assert (topo.F, topo.V, topo.E, topo.max_valence, topo.max_outgoing, topo.readbacks) == (0, V, 0, 0, 0, 0)
        assert topo.edges.shape == (0, 2) and topo.array('nbr_start').tolist() == [0] * (V + 1) and topo.array('edge_he_start').tolist() == [0]
        ev, cf = topo.face_connectivity()
        assert ev.shape == cf.shape == (0, 2)
        x = torch.arange(V * 3, dtype=torch.float32, device='cuda:0').reshape(V, 3) + 1
        got = topo.smooth(x, None, 0.33, 1)
        want = T.taubin(x.cpu().numpy(), T.halfedge_build(np.zeros((0, 3), dtype=np.int64), V), None, 0.33, 1)
        assert torch.equal(bits(got), bits(torch.from_numpy(want).reshape(V, 3)))
        assert not topo.dilate(torch.ones(V, dtype=torch.bool), 1).any()
        topo.close()


def test_errors_and_ownership(eng):
    from relightableavatar_amd.engine import Engine
    L, null = eng.lib, None
    v, f = T.mesh('octa')
    faces = D(f.astype(np.int32))
    h = C.c_void_p()

    def err(rc, text):
        msg = L.ra_last_error().decode()
        print(rc, msg)
        assert rc != 0 and text in msg, (text, msg)

    p = lambda t: C.c_void_p(t.data_ptr())
    err(L.ra_topo_create(eng.ctx, p(faces), 8, 6, None, eng.stream), 'null argument')
    err(L.ra_topo_create(None, p(faces), 8, 6, C.byref(h), eng.stream), 'null argument')
    err(L.ra_topo_create(eng.ctx, None, 8, 6, C.byref(h), eng.stream), 'null argument')
    err(L.ra_topo_create(eng.ctx, p(faces), -1, 6, C.byref(h), eng.stream), 'bad sizes')
    err(L.ra_topo_create(eng.ctx, p(faces), 8, 0, C.byref(h), eng.stream), 'bad sizes')
    err(L.ra_topo_create(eng.ctx, p(faces), 8, 5, C.byref(h), eng.stream), 'face index')
    bad = faces.clone()
    bad[3, 1] = -1
    err(L.ra_topo_create(eng.ctx, p(bad), 8, 6, C.byref(h), eng.stream), 'face index')
    assert not h.value
    with pytest.raises(RaError, match='face index'):
        eng.topology(bad, 6)
    topo = eng.topology(faces, 6)
    x, out = D(values('octa', 3)), torch.empty(6, 3, device='cuda:0')
    sm = lambda *a: L.ra_mesh_smooth(eng.ctx, *a, eng.stream)
    err(sm(None, p(x), 6, 3, None, 0, 0.33, 1, p(out)), 'null argument')
    err(sm(topo._handle, None, 6, 3, None, 0, 0.33, 1, p(out)), 'null argument')
    err(sm(topo._handle, p(x), 6, 3, None, 0, 0.33, 1, None), 'null argument')
    err(sm(topo._handle, p(x), 6, 3, None, 0, 0.33, 1, p(x)), 'null argument')
    for args in ((5, 3, None, 0, 0.33, 1), (6, 0, None, 0, 0.33, 1), (6, 65, None, 0, 0.33, 1), (6, 3, None, 0, 0.33, -1), (6, 3, None, 2, 0.33, 1)):
        err(sm(topo._handle, p(x), *args, p(out)), 'bad sizes')
    err(sm(topo._handle, p(x), 6, 3, None, 0, float('nan'), 1, p(out)), 'bad alpha')
    err(L.ra_topo_array(eng.ctx, topo._handle, 11, p(out), eng.stream), 'unknown array')
    err(L.ra_topo_array(eng.ctx, topo._handle, 0, None, eng.stream), 'null argument')
    err(L.ra_topo_sizes(eng.ctx, topo._handle, None), 'null argument')
    m = torch.ones(6, dtype=torch.uint8, device='cuda:0')
    err(L.ra_topo_dilate(eng.ctx, topo._handle, p(m), 6, 1, p(m), eng.stream), 'null argument')
    err(L.ra_topo_dilate(eng.ctx, topo._handle, p(m), 5, 1, p(m.clone()), eng.stream), 'bad sizes')
    # out-of-range row indices name no row
    far = topo.smooth(x, torch.tensor([0, 6, 10 ** 12]), 0.33, 2)
    assert torch.equal(bits(far), bits(torch.from_numpy(T.taubin(values('octa', 3), T.topo('octa'), np.array([0]), 0.33, 2))))
    with pytest.raises(ValueError):
        topo.smooth(torch.zeros(5, 3))
    with pytest.raises(ValueError):
        topo.dilate(torch.zeros(5, dtype=torch.bool), 1)
    # a topology belongs to its ctx
    other = Engine(make_cfg('relight'), device='cuda:0')
    err(L.ra_mesh_smooth(other.ctx, topo._handle, p(x), 6, 3, None, 0, 0.33, 1, p(out), other.stream), 'not a topology of this ctx')
    err(L.ra_topo_destroy(other.ctx, topo._handle), 'not a topology of this ctx')
    err(L.ra_topo_sizes(other.ctx, topo._handle, (C.c_int * 7)()), 'not a topology of this ctx')
    assert L.ra_topo_destroy(eng.ctx, None) == 0
    # destroy order: the ctx frees what is left; the handle then only refuses
    orphan = other.topology(faces, 6)
    L.ra_ctx_destroy(other.ctx)
    other.ctx = C.c_void_p()
    with pytest.raises(RaError, match='engine that built this topology is gone'):
        orphan.smooth(x)
    orphan.close()
    topo.close()
    with pytest.raises(RaError, match='closed'):
        topo.smooth(x)
    topo.close()


def test_mesh_utils_against_the_golden(eng):
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'topology.npz'))
    for name in ('octa', 'patch5', 'fin', 'v65', 'repeat'):
        v, f = T.mesh(name)
        tf, tv = D(f), D(v.astype(np.float32))
        e, i, c = mesh_utils.get_edges(tf, engine=eng)
        ref_e = golden[f'{name}/ge_e']
        last = e[:, 1].cpu().numpy() == f.max()
        assert np.array_equal(i.cpu().numpy(), golden[f'{name}/ge_i']) and np.array_equal(c.cpu().numpy(), golden[f'{name}/ge_c'])
        assert np.array_equal(e.cpu().numpy()[~last], ref_e[~last]) and last.any() and not np.array_equal(e.cpu().numpy()[last], ref_e[last])
        assert np.array_equal(e.cpu().numpy(), T.topo(name)['edges'])
        he = mesh_utils.triangle_to_halfedge(tv, tf, engine=eng)
        for k in ('twin', 'vert', 'edge'):
            assert he[k].dtype == torch.int64 and np.array_equal(he[k].cpu().numpy(), golden[f'{name}/he_{k}']), k
        assert (he.E, he.V, he.F, he.HE) == (int(golden[f'{name}/he_E']), len(v), len(f), 3 * len(f)) and he.verts is tv
        assert mesh_utils.triangle_to_halfedge(None, tf, engine=eng).V == int(f.max())
        ev, cf = mesh_utils.get_face_connectivity(tf, engine=eng)
        big = len(f) + 1
        assert np.array_equal(np.sort((ev * big + cf).cpu().numpy(), axis=1), np.sort(golden[f'{name}/fc_edges'] * big + golden[f'{name}/fc_faces'], axis=1))
        for case, inds in (('90', None), ('90_inds', D(T.smooth_inds(name)))):
            keep = tv.clone()
            got = mesh_utils.laplacian_smoothing(tv, e, inds)
            assert torch.equal(tv, keep) and got.data_ptr() != tv.data_ptr(), 'a new tensor'
            assert torch.equal(bits(got), bits(torch.from_numpy(want_smooth(name, 3, 90, inds is not None))))
            gold = golden[f'{name}/smooth{case}']
            d = np.abs(got.cpu().numpy().astype(np.float64) - gold).max()
            print(f'{name}/{case}: device vs the reference\'s float32 max |diff| {d:.3e}')
        with pytest.raises(ValueError, match='get_edges returned'):
            mesh_utils.laplacian_smoothing(tv, e.clone())
    with pytest.raises(ValueError):
        mesh_utils.get_edges(torch.zeros(4, 3), engine=eng)


def test_extract_smooth_measure_end_to_end(eng):
    """marching cubes -> largest component -> topology -> 10 Taubin iterations on the 24^3 sphere volume of the extraction tests; the
    smoothed mesh goes to Engine.mesh: every vertex stays within one voxel of the analytic sphere, and so does the closest point of
    the smoothed surface to every extracted vertex"""
    Rr, centre = X.SPHERE['R'], torch.tensor(X.SPHERE['centre'], dtype=torch.float32, device='cuda:0')
    v, f = eng.largest_component(*eng.marching_cubes(D(X.sphere_volume()), 0.0))
    assert f.dtype == torch.int32 and f.is_cuda
    topo = eng.topology(f, v.shape[0])
    assert topo.readbacks == 1 and bool((topo.edge_counts == 2).all()), 'closed and manifold'
    assert topo.V - topo.E + topo.F == 2
    s = topo.smooth(v, iter=10)
    r0, r1 = (v - centre).norm(dim=1), (s - centre).norm(dim=1)
    print(f'V {topo.V} F {topo.F} E {topo.E}: extracted |r - R| max {float((r0 - Rr).abs().max()):.4f}, smoothed {float((r1 - Rr).abs().max()):.4f}')
    assert float((r1 - Rr).abs().max()) <= 1.0
    d2 = eng.mesh(s, f.cpu()).closest(v, want=('d2',)).d2
    print(f'extracted vertices to the smoothed surface: max distance {float(d2.max().sqrt()):.4f}')
    assert float(d2.max().sqrt()) <= 1.0
    topo.close()


# ---------------------------------------------------------------------------------------------- Loop subdivision (ra_mesh_subdivide)
@functools.lru_cache(None)
def library_table(n_max=64):
    """the (w_self, beta) pairs of the library's own table (ra_loop_weights), float32: what the restatement is handed"""
    L = _lib.lib()
    t = np.zeros((n_max + 1, 2), dtype=np.float32)
    for n in range(1, n_max + 1):
        w, b = C.c_float(), C.c_float()
        assert L.ra_loop_weights(n, C.byref(w), C.byref(b)) == 0
        t[n] = (w.value, b.value)
    return t


def loop_depth(name):
    """chained steps per mesh: what the numpy restatement's python loops do in a second or two"""
    n = len(T.mesh(name)[0])
    return 3 if n < 100 else 2 if n < 300 else 1


@functools.lru_cache(None)
def want_loop(name, Cn, steps):
    """[(values, topo)] after every step of the float32 restatement, given the library's table"""
    x, t, out = values(name, Cn), T.topo(name), []
    for _ in range(steps):
        y = T.loop_step(x, t, library_table(), np.float32)
        t = T.child_topology(t, len(x))
        x = y
        out.append((x, t))
    return out


@pytest.mark.parametrize('name', NAMES)
def test_subdivide_equals_the_float32_restatement_bit_for_bit(eng, name):
    root = make(eng, name)
    tab_np = T.loop_table(64, np.float32)
    print(f'library table equals numpy float64 formula rounded once: {np.array_equal(tab_np, library_table())}')
    for Cn in (3, 1, 4, 55):
        steps = loop_depth(name) if Cn == 3 else 1
        topo, x = root, D(values(name, Cn))
        for k, (wx, wt) in enumerate(want_loop(name, Cn, steps)):
            keep = x.clone()
            y, faces, child = topo.subdivide(x)
            same = bool(torch.equal(bits(y), bits(torch.from_numpy(wx))))
            print(f'{name}: C {Cn} step {k + 1}: V {child.V} F {child.F} E {child.E}: bit-equal {same}, max |diff| {float((y.cpu().double() - torch.from_numpy(wx).double()).abs().max()):.3e}')
            assert y.shape == (topo.V + topo.E, Cn) and faces.shape == (4 * topo.F, 3) and faces.dtype == torch.int32
            assert same, (name, Cn, k)
            assert torch.equal(x, keep), 'the input is not modified'
            assert (child.F, child.V, child.E, child.readbacks) == (4 * topo.F, topo.V + topo.E, 2 * topo.E + 3 * topo.F, 0)
            assert np.array_equal(faces.cpu().numpy(), wt['vert'].reshape(-1, 3))
            if Cn == 3:
                for a in _lib.RA_TOPO_ARRAYS:
                    assert np.array_equal(child.array(a).cpu().numpy(), wt[a].reshape(-1)), (name, k, a)
                assert child.max_outgoing == wt['max_outgoing'] and child.max_valence >= wt['max_valence']
                y2, faces2, child2 = topo.subdivide(x)
                assert torch.equal(bits(y2), bits(y)) and torch.equal(faces2, faces) and all(torch.equal(child2.array(a), child.array(a)) for a in _lib.RA_TOPO_ARRAYS), 'twice'
                child2.close()
                if k == 0:      # the child smooths like any topology
                    sm = child.smooth(y, None, 0.33, 2)
                    assert torch.equal(bits(sm), bits(torch.from_numpy(T.taubin(wx, wt, None, 0.33, 2))))
            if topo is not root:
                topo.close()
            topo, x = child, y
        if topo is not root:
            topo.close()
    root.close()


@pytest.mark.parametrize('name', ('octa', 'sphere66', 'patch5', 'two', 'fan40', 'unref', 'v65'))
def test_chained_step_equals_a_fresh_topology_in_corner_positions(eng, name):
    """closed and open manifold meshes: step 2 through the child's arithmetic = step 2 on a topology built from the step-1 faces.
    The edge ids differ (arithmetic against lexicographic), hence the row order; the corner positions are the same bits"""
    root = make(eng, name)
    y1, f1, child = root.subdivide(D(values(name, 3)))
    fresh = eng.topology(f1, y1.shape[0])
    assert torch.equal(fresh.array('twin'), child.array('twin')) and torch.equal(fresh.array('nbr'), child.array('nbr')) and fresh.readbacks == 1
    ya, fa, ca = child.subdivide(y1)
    yb, fb, cb = fresh.subdivide(y1)
    same = torch.equal(bits(ya[fa.long()]), bits(yb[fb.long()]))
    print(f'{name}: chained = fresh in {fa.numel()} corner positions: {same}')
    assert same
    for t in (ca, cb, fresh, child, root):
        t.close()


def test_subdivide_against_the_golden_and_mesh_utils(eng, tmp_path):
    """the device, through mesh_utils' reference-named functions, against the reference's own float32 run under the 10 x rule"""
    from relightableavatar_amd.visualizers.mesh_visualizer import export_mesh
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'topology.npz'))
    for name in ('octa', 'patch5', 'fin', 'fan40', 'repeat', 'unref', 'sphere66'):
        v, f = T.mesh(name)
        v32 = v.astype(np.float32)
        for steps in T.loop_steps(name):
            sv, sf = mesh_utils.loop_subdivision(D(v32), D(f), steps, engine=eng)
            assert sv.dtype == torch.float32 and sf.dtype == torch.int64 and sf.shape == (4 ** steps * len(f), 3)
            faces = golden[f'{name}/loop{steps}_faces'].astype(np.int64)
            assert np.array_equal(sf.cpu().numpy(), faces)
            r64 = T.subdivide(v32, T.topo(name), steps, np.float64)[0]
            ref = np.abs(r64[faces]).max()
            gerr, derr = (np.abs(a.astype(np.float64)[faces] - r64[faces]) / ref for a in (golden[f'{name}/loop{steps}_v32'], sv.cpu().numpy()))
            print(f'{name}/{steps}: reference float32 max {gerr.max():.3e} median {np.median(gerr):.3e}; device max {derr.max():.3e} median {np.median(derr):.3e}')
            assert derr.max() <= 10 * (gerr.max() or 2.0 ** -23) and np.median(derr) <= 10 * (np.median(gerr) or 2.0 ** -23)
        he = mesh_utils.triangle_to_halfedge(D(v32), D(f), engine=eng)
        he2 = mesh_utils.multiple_halfedge_loop_subdivision(he, 1)
        for k in ('twin', 'vert', 'edge'):
            assert he2[k].dtype == torch.int64 and np.array_equal(he2[k].cpu().numpy(), golden[f'{name}/loop1_{k}']), k
        assert (he2.V, he2.E, he2.F, he2.HE) == (he.V + he.E, 2 * he.E + 3 * he.F, 4 * he.F, 4 * he.HE)
        sv, sf = mesh_utils.halfedge_to_triangle(he2)
        assert sv is he2.verts and np.array_equal(sf.cpu().numpy(), golden[f'{name}/loop1_faces'])
    with pytest.raises(ValueError, match='triangle_to_halfedge'):
        mesh_utils.halfedge_loop_subdivision(mesh_utils.triangle_to_halfedge(None, D(T.mesh('octa')[1]), engine=eng))
    v, f = T.mesh('octa')
    path = str(tmp_path / 'octa.npz')
    export_mesh(torch.from_numpy(v.copy()), torch.from_numpy(f.copy()), path, subdivision=2, engine=eng)
    got = np.load(path)
    assert got['verts'].shape == (66, 3) and got['faces'].shape == (128, 3)
    export_mesh(v, f, path)
    assert np.load(path)['faces'].shape == (8, 3)


def test_subdivide_errors(eng):
    from relightableavatar_amd.engine import Engine
    L = eng.lib
    topo = make(eng, 'octa')
    x, out, faces, h = D(values('octa', 3)), torch.empty(18, 3, device='cuda:0'), torch.empty(32, 3, dtype=torch.int32, device='cuda:0'), C.c_void_p()
    p = lambda t: C.c_void_p(t.data_ptr())

    def err(rc, text):
        msg = L.ra_last_error().decode()
        print(rc, msg)
        assert rc != 0 and text in msg, (text, msg)
    sub = lambda *a: L.ra_mesh_subdivide(eng.ctx, *a, eng.stream)
    err(sub(None, p(x), 6, 3, p(out), p(faces), C.byref(h)), 'null argument')
    err(sub(topo._handle, None, 6, 3, p(out), p(faces), C.byref(h)), 'null argument')
    err(sub(topo._handle, p(x), 6, 3, None, p(faces), C.byref(h)), 'null argument')
    err(sub(topo._handle, p(x), 6, 3, p(x), p(faces), C.byref(h)), 'null argument')
    for n, c in ((5, 3), (6, 0), (6, 65)):
        err(sub(topo._handle, p(x), n, c, p(out), p(faces), C.byref(h)), 'bad sizes')
    assert not h.value
    other = Engine(make_cfg('relight'), device='cuda:0')
    err(L.ra_mesh_subdivide(other.ctx, topo._handle, p(x), 6, 3, p(out), p(faces), C.byref(h), other.stream), 'not a topology of this ctx')
    # positions only, and faces without a child (one synchronisation): the same values
    want = topo.subdivide(x)
    assert sub(topo._handle, p(x), 6, 3, p(out), None, None) == 0 and torch.equal(bits(out), bits(want[0]))
    out.zero_()
    assert sub(topo._handle, p(x), 6, 3, p(out), p(faces), None) == 0 and torch.equal(bits(out), bits(want[0])) and torch.equal(faces, want[1])
    with pytest.raises(ValueError):
        topo.subdivide(torch.zeros(5, 3))
    # an empty mesh subdivides to an empty mesh; vertices without faces move to the origin
    empty = eng.topology(torch.zeros(0, 3, dtype=torch.int32), 4)
    y, f2, child = empty.subdivide(torch.ones(4, 2))
    assert y.shape == (4, 2) and not y.any() and f2.shape == (0, 3) and (child.F, child.V, child.E) == (0, 4, 0)
    assert child.array('nbr_start').tolist() == [0] * 5
    # a child outlives its parent; closing order is free
    kid = want[2]
    topo.close()
    y2, _, kid2 = kid.subdivide(want[0])
    assert y2.shape == (66, 3)
    kid.close(), kid2.close(), child.close(), empty.close()


def test_extract_smooth_subdivide_end_to_end(eng):
    """marching cubes -> largest component -> topology -> 10 Taubin iterations -> one Loop step on the 24^3 sphere volume of the
    extraction tests: exactly four times the triangles, every subdivided vertex within one voxel of the analytic sphere, measured
    directly and through Engine.mesh(...).closest against the extracted surface"""
    Rr, centre = X.SPHERE['R'], torch.tensor(X.SPHERE['centre'], dtype=torch.float32, device='cuda:0')
    v, f = eng.largest_component(*eng.marching_cubes(D(X.sphere_volume()), 0.0))
    topo = eng.topology(f, v.shape[0])
    s = topo.smooth(v, iter=10)
    sv, sf, child = topo.subdivide(s)
    assert sf.shape[0] == 4 * f.shape[0] and sv.shape[0] == topo.V + topo.E and child.readbacks == 0
    assert bool((child.edge_counts == 2).all()) and child.V - child.E + child.F == 2, 'still closed, still a sphere'
    r = (sv - centre).norm(dim=1)
    d2 = eng.mesh(v, f.cpu()).closest(sv, want=('d2',)).d2
    print(f'V {child.V} F {child.F}: subdivided |r - R| max {float((r - Rr).abs().max()):.4f}; to the extracted surface max {float(d2.max().sqrt()):.4f}')
    assert float((r - Rr).abs().max()) <= 1.0 and float(d2.max().sqrt()) <= 1.0
    sub_mesh = eng.mesh(sv, sf.cpu())
    assert float(sub_mesh.closest(v, want=('d2',)).d2.max().sqrt()) <= 1.0
    child.close(), topo.close()

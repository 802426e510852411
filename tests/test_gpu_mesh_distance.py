"""ra_mesh_create / ra_mesh_closest, Engine.mesh, mesh_utils and the mesh evaluator on the device.
Run with `-m gpu` on an MI355X.

No tolerance is chosen here.  d2 and sqrt(d2) are held to the project's 10 x float32 rule as DESIGN.md section 15 states it
(frame_stage_ref.parity): max and median |diff| against the float64 reference (tests/mesh_distance_ref.py), normalised by max |ref|, at
most 10 x the float32 restatement's own error on the same inputs; where that is exactly 0, 10 x 2^-23 of max |ref|.  Face ids are never
compared with the reference's (outside a convex body a fifth of the points have a float64 tie): face, closest and bary are checked by
identities evaluated in float64 on what the kernel returned, with bounds counted in fp32 roundings.  The sweep's exactness is bit
equality: default call = RA_MESH_BRUTE = unsorted call = any order of the points = any subset of the points.
Every test prints its figures before it asserts."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

import mesh_distance_ref as M
from frame_stage_ref import parity
from relightableavatar_amd import _lib, mesh_utils, synthetic
from relightableavatar_amd._lib import RaError
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.evaluators import make_evaluator, mesh_evaluator

pytestmark = pytest.mark.gpu
U = 2.0 ** -23
KEYS = ('d2', 'closest', 'face', 'bary')


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from relightableavatar_amd.engine import Engine
    return Engine(make_cfg('relight'), device='cuda:0')          # any context will do: no weights are read


@functools.lru_cache(None)
def hull():
    b = synthetic.make_body(0, posed=False, n_verts=301)
    tv = b.tverts[0].numpy()
    return tv, synthetic._template_faces(tv.astype(np.float64) / (0.4 * np.array([0.8, 0.7, 1.1])))


@functools.lru_cache(None)
def mesh_case(name):
    v, f = hull()
    if name == 'hull':
        return v, f
    if name == 'planar':                       # all z equal: the two hemispheres fall onto each other, a box of no height
        p = v.copy()
        p[:, 2] = 0.25
        return p, f
    if name == 'two':                          # two copies 5 m apart
        return np.concatenate([v, v + np.float32([5, 0, 0])]), np.concatenate([f, f + len(v)])
    if name == 'far':                          # 100 m from the origin
        return v + np.float32([60, -80, 0]), f
    if name == 'degenerate':                   # plus a collinear face and a face of three equal vertices, both outside the hull
        a, b = np.float32([0.5, 0.0, 0.0]), np.float32([0.6, 0.05, 0.02])
        extra = np.stack([a, b, a + np.float32(2) * (b - a), np.float32([0.0, 0.5, 0.3])])
        n = len(v)
        return np.concatenate([v, extra]), np.concatenate([f, [[n, n + 1, n + 2], [n + 3, n + 3, n + 3]]])
    raise KeyError(name)


MESHES = ('hull', 'planar', 'two', 'far', 'degenerate')


@functools.lru_cache(None)
def point_sets(name):
    """near: 1e-4, 1e-2 and 0.3 off the centroids of every 7th face (along the normal, 1e-2 also inwards), points exactly on vertices,
    midpoints of shared edges, and points off the two degenerate faces; vertex: the points on vertices alone; far: one point 1 km away"""
    v, f = mesh_case(name)
    v64 = v.astype(np.float64)
    tri = v64[f[::7]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    ln = np.linalg.norm(nrm, axis=-1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1), [0.0, 0.0, 1.0])
    cen = tri.mean(1)
    on_vertex = v[::5][:40]
    mid = ((v[f[::9, 0]] + v[f[::9, 1]]) * np.float32(0.5))
    near = [cen + s * nrm for s in (1e-4, 1e-2, 0.3, -1e-2)] + [on_vertex, mid]
    if name == 'degenerate':
        seg = v64[-4] + np.linspace(-0.5, 2.5, 13)[:, None] * (v64[-3] - v64[-4])
        near += [seg + [0.0, 0.02, 0.0], v64[-1:] + [[0.0, 0.01, 0.0]], v64[-1:]]
    near = np.concatenate(near).astype(np.float32)
    far = (v64.mean(0, keepdims=True) + [[600.0, 800.0, 0.0]]).astype(np.float32)
    return {'near': near, 'vertex': np.ascontiguousarray(on_vertex), 'far': far}


@functools.lru_cache(None)
def reference(name, group):
    v, f = mesh_case(name)
    p = point_sets(name)[group]
    return M.closest_point(p, v, f, np.float64), M.closest_point(p, v, f, np.float32)


def T(a, dev='cuda:0'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(o):
    return {k: (o[k] if k == 'face' else o[k].view(torch.int32)).cpu() for k in KEYS}


def assert_same_bits(tag, a, b, rows=None):
    a, b = bits(a), bits(b)
    for k in KEYS:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        same = bool(torch.equal(x, y))
        print(f'{tag}: {k} bit-equal {same} ({x.shape[0]} points)')
        assert same, f'{tag}: {k}'


def sqrt_tolerance(r32, r64):
    """the absolute tolerance the rule gives sqrt(d2) on these inputs"""
    s32, s64 = np.sqrt(r32[0].astype(np.float64)), np.sqrt(r64[0])
    e = np.abs(s32 - s64).max()
    return 10 * e if e > 0 else 10 * U * s64.max()


def check_identities(tag, out, p, v, f, r32, r64):
    """face, closest and bary by identities in float64 on the kernel's own outputs"""
    d2, q, face, bary = (out[k].cpu().numpy() for k in KEYS)
    p64, v64, q64, b64 = p.astype(np.float64), v.astype(np.float64), q.astype(np.float64), bary.astype(np.float64)
    assert (face >= 0).all() and (face < len(f)).all() and np.isfinite(d2).all() and np.isfinite(q).all() and np.isfinite(bary).all(), tag
    tol = sqrt_tolerance(r32, r64)
    excess = M.distance_to_face(p64, v64, f, face) - np.sqrt(r64[0])
    rebuilt = (b64[:, :, None] * v64[f[face]]).sum(1)
    coord = np.abs(v64).max()
    e_q = np.abs(q64 - rebuilt).max() / (U * coord)
    e_sum = np.abs(b64.sum(1) - 1).max() / U
    b_min = b64.min() / U
    own = ((p64 - q64) ** 2).sum(1)
    e_d2 = (np.abs(own - d2) / np.where(d2 > 0, U * d2.astype(np.float64), 1))
    e_d2 = np.where(d2 > 0, e_d2, np.where(own == 0, 0, np.inf)).max()
    print(f'{tag}: returned face {excess.max():.3e} above the float64 minimum (allowed {tol:.3e}); |closest - sum bary v| {e_q:.2f} units of '
          f'2^-23 max|coord| (8); |sum bary - 1| {e_sum:.2f} (4); min bary {b_min:.2f} (-4); | |p - closest|^2 - d2 | {e_d2:.2f} units of 2^-23 d2 (4)')
    assert excess.max() <= tol, tag
    assert e_q <= 8 and e_sum <= 4 and b_min >= -4 and e_d2 <= 4, tag


def check_parity(tag, out, r32, r64):
    d2 = out.d2.cpu().numpy()
    parity(f'{tag} d2', d2, r32[0], r64[0])
    parity(f'{tag} sqrt(d2)', np.sqrt(d2.astype(np.float64)), np.sqrt(r32[0].astype(np.float64)), np.sqrt(r64[0]))


# ------------------------------------------------------------------------------------------------ meshes x point sets
@pytest.mark.parametrize('group', ['near', 'far'])
@pytest.mark.parametrize('name', MESHES)
def test_meshes_parity_identities_and_exactness(eng, name, group):
    v, f = mesh_case(name)
    p = point_sets(name)[group]
    r64, r32 = reference(name, group)
    mesh = eng.mesh(T(v), T(f))
    tag = f'{name}/{group} ({len(f)} faces, {len(p)} points)'
    out = mesh.closest(T(p))
    check_parity(tag, out, r32, r64)
    check_identities(tag, out, p, v, f, r32, r64)
    assert_same_bits(f'{tag} default = brute', out, mesh.closest(T(p), brute=True))
    assert_same_bits(f'{tag} default = unsorted', out, mesh.closest(T(p), sort=False))
    assert_same_bits(f'{tag} twice', out, mesh.closest(T(p)))
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(p)))
    assert_same_bits(f'{tag} permuted points', mesh.closest(T(p)[perm.cuda()]), out, rows=(slice(None), perm))
    # a subset of the outputs is the same call
    part = mesh.closest(T(p), want=('face', 'd2'))
    assert set(part) == {'face', 'd2'} and torch.equal(part.face, out.face) and torch.equal(part.d2.view(torch.int32), out.d2.view(torch.int32))
    mesh.close()


@pytest.mark.parametrize('name', MESHES)
def test_points_on_vertices_have_distance_zero(eng, name):
    v, f = mesh_case(name)
    p = point_sets(name)['vertex']
    mesh = eng.mesh(T(v), T(f))
    out = mesh.closest(T(p))
    d2 = out.d2.cpu().numpy()
    print(f'{name}: max d2 of {len(p)} points on vertices {d2.max():.3e}')
    assert (d2 == 0).all() and torch.equal(out.closest.cpu(), torch.from_numpy(p))
    mesh.close()


def test_two_copies_restricted_to_one(eng):
    """points near copy A of the two-copies mesh: the values and face ids of copy A alone"""
    v, f = hull()
    p = point_sets('hull')['near']
    one, two = eng.mesh(T(v), T(f)), eng.mesh(T(mesh_case('two')[0]), T(mesh_case('two')[1]))
    assert_same_bits('two copies vs one', two.closest(T(p)), one.closest(T(p)))
    one.close(), two.close()


def test_tie_rule_lowest_original_index(eng):
    """every face twice: the lower copy wins, whatever order the faces are given in"""
    v, f = hull()
    cen = v.astype(np.float64)[f].mean(1)
    p = (cen * 1.02).astype(np.float32)                           # one nearest face each, 1 % outside its centroid
    alone = eng.mesh(T(v), T(f))
    base = alone.closest(T(p))
    assert (base.face.cpu().numpy() == np.arange(len(f))).all()
    doubled = eng.mesh(T(v), T(np.concatenate([f, f])))
    assert_same_bits('faces twice', doubled.closest(T(p)), base)
    order = np.random.default_rng(5).permutation(len(f))
    shuffled = eng.mesh(T(v), T(np.concatenate([f[order], f])))
    out = shuffled.closest(T(p))
    where = np.argsort(order)                                     # position of original face j in the shuffled block
    want = np.minimum(where, len(f) + np.arange(len(f)))
    print(f'tie rule: {int((out.face.cpu().numpy() == want).sum())} of {len(f)} points answer the lower of their two copies')
    assert (out.face.cpu().numpy() == want).all()
    assert torch.equal(out.d2.view(torch.int32), base.d2.view(torch.int32)) and torch.equal(out.closest.view(torch.int32), base.closest.view(torch.int32))
    # the barycentrics follow the face's own vertex order
    rolled = eng.mesh(T(v), T(np.roll(f, 1, axis=1)))
    r = rolled.closest(T(p))
    rebuilt = (r.bary.cpu().double()[:, :, None] * torch.from_numpy(v.astype(np.float64)[np.roll(f, 1, axis=1)[r.face.cpu().numpy()]])).sum(1)
    assert float((rebuilt - r.closest.cpu().double()).abs().max()) <= 8 * U * np.abs(v).max()
    for m in (alone, doubled, shuffled, rolled):
        m.close()


# ------------------------------------------------------------------------------------------------ shapes
def test_edge_shapes(eng):
    """F around the leaf and group sizes x n around the wave and the sort threshold: parity on the full point set, and every smaller n
    is the prefix of the full call, default and brute (the answer of a point does not depend on its neighbours)"""
    L, G, S = eng.lib.ra_mesh_tile(0), eng.lib.ra_mesh_tile(1), eng.lib.ra_mesh_tile(2)
    v, f = hull()
    assert G * L + 1 <= len(f)
    r = np.random.default_rng(11)
    pool = np.concatenate([point_sets('hull')['near'][:193], r.uniform(-0.6, 0.6, (64, 3)).astype(np.float32)])
    pool = pool[r.permutation(len(pool))]
    assert len(pool) == 257 and 1 <= S < 257          # both sides of the sort threshold are among the n below
    for F in (1, L - 1, L, L + 1, G * L - 1, G * L, G * L + 1):
        mesh = eng.mesh(T(v), T(f[:F]))
        r64, r32 = M.closest_point(pool, v, f[:F], np.float64), M.closest_point(pool, v, f[:F], np.float32)
        full = mesh.closest(T(pool))
        check_parity(f'F = {F}, n = 257', full, r32, r64)
        check_identities(f'F = {F}, n = 257', full, pool, v, f[:F], r32, r64)
        for n in (0, 1, 63, 64, 65, 257):
            for brute in (False, True):
                o = mesh.closest(T(pool[:n]), brute=brute)
                assert all(o[k].shape[0] == n for k in KEYS)
                a, b = bits(o), bits(full)
                same = all(torch.equal(a[k], b[k][:n]) for k in KEYS)
                print(f'F = {F}, n = {n}, brute = {brute}: the prefix of the full call {same}')
                assert same
        mesh.close()


# ------------------------------------------------------------------------------------------------ degenerate inputs
@pytest.mark.parametrize('n', [64, 130])
def test_non_finite_points_do_not_touch_their_wave(eng, n):
    v, f = hull()
    mesh = eng.mesh(T(v), T(f))
    p = point_sets('hull')['near'][:n].copy()
    clean = mesh.closest(T(p))
    bad = p.copy()
    bad[17] = [np.nan, 0.1, 0.2]
    bad[40, 2] = np.inf
    bad[41] = -np.inf
    others = np.setdiff1d(np.arange(n), [17, 40, 41])
    for brute in (False, True):
        o = mesh.closest(T(bad), brute=brute)
        for k in ('d2', 'closest', 'bary'):
            assert bool(torch.isnan(o[k][[17, 40, 41]]).all()), k
        assert o.face[[17, 40, 41]].tolist() == [-1, -1, -1]
        assert_same_bits(f'n = {n}, brute = {brute}: the finite points beside NaN / inf points', o, clean, rows=(others, others))
    mesh.close()


def test_faces_with_non_finite_vertices_are_dropped(eng):
    v, f = hull()
    p = point_sets('hull')['near']
    bad = v.copy()
    bad[f[7, 1]] = np.nan
    bad[f[300, 0], 1] = np.inf
    touched = (f == f[7, 1]).any(1) | (f == f[300, 0]).any(1)
    kept = np.nonzero(~touched)[0]
    holed, cut = eng.mesh(T(bad), T(f)), eng.mesh(T(v), T(f[kept]))
    a, b = holed.closest(T(p)), cut.closest(T(p))
    print(f'{int(touched.sum())} faces dropped; answers among the other {len(kept)}')
    assert torch.equal(a.face.cpu(), torch.from_numpy(kept)[b.face.cpu().long()])
    for k in ('d2', 'closest', 'bary'):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert_same_bits('dropped faces: default = brute', a, holed.closest(T(p), brute=True))
    # every face dropped: +inf and -1
    empty = eng.mesh(T(np.full_like(v, np.nan)), T(f))
    for brute in (False, True):
        o = empty.closest(T(p), brute=brute)
        assert bool(torch.isinf(o.d2).all()) and bool((o.d2 > 0).all()) and bool((o.face == -1).all())
        assert bool(torch.isnan(o.closest).all()) and bool(torch.isnan(o.bary).all())
    for m in (holed, cut, empty):
        m.close()


def test_argument_errors(eng):
    v, f = hull()
    tv = T(v)
    for bad, msg in ((np.array([[0, 1, len(v)]]), 'face index'), (np.array([[0, -1, 2]]), 'face index'), (np.zeros((0, 3), dtype=np.int64), 'bad sizes')):
        with pytest.raises(RaError, match=msg):
            eng.mesh(tv, T(bad))
    with pytest.raises(RaError, match='bad sizes|null argument'):            # no vertices: an empty tensor has no address either
        eng.mesh(torch.zeros(0, 3, device='cuda:0'), T(f[:1]))
    mesh = eng.mesh(tv, T(f))
    pts = T(point_sets('hull')['near'][:8])
    L = eng.lib
    null = [None] * 4
    assert L.ra_mesh_closest(eng.ctx, mesh._handle, C.c_void_p(pts.data_ptr()), 8, 0, *null, eng.stream) == 1 and b'null argument' in L.ra_last_error()
    d2 = torch.empty(8, device='cuda:0')
    out = [C.c_void_p(d2.data_ptr()), None, None, None]
    assert L.ra_mesh_closest(eng.ctx, mesh._handle, C.c_void_p(pts.data_ptr()), 8, 4, *out, eng.stream) == 1 and b'unknown flag' in L.ra_last_error()
    assert L.ra_mesh_closest(eng.ctx, mesh._handle, C.c_void_p(pts.data_ptr()), -1, 0, *out, eng.stream) == 1 and b'bad sizes' in L.ra_last_error()
    assert L.ra_mesh_closest(eng.ctx, mesh._handle, None, 8, 0, *out, eng.stream) == 1 and b'null argument' in L.ra_last_error()
    assert L.ra_mesh_closest(eng.ctx, mesh._handle, None, 0, 0, *out, eng.stream) == 0          # n == 0: nothing to read, nothing launched
    with pytest.raises(ValueError, match='want'):
        mesh.closest(pts, want=())
    mesh.close()
    with pytest.raises(RaError, match='closed'):
        mesh.closest(pts)
    assert L.ra_mesh_closest(eng.ctx, mesh._handle, C.c_void_p(pts.data_ptr()), 8, 0, *out, eng.stream) == 1      # a null mesh
    mesh.close()                                                                                                  # twice is harmless


def test_meshes_are_freed_with_their_handle_and_with_their_context(eng):
    """no allocation counter in the context: 100 meshes created and destroyed leave the device's free memory where it was, and so do 100
    meshes left to ra_ctx_destroy"""
    from relightableavatar_amd.engine import Engine
    v, f = hull()
    tv, tf = T(v), T(f)
    eng.mesh(tv, tf).close()                      # the context's build scratch exists from here on
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    held = [eng.mesh(tv, tf) for _ in range(100)]
    torch.cuda.synchronize()
    free_held = torch.cuda.mem_get_info()[0]
    for m in held:
        m.close()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print(f'free memory: {free0} before, {free_held} with 100 meshes alive, {free1} after ra_mesh_destroy')
    assert free1 >= free0
    other = Engine(make_cfg('relight'), device='cuda:0')
    other.mesh(tv, tf).close()
    torch.cuda.synchronize()
    free2 = torch.cuda.mem_get_info()[0]
    held = [other.mesh(tv, tf) for _ in range(100)]
    probe = held[0].closest(tv[:4])
    torch.cuda.synchronize()
    free_held = torch.cuda.mem_get_info()[0]
    del other
    gc.collect()
    torch.cuda.synchronize()
    free3 = torch.cuda.mem_get_info()[0]
    print(f'free memory: {free2} before, {free_held} with 100 meshes alive, {free3} after ra_ctx_destroy alone')
    assert free3 >= free2
    with pytest.raises(RaError, match='gone'):
        held[0].closest(tv[:4])
    for m in held:
        m.close()                                 # the context freed them: the handles only forget


# ------------------------------------------------------------------------------------------------ mesh_utils
def test_mesh_utils_distances(eng):
    v, f = hull()
    p = point_sets('hull')['near']
    r64, r32 = reference('hull', 'near')
    d = mesh_utils.bvh_distance(T(p), T(v), T(f), engine=eng)
    parity('bvh_distance', d.cpu().double(), np.sqrt(r32[0].astype(np.float64)), np.sqrt(r64[0]))
    d1 = mesh_utils.sample_closest_points_on_surface(T(p)[None], T(v)[None], T(f)[None], engine=eng)
    assert tuple(d1.shape) == (1, len(p), 1) and torch.equal(d1.view(-1), d)
    # values that are linear in space are reproduced at the closest point
    w = np.float64([[0.3, -1.0, 2.0, 0.5], [1.0, 0.25, -0.5, 0.0]])
    values = torch.from_numpy(v.astype(np.float64) @ w[:, :3].T + w[:, 3]).float()
    interp, d2 = mesh_utils.sample_closest_points_on_surface(T(p)[None], T(v)[None], T(f)[None], values.cuda()[None], engine=eng)
    q = eng.mesh(T(v), T(f)).closest(T(p), want=('closest',)).closest.cpu().double().numpy()
    err = np.abs(interp[0].cpu().double().numpy() - (q @ w[:, :3].T + w[:, 3])).max()
    print(f'sample_closest_points_on_surface: linear values at the closest point to {err:.2e}')
    assert tuple(interp.shape) == (1, len(p), 2) and torch.equal(d2.view(-1), d) and err <= 16 * U * np.abs(values.numpy()).max()
    with pytest.raises(NotImplementedError, match='B > 1'):
        mesh_utils.sample_closest_points_on_surface(T(p)[None].repeat(2, 1, 1), T(v)[None].repeat(2, 1, 1), T(f)[None].repeat(2, 1, 1), engine=eng)


# ------------------------------------------------------------------------------------------------ the evaluator
def displaced_hull(mm=3.0):
    v, f = hull()
    v64 = v.astype(np.float64)
    fn = np.cross(v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]])
    vn = np.zeros_like(v64)
    for k in range(3):
        np.add.at(vn, f[:, k], fn)
    vn /= np.linalg.norm(vn, axis=-1, keepdims=True)
    return (v64 + mm * 1e-3 * vn).astype(np.float32), f


def _ref_metrics(src, tgt, src_pts, tgt_pts, p2s_pts, dtype):
    mean = lambda pts, m: np.sqrt(M.closest_point(pts, m[0], m[1], dtype)[0].astype(np.float64)).mean()
    return np.array([(mean(src_pts, tgt) + mean(tgt_pts, src)) / 2, mean(p2s_pts, tgt)])


def test_evaluator_arithmetic_on_given_samples(eng):
    src, tgt = hull(), displaced_hull()
    g = torch.Generator().manual_seed(0)
    draw = lambda m, n: mesh_utils.sample_surface(torch.from_numpy(m[0]), torch.from_numpy(m[1]), n, g)[0].numpy()
    src_pts, tgt_pts, p2s_pts = draw(src, 300), draw(tgt, 300), draw(src, 700)
    ms, mt = eng.mesh(T(src[0]), T(src[1])), eng.mesh(T(tgt[0]), T(tgt[1]))
    got = mesh_evaluator.chamfer_and_p2s(ms, mt, T(src_pts), T(tgt_pts), T(p2s_pts))
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (2,)
    r64, r32 = _ref_metrics(src, tgt, src_pts, tgt_pts, p2s_pts, np.float64), _ref_metrics(src, tgt, src_pts, tgt_pts, p2s_pts, np.float32)
    print(f'chamfer, p2s: device {got.tolist()}, float64 {r64.tolist()}, float32 {r32.tolist()}')
    parity('chamfer, p2s (3 mm apart)', got, r32, r64)
    row = torch.zeros(2, dtype=torch.float64, device='cuda:0')
    assert mesh_evaluator.chamfer_and_p2s(ms, mt, T(src_pts), T(tgt_pts), T(p2s_pts), out=row) is row and torch.equal(row, got)
    ms.close(), mt.close()


def test_evaluator_identical_meshes_score_the_samples_own_rounding(eng):
    """identical meshes: the distances are those of the float32 samples from the surface they were drawn on — no absolute threshold,
    the float64 reference on the same samples"""
    src = hull()
    dev_gen = lambda: torch.Generator(device='cuda:0').manual_seed(7)
    ev = mesh_evaluator.MeshEvaluator(eng, dev_gen())
    ev.set_src_mesh({'verts': T(src[0])[None], 'faces': T(src[1])[None]})
    ev.set_tgt_mesh((src[0], src[1]))
    got = torch.stack([ev.get_chamfer_dist(200), ev.get_surface_dist(500)])
    ev.close()
    g = dev_gen()
    draw = lambda n: mesh_utils.sample_surface(T(src[0]), T(src[1]), n, g)[0].cpu().numpy()
    src_pts, tgt_pts, p2s_pts = draw(200), draw(200), draw(500)
    r64, r32 = _ref_metrics(src, src, src_pts, tgt_pts, p2s_pts, np.float64), _ref_metrics(src, src, src_pts, tgt_pts, p2s_pts, np.float32)
    print(f'identical meshes: device {got.tolist()}, float64 {r64.tolist()}, float32 {r32.tolist()}')
    parity('chamfer, p2s (identical meshes)', got, r32, r64)


def test_evaluator_end_to_end(eng, tmp_path):
    src, tgt = hull(), displaced_hull()
    obj = tmp_path / 'scan.obj'
    obj.write_text(''.join(f'v {x!r} {y!r} {z!r}\n' for x, y, z in tgt[0].tolist()) + ''.join(f'f {a + 1} {b + 1} {c + 1}\n' for a, b, c in tgt[1].tolist()))

    class Tri:
        vertices, faces = src
    ev = make_evaluator(make_cfg('relight', evaluator_module='relightableavatar_amd.evaluators.mesh_evaluator'))
    assert type(ev) is mesh_evaluator.Evaluator
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ev.evaluate({'mesh': Tri()}, {'obj': [str(obj)]})
    runs = []
    for _ in range(2):
        g = torch.Generator(device='cuda:0').manual_seed(1)
        ev.evaluate({'mesh': Tri()}, {'obj': [str(obj)]}, engine=eng, generator=g)                                   # a trimesh-like object, a path
        ev.evaluate({'mesh': {'verts': T(src[0])[None], 'faces': T(src[1])[None]}}, {'obj': [tgt]}, engine=eng, generator=g)      # the renderer's keys, a pair
        assert len(ev) == 2
        s = ev.summarize()
        assert len(ev) == 0 and set(s) == {'chamfer', 'p2s'} and set(ev.metrics) == {'chamfer', 'p2s'}
        assert all(len(ev.metrics[k]) == 2 and s[k] == float(np.mean(ev.metrics[k])) for k in s)
        runs.append((s, ev.metrics))
    print(f'two frames, twice: {runs[0][0]}; per frame {runs[0][1]}')
    assert runs[0] == runs[1]                                                     # equal generators: bit-equal
    with pytest.raises(RuntimeError, match='no frame'):
        ev.summarize()

"""ra_mesh_raycast, ra_ray_tri_pairs, Mesh.raycast and the ray helpers of mesh_utils on the device.
Run with `-m gpu` on an MI355X.

No tolerance is chosen here.  u, v, t are held to the project's 10 x float32 rule (frame_stage_ref.parity) against float64, the float32
reference being the restatement of the kernel's operations (tests/raycast_ref.py) or, for the dense pairs, the reference's own float32
result stored in the golden, whose error is also the ceiling: on the median of all pairs and on the maximum over the pairs near their
face (raycast_ref.check_pairs).  face and count are compared exactly
with the float64 exhaustive result on the DECIDED rays (raycast_ref's classification condition).  Exactness is bit equality: a ray's
four outputs do not depend on the sweep (default = RA_RAYCAST_BRUTE), the internal order (= RA_RAYCAST_UNSORTED), the pruning by t
(a call without count prunes, a call with count does not), the call (twice), the order of the rays (permuted and back) or n
(prefixes).  On the mesh 'degenerate' and the ray set 'graze' only bit equality, determinism and finiteness are asserted.  Every test
prints its figures before it asserts."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import raycast_ref as R
import winding_ref as W
from frame_stage_ref import parity
from relightableavatar_amd import _lib, mesh_utils
from relightableavatar_amd._lib import RaError
from relightableavatar_amd.config import make_cfg

pytestmark = pytest.mark.gpu
KEYS = ('t', 'face', 'uv', 'count')
NEAR = ('t', 'face', 'uv')


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from relightableavatar_amd.engine import Engine
    return Engine(make_cfg('relight'), device='cuda:0')          # any context will do: no weights are read


@functools.lru_cache(None)
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'raycast.npz'))


def T(a, dev='cuda:0'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same_bits(tag, a, b, keys=KEYS, rows=None):
    """a[k][rows[0]] and b[k][rows[1]] hold the same bits for every key"""
    ra, rb = rows if rows is not None else (slice(None), slice(None))
    for k in keys:
        x, y = a[k].cpu()[ra].view(torch.int32), b[k].cpu()[rb].view(torch.int32)
        same = bool(torch.equal(x, y))
        print(f'{tag}: {k} bit-equal {same} ({x.shape[0]} rays)')
        assert same, (tag, k)


def all_ways(tag, mesh, o, d):
    """the default call, and everything that must return its bits; returns the default call's outputs"""
    to, td = T(o), T(d)
    out = mesh.raycast(to, td)
    near = mesh.raycast(to, td, want=NEAR)                        # pruned by t
    assert set(out) == set(KEYS) and set(near) == set(NEAR)
    same_bits(f'{tag} with count = without (pruned by t)', out, near, NEAR)
    same_bits(f'{tag} default = brute', out, mesh.raycast(to, td, brute=True))
    same_bits(f'{tag} pruned = brute', near, mesh.raycast(to, td, want=NEAR, brute=True), NEAR)
    same_bits(f'{tag} default = unsorted', out, mesh.raycast(to, td, sort=False))
    same_bits(f'{tag} pruned = unsorted', near, mesh.raycast(to, td, want=NEAR, sort=False), NEAR)
    same_bits(f'{tag} twice', out, mesh.raycast(to, td))
    if len(o) > 1:
        perm = torch.from_numpy(np.random.default_rng(3).permutation(len(o)))
        same_bits(f'{tag} permuted rays', mesh.raycast(to[perm.cuda()], td[perm.cuda()]), out, rows=(slice(None), perm))
        same_bits(f'{tag} permuted rays, pruned', mesh.raycast(to[perm.cuda()], td[perm.cuda()], want=NEAR), out, NEAR, rows=(slice(None), perm))
    part = mesh.raycast(to, td, want=('count',))
    assert set(part) == {'count'} and torch.equal(part.count, out.count)
    return out


def check_documented_shape(tag, out):
    """what every finite ray's answer looks like"""
    t, face, uv, count = (out[k].cpu().numpy() for k in KEYS)
    hit = face >= 0
    assert not np.isnan(t).any() and np.isfinite(t[hit]).all() and (t[hit] >= 0).all() and np.isposinf(t[~hit]).all(), tag
    assert np.isfinite(uv[hit]).all() and np.isnan(uv[~hit]).all() and (uv[hit] >= 0).all() and (uv[hit].sum(-1) <= 1).all(), tag
    assert (count >= 0).all() and ((count > 0) == hit).all(), tag


def check_against_truth(tag, out, e):
    """face and count exactly on the decided rays; t and uv under the 10 x rule on the decided rays that hit"""
    t, face, uv, count = (out[k].cpu().numpy() for k in KEYS)
    dec = e['decided']
    t64, f64, uv64, c64 = e['truth']
    tk, fk, uvk, ck = e['restated']
    print(f'{tag}: {int(dec.sum())} of {len(dec)} rays decided (margin {e["margin"]:.3e}); face differs on {int((face != f64)[dec].sum())}, count on {int((count != c64)[dec].sum())}; '
          f'bit-equal to the restatement: t {np.array_equal(t, tk)}, face {np.array_equal(face, fk)}, count {np.array_equal(count, ck)}')
    assert np.array_equal(face[dec], f64[dec]) and np.array_equal(count[dec], c64[dec]), tag
    keep = dec & (f64 >= 0)
    parity(f'{tag} t', t, tk, t64, keep=keep, relative=True)
    parity(f'{tag} uv', uv, uvk, uv64, keep=keep)


# ------------------------------------------------------------------------------------------------ the dense pairs
@pytest.mark.parametrize('name', R.GOLDEN_MESHES)
def test_pairs_against_the_golden(eng, name):
    o, d, tris = R.golden_pairs(name)
    got = eng.ray_tri_pairs(T(o), T(d), T(tris))
    k32 = R.kernel32(o, d, tris)
    for i, k in enumerate('uvt'):
        x = got[i].cpu().numpy()
        assert x.shape == (len(o), len(tris)) and x.dtype == np.float32
        print(f'{name}/{k}: bit-equal to the restatement on {(x == k32[i]).mean():.4f} of the pairs')
        R.check_pairs(f'{name}/{k} ra_ray_tri_pairs', x, golden()[f'{name}/{k}32'], golden()[f'{name}/{k}64'],
                      R.near_pairs(golden()[f'{name}/u64'], golden()[f'{name}/v64']))
    again = eng.ray_tri_pairs(T(o), T(d), T(tris))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, again))


def test_pairs_edge_sizes_and_errors(eng):
    o, d, tris = R.golden_pairs('hull')
    pb = eng.lib.ra_raycast_tile(1)
    full = [x.cpu() for x in eng.ray_tri_pairs(T(o), T(d), T(tris))]
    for n, f in ((1, 1), (1, pb - 1), (1, pb), (3, pb // 3 + 1), (7, 37), (84, 60)):
        tr = np.concatenate([tris] * ((f + len(tris) - 1) // len(tris)))[:f]
        got = eng.ray_tri_pairs(T(o[:n]), T(d[:n]), T(tr))
        cols = np.arange(f) % len(tris)
        for a, b in zip(got, full):
            assert a.shape == (n, f) and torch.equal(a.cpu().view(torch.int32), b[:n][:, cols].view(torch.int32)), (n, f)
    u, v, t = eng.ray_tri_pairs(T(o[:0]), T(d[:0]), T(tris))
    assert u.shape == (0, len(tris))
    u, v, t = mesh_utils.moller_trumbore(T(o)[None], T(d)[None], T(tris)[None], engine=eng)
    assert u.shape == v.shape == t.shape == (1, len(o), len(tris)) and torch.equal(t[0].cpu(), full[2])
    u, v, t = mesh_utils.moller_trumbore(T(o), T(d), T(tris), engine=eng)
    assert u.shape == (len(o), len(tris)) and torch.equal(u.cpu(), full[0]) and torch.equal(v.cpu(), full[1])
    lib, p = eng.lib, C.c_void_p(T(o).data_ptr())
    assert lib.ra_ray_tri_pairs(eng.ctx, p, p, 1 << 16, p, 1 << 15, p, p, p, eng.stream) != 0 and b'bad sizes' in lib.ra_last_error()
    assert lib.ra_ray_tri_pairs(eng.ctx, p, p, -1, p, 1, p, p, p, eng.stream) != 0 and b'bad sizes' in lib.ra_last_error()
    assert lib.ra_ray_tri_pairs(eng.ctx, p, p, 1, p, 1, None, None, None, eng.stream) != 0 and b'null argument' in lib.ra_last_error()
    assert lib.ra_ray_tri_pairs(eng.ctx, None, None, 0, None, 5, None, None, None, eng.stream) == 0


# ------------------------------------------------------------------------------------------------ meshes x ray sets
@pytest.mark.parametrize('group', R.SETS + (R.GRAZE,))
@pytest.mark.parametrize('name', R.MESHES)
def test_meshes_and_ray_sets(eng, name, group):
    v, f = R.mesh_case(name)
    o, d = R.ray_sets(name)[group]
    mesh = eng.mesh(T(v), T(f))
    tag = f'{name}/{group} ({len(f)} faces, {len(o)} rays)'
    out = all_ways(tag, mesh, o, d)
    check_documented_shape(tag, out)
    check_against_truth(tag, out, R.evaluate(name, group))
    mesh.close()


def test_prefixes_of_the_257_ray_call(eng):
    v, f = R.mesh_case('hull')
    o, d = R.ray_sets('hull')['outside']
    assert len(o) == 257
    mesh = eng.mesh(T(v), T(f))
    full = mesh.raycast(T(o), T(d))
    full_near = mesh.raycast(T(o), T(d), want=NEAR)
    wave, unsorted_up_to = eng.lib.ra_raycast_tile(0), eng.lib.ra_raycast_tile(2)
    assert (wave, unsorted_up_to) == (64, 64)
    for n in (0, 1, wave - 1, wave, wave + 1, 257):
        part = mesh.raycast(T(o[:n]), T(d[:n]))
        assert all(part[k].shape[0] == n for k in KEYS)
        same_bits(f'n = {n}: prefix of the 257-ray call', part, full, rows=(slice(None), slice(0, n)))
        same_bits(f'n = {n}: prefix, pruned by t', mesh.raycast(T(o[:n]), T(d[:n]), want=NEAR), full_near, NEAR, rows=(slice(None), slice(0, n)))
    mesh.close()


def test_edge_face_counts(eng):
    v, f = R.mesh_case('hull')
    o, d = R.ray_sets('hull')['outside']
    t0, t1 = eng.lib.ra_mesh_tile(0), eng.lib.ra_mesh_tile(1)
    sizes = (1, t0 - 1, t0, t0 + 1, t0 * t1 - 1, t0 * t1, t0 * t1 + 1)
    assert sizes == (1, 31, 32, 33, 255, 256, 257)
    order = np.random.default_rng(5).permutation(len(f))          # faces from all over the hull, so that most rays meet some
    for n_faces in sizes:
        sub = f[order[:n_faces]]
        mesh = eng.mesh(T(v), T(sub))
        tag = f'{n_faces} faces'
        out = all_ways(tag, mesh, o, d)
        check_documented_shape(tag, out)
        check_against_truth(tag, out, R.evaluate_mesh(o, d, v, sub))
        mesh.close()


# ------------------------------------------------------------------------------------------------ further properties
def test_two_copies_answer_like_one_where_only_one_is_reached(eng):
    v, f = R.mesh_case('hull')
    v2, f2 = R.mesh_case('two')
    o = np.concatenate([R.ray_sets('hull')[g][0] for g in ('outside', 'inside', R.GRAZE)])
    d = np.concatenate([R.ray_sets('hull')[g][1] for g in ('outside', 'inside', R.GRAZE)])
    # a ray reaches copy B only through B's box, widened by 0.1: everything else is decided by copy A alone
    lo, hi = v2[len(v):].min(0) - 0.1, v2[len(v):].max(0) + 0.1
    with np.errstate(all='ignore'):
        t1, t2 = (lo - o) / d, (hi - o) / d
        near, far = np.fmin(t1, t2).max(-1), np.fmax(t1, t2).min(-1)
    only_a = ~((near <= far) & (far >= 0)) & (d != 0).all(-1)
    assert 200 < only_a.sum() < len(o)
    one, two = eng.mesh(T(v), T(f)), eng.mesh(T(v2), T(f2))
    a, b = one.raycast(T(o), T(d)), two.raycast(T(o), T(d))
    rows = torch.from_numpy(np.nonzero(only_a)[0])
    same_bits(f'{int(only_a.sum())} rays that only reach copy A: two copies = one', a, b, rows=(rows, rows))
    assert int(b.face.max()) < 2 * len(f)
    one.close(), two.close()


def test_every_face_twice_answers_the_lower_copy(eng):
    v, f = R.mesh_case('hull')
    o, d = R.ray_sets('hull')['outside']
    one, twice = eng.mesh(T(v), T(f)), eng.mesh(T(v), T(np.concatenate([f, f])))
    a, b = one.raycast(T(o), T(d)), all_ways('every face twice', twice, o, d)
    same_bits('every face twice: t, face, uv of the single mesh', a, b, NEAR)
    assert torch.equal(b.count, 2 * a.count) and int(b.face.max()) < len(f)
    one.close(), twice.close()


@pytest.mark.parametrize('n', [64, 130])
def test_non_finite_rays(eng, n):
    v, f = R.mesh_case('hull')
    o, d = (x[:n].copy() for x in R.ray_sets('hull')['outside'])
    mesh = eng.mesh(T(v), T(f))
    clean = mesh.raycast(T(o), T(d))
    bad = {3: ('o', 0, np.nan), 17: ('d', 2, np.nan), 40: ('o', 1, np.inf), 63: ('d', 0, -np.inf)}
    if n > 64:
        bad.update({64: ('d', 1, np.inf), 100: ('o', 2, -np.inf), n - 1: ('o', 0, np.nan)})
    for i, (which, k, val) in bad.items():
        (o if which == 'o' else d)[i, k] = val
    rows = np.array(sorted(bad))
    others = torch.from_numpy(np.setdiff1d(np.arange(n), rows))
    for kw in (dict(), dict(brute=True), dict(sort=False), dict(want=NEAR)):
        out = mesh.raycast(T(o), T(d), **kw)
        keys = kw.get('want', KEYS)
        same_bits(f'n = {n} {kw}: the other rays', out, clean, keys, rows=(others, others))
        assert torch.isnan(out.t.cpu()[rows]).all() and torch.isnan(out.uv.cpu()[rows]).all() and (out.face.cpu()[rows] == -1).all(), kw
        if 'count' in keys:
            assert (out.count.cpu()[rows] == -1).all(), kw
    mesh.close()


def test_dropped_faces_are_never_answered(eng):
    v, f = R.mesh_case('hull')
    o, d = R.ray_sets('hull')['outside']
    bad = v.copy()
    vert = int(f[3, 0])
    bad[vert] = [np.nan, 0, np.inf]
    gone = (f == vert).any(1)
    assert 2 < gone.sum() < 20
    mesh, rest = eng.mesh(T(bad), T(f)), eng.mesh(T(v), T(f[~gone]))
    out, ref = all_ways('faces at a non-finite vertex', mesh, o, d), rest.raycast(T(o), T(d))
    same_bits('faces at a non-finite vertex: the mesh without them', out, ref, ('t', 'uv', 'count'))
    kept = np.nonzero(~gone)[0]
    assert np.array_equal(out.face.cpu().numpy(), np.where(ref.face.cpu().numpy() >= 0, kept[np.maximum(ref.face.cpu().numpy(), 0)], -1))
    assert not np.isin(out.face.cpu().numpy(), np.nonzero(gone)[0]).any()
    check_against_truth('faces at a non-finite vertex', out, R.evaluate_mesh(o, d, bad, f))
    mesh.close(), rest.close()
    nothing = eng.mesh(T(np.full_like(v, np.nan)), T(f))
    for kw in (dict(), dict(brute=True), dict(sort=False)):
        out = nothing.raycast(T(o), T(d), **kw)
        assert torch.isposinf(out.t).all() and (out.face == -1).all() and (out.count == 0).all() and torch.isnan(out.uv).all(), kw
    nothing.close()


def test_errors_come_back_as_such(eng):
    v, f = R.mesh_case('single')
    o, d = (T(x[:8]) for x in R.ray_sets('single')['outside'])
    mesh = eng.mesh(T(v), T(f))
    lib, P = eng.lib, lambda t: C.c_void_p(t.data_ptr())
    t = torch.empty(8, device='cuda:0')

    def call(ctx, handle, po, pd, n, flags, pt):
        return lib.ra_mesh_raycast(ctx, handle, po, pd, n, flags, pt, None, None, None, eng.stream)
    assert call(eng.ctx, mesh._handle, P(o), P(d), 8, 0, P(t)) == 0
    for args, text in (((None, mesh._handle, P(o), P(d), 8, 0, P(t)), b'null argument'), ((eng.ctx, None, P(o), P(d), 8, 0, P(t)), b'null argument'),
                       ((eng.ctx, mesh._handle, None, P(d), 8, 0, P(t)), b'null argument'), ((eng.ctx, mesh._handle, P(o), None, 8, 0, P(t)), b'null argument'),
                       ((eng.ctx, mesh._handle, P(o), P(d), 8, 0, None), b'null argument'), ((eng.ctx, mesh._handle, P(o), P(d), -1, 0, P(t)), b'bad sizes'),
                       ((eng.ctx, mesh._handle, P(o), P(d), 1 << 30, 0, P(t)), b'bad sizes'), ((eng.ctx, mesh._handle, P(o), P(d), 8, 4, P(t)), b'unknown flag'),
                       ((eng.ctx, C.c_void_p(P(o).value), P(o), P(d), 8, 0, P(t)), b'not a mesh of this ctx')):
        assert call(*args) != 0 and text in lib.ra_last_error(), (text, lib.ra_last_error())
    assert call(eng.ctx, mesh._handle, None, None, 0, 0, None) == 0          # n == 0 reads no pointer
    with pytest.raises(ValueError):
        mesh.raycast(o, d, want=())
    with pytest.raises(ValueError):
        mesh.raycast(o, d, want=('t', 'd2'))
    with pytest.raises(ValueError):
        mesh.raycast(o, d[:4])
    mesh.close()
    with pytest.raises(RaError):
        mesh.raycast(o, d)


def test_closest_and_winding_keep_their_bits(eng):
    v, f = R.mesh_case('hull')
    p = T(W.point_sets('hull')['near'])
    mesh = eng.mesh(T(v), T(f))
    c0, w0 = mesh.closest(p), mesh.winding(p)
    for group in ('outside', R.GRAZE):
        o, d = R.ray_sets('hull')[group]
        mesh.raycast(T(o), T(d))
        mesh.raycast(T(o), T(d), want=NEAR, brute=True)
    c1, w1 = mesh.closest(p), mesh.winding(p)
    for k in ('d2', 'closest', 'face', 'bary'):
        assert torch.equal(c0[k].view(torch.int32), c1[k].view(torch.int32)), k
    assert torch.equal(w0.view(torch.int32), w1.view(torch.int32))
    mesh.close()


# ------------------------------------------------------------------------------------------------ mesh_utils
def test_ray_stabbing(eng):
    v, f = R.mesh_case('hull')
    o = np.concatenate([R.ray_sets('hull')[g][0] for g in ('inside', 'miss', 'outside')])
    d = np.concatenate([R.ray_sets('hull')[g][1] for g in ('inside', 'miss', 'outside')])
    e = R.evaluate_mesh(o, d, v, f)
    occ = mesh_utils.ray_stabbing(T(o), T(v), T(f), ray_d=T(d), engine=eng)
    assert occ.shape == (len(o), 1) and occ.dtype == torch.float32
    dec = e['decided']
    want = (e['truth'][3] % 2).astype(np.float32)
    print(f'ray_stabbing, given directions: {int(dec.sum())} of {len(dec)} points decided; parity differs on {int((occ.cpu().numpy()[:, 0] != want)[dec].sum())}')
    assert np.array_equal(occ.cpu().numpy()[dec, 0], want[dec]) and want[dec].sum() > 100 and (1 - want[dec]).sum() > 100      # both answers occur
    # multiplier: the directions of the expanded points; three times the same directions give the same share
    occ3 = mesh_utils.ray_stabbing(T(o), T(v), T(f), multiplier=3, ray_d=T(np.concatenate([d, d, d])), engine=eng)
    assert torch.equal(occ3, occ)
    with pytest.raises(ValueError):
        mesh_utils.ray_stabbing(T(o), T(v), T(f), multiplier=2, ray_d=T(d), engine=eng)
    # drawn directions against the winding number, at grid points at least 1 cm from the surface
    p = T(W.point_sets('hull')['grid'][::23])
    mesh = eng.mesh(T(v), T(f))
    keep = mesh.closest(p, want=('d2',)).d2.sqrt() >= 0.01
    inside = mesh.winding(p) > 0.5
    mesh.close()
    g = torch.Generator(device='cuda:0').manual_seed(11)
    a = mesh_utils.ray_stabbing(p, T(v), T(f), multiplier=3, generator=g, engine=eng)
    b = mesh_utils.ray_stabbing(p, T(v), T(f), multiplier=3, generator=torch.Generator(device='cuda:0').manual_seed(11), engine=eng)
    assert torch.equal(a, b) and a.shape == (len(p), 1)
    agree = ((a[:, 0] > 0.5) == inside)[keep]
    print(f'ray_stabbing, drawn directions x 3: {int(keep.sum())} of {len(p)} grid points at least 1 cm off the surface, {int(inside[keep].sum())} inside; '
          f'the majority disagrees with winding > 0.5 on {int((~agree).sum())}; shares {sorted(set(a[:, 0].cpu().tolist()))}')
    assert int(keep.sum()) > 300 and int(inside[keep].sum()) > 30 and bool(agree.all())


def test_raycast_maps_on_a_ray_grid(eng):
    v, f = R.mesh_case('hull')
    cen, ext = v.astype(np.float64).mean(0), np.abs(v - v.mean(0)).max(0).astype(np.float64)
    gx, gz = np.meshgrid(np.linspace(-1.3, 1.3, 16), np.linspace(-1.3, 1.3, 16), indexing='ij')
    target = cen + np.stack([gx * ext[0], np.zeros_like(gx), gz * ext[2]], -1)
    o = np.broadcast_to(cen + [0.3, -3.0, 0.2], target.shape)
    d = target - o                                                    # a pinhole 3 m in front; d not normalised
    o32, d32 = o.astype(np.float32), d.astype(np.float32)
    e = R.evaluate_mesh(o32.reshape(-1, 3), d32.reshape(-1, 3), v, f)
    maps = mesh_utils.raycast_maps(T(o32), T(d32), T(v), T(f), engine=eng)
    assert maps.acc_map.shape == (16, 16, 1) and maps.depth_map.shape == (16, 16, 1) and maps.norm_map.shape == (16, 16, 3) and maps.face.shape == (16, 16)
    dec = e['decided']
    t64, f64, _, _ = e['truth']
    tk = e['restated'][0]
    acc = maps.acc_map.cpu().numpy().reshape(-1)
    print(f'raycast_maps: {int(dec.sum())} of 256 rays decided, {int((f64 >= 0).sum())} hit; mask differs on {int((acc != (f64 >= 0))[dec].sum())}')
    assert 60 < (f64 >= 0).sum() < 200 and dec.mean() > 0.9
    assert np.array_equal(acc[dec], (f64 >= 0)[dec].astype(np.float32)) and np.array_equal(maps.face.cpu().numpy().reshape(-1)[dec], f64[dec])
    keep = dec & (f64 >= 0)
    parity('raycast_maps depth', maps.depth_map.cpu().numpy().reshape(-1), np.where(np.isfinite(tk), tk, 0), np.where(np.isfinite(t64), t64, 0), keep=keep, relative=True)
    assert (maps.depth_map.cpu().numpy().reshape(-1)[acc == 0] == 0).all() and (maps.norm_map.cpu().numpy().reshape(-1, 3)[acc == 0] == 0).all()
    tri = v.astype(np.float64)[f[np.maximum(f64, 0)]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    got = maps.norm_map.cpu().numpy().reshape(-1, 3)
    assert np.abs(got[keep] - nrm[keep]).max() < 1e-5 and np.abs(np.linalg.norm(got[keep], axis=-1) - 1).max() < 1e-6

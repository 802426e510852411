"""ra_mesh_winding, Mesh.winding and the winding-distance remesh of mesh_utils on the device.
Run with `-m gpu` on an MI355X.

No tolerance is chosen here.  The winding number is held to the project's 10 x float32 rule (frame_stage_ref.parity): max and median
|diff| against the float64 reference (the reference's own formula, tests/winding_ref.py; on the golden's inputs the stored float64
result of the reference itself, which test_oracle_winding.py shows to be the same numbers) are at most 10 x the error of the float32
restatement of the kernel's operations on the same inputs, and the max is also no larger than the reference's own float32 error (the
golden's float32 result against its float64 one).  Exactness is bit equality: a point's result does not depend on n, on the order or
the subset of the points, or on the launch shape.  Every test prints its figures before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mesh_distance_ref as M
import mesh_extract_ref as X
import winding_ref as W
from frame_stage_ref import parity
from relightableavatar_amd import mesh_utils
from relightableavatar_amd._lib import RaError
from relightableavatar_amd.config import make_cfg

pytestmark = pytest.mark.gpu
REMESH = dict(voxel_size=0.04, dist_th_verts=0.2, dist_th_tris=0.08)


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from relightableavatar_amd.engine import Engine
    return Engine(make_cfg('relight'), device='cuda:0')          # any context will do: no weights are read


@functools.lru_cache(None)
def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'winding.npz'))


@functools.lru_cache(None)
def restated(name, group):
    v, f = W.mesh_case(name)
    return W.winding_number_kernel32(W.point_sets(name)[group], v, f)


@functools.lru_cache(None)
def large():
    """the hull at 10 001 vertices (19 998 faces), 256 points 1 cm inside and outside it, and their references"""
    v, f = W.hull(10001)
    tri = v.astype(np.float64)[f[::157][:128]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    p = np.concatenate([tri.mean(1) + 1e-2 * nrm, tri.mean(1) - 1e-2 * nrm]).astype(np.float32)
    assert len(p) == 256
    return v, f, p


@functools.lru_cache(None)
def large_refs(n_faces):
    v, f, p = large()
    f = f[:n_faces]
    return W.winding_number(p, v, f), W.winding_number_kernel32(p, v, f), W.winding_number(p, v, f, np.float32)


def T(a, dev='cuda:0'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same_bits(tag, a, b):
    same = bool(torch.equal(a.view(torch.int32).cpu(), b.view(torch.int32).cpu()))
    print(f'{tag}: bit-equal {same} ({a.numel()} points)')
    assert same, tag


def check_parity(tag, w, r32, r64, own32):
    """the 10 x rule, and the ceiling: the reference's own float32 error"""
    w = w.cpu().numpy()
    parity(tag, w, r32, r64)
    e, own = np.abs(w.astype(np.float64) - r64).max(), np.abs(own32.astype(np.float64) - r64).max()
    print(f'{tag}: max |kernel - float64| {e:.3e}, the reference in float32 {own:.3e}')
    assert e <= own, tag
    return e


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('group', W.SETS)
@pytest.mark.parametrize('name', W.MESHES)
def test_parity(eng, name, group):
    v, f = W.mesh_case(name)
    p = W.point_sets(name)[group]
    g = golden()
    mesh = eng.mesh(T(v), T(f))
    w = mesh.winding(T(p))
    check_parity(f'{name}/{group} ({len(f)} faces, {len(p)} points)', w, restated(name, group), g[f'{name}/{group}/w64'], g[f'{name}/{group}/w32'])
    same_bits(f'{name}/{group} twice', w, mesh.winding(T(p)))
    mesh.close()


def test_large_face_count(eng):
    """19 998 faces, 20 chunks: where a plain fp32 running sum would show"""
    v, f, p = large()
    r64, r32, own = large_refs(len(f))
    mesh = eng.mesh(T(v), T(f))
    w = mesh.winding(T(p))
    check_parity(f'large hull ({len(f)} faces, {len(p)} points)', w, r32, r64, own)
    assert np.abs(np.rint(r64) - np.r_[np.zeros(128), np.ones(128)]).max() == 0          # outside first, then inside
    mesh.close()


# ------------------------------------------------------------------------------------------------ exactness
def test_any_order_any_subset_any_n(eng):
    v, f = W.mesh_case('opened')
    p = T(W.point_sets('opened')['near'])
    tile = eng.lib.ra_winding_tile(0)
    assert tile == 64 and len(p) > 2 * tile
    mesh = eng.mesh(T(v), T(f))
    base = mesh.winding(p)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(p))).cuda()
    same_bits('permuted points', mesh.winding(p[perm]), base[perm])
    pick = torch.from_numpy(np.sort(np.random.default_rng(4).choice(len(p), 97, replace=False))).cuda()
    same_bits('a subset of 97', mesh.winding(p[pick]), base[pick])
    for n in (1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1):
        same_bits(f'the first {n}', mesh.winding(p[:n]), base[:n])
        same_bits(f'the last {n}', mesh.winding(p[-n:]), base[-n:])
    mesh.close()


def test_face_counts_at_tile_and_chunk_edges_and_both_launch_shapes(eng):
    """prefixes of the large hull's faces one short of, at and one past the leaf, the point tile and the chunk, and two chunks + 1:
    the default launch, the one-pass kernel and the split launch agree bit for bit, and all hold the 10 x rule"""
    v, f, p = large()
    leaf, tile, chunk = eng.lib.ra_mesh_tile(0), eng.lib.ra_winding_tile(0), eng.lib.ra_winding_tile(1)
    split_tiles = eng.lib.ra_winding_tile(2)
    assert (leaf, tile, chunk) == (32, 64, W.CHUNK) and split_tiles > len(p) // tile
    counts = sorted({t + d for t in (leaf, tile, chunk) for d in (-1, 0, 1)} | {2 * chunk + 1})
    assert counts[-1] < len(f)
    for n_faces in counts:
        r64, r32, _ = large_refs(n_faces)
        mesh = eng.mesh(T(v), T(f[:n_faces]))
        w = mesh.winding(T(p))
        parity(f'{n_faces} faces', w, r32, r64)          # no ceiling here: with a few faces both float32 errors are the rounding of the result itself
        one, split = mesh.winding(T(p), shape='one_pass'), mesh.winding(T(p), shape='split')
        same_bits(f'{n_faces} faces: default = one pass', w, one)
        same_bits(f'{n_faces} faces: split = one pass', split, one)
        same_bits(f'{n_faces} faces: one point, split', mesh.winding(T(p[5:6]), shape='split'), one[5:6])
        mesh.close()


def test_split_launch_against_the_one_pass_kernel_on_the_large_hull(eng):
    """256 points against 20 chunks take the split launch by default; 64 x 2048 points and more the one-pass kernel"""
    v, f, p = large()
    mesh = eng.mesh(T(v), T(f))
    one = mesh.winding(T(p), shape='one_pass')
    same_bits('default (split) = one pass', mesh.winding(T(p)), one)
    same_bits('forced split = one pass', mesh.winding(T(p), shape='split'), one)
    many = T(p).repeat(eng.lib.ra_winding_tile(2) * eng.lib.ra_winding_tile(0) // len(p) + 1, 1)       # past the split threshold: one pass by default
    same_bits(f'{len(many)} points, default (one pass) = the 256 alone, repeated', mesh.winding(many), one.repeat(len(many) // len(p)))
    mesh.close()


# ------------------------------------------------------------------------------------------------ NaN rules, n == 0, errors
@pytest.mark.parametrize('shape', [None, 'one_pass', 'split'])
def test_nan_rules(eng, shape):
    v, f, _ = large()
    base = W.point_sets('hull')['near'][:130].copy()
    p = base.copy()
    bad = {3: [np.nan, 0, 0], 64: [0, np.inf, 0], 65: [0, 0, -np.inf], 70: v[f[1234, 1]], 129: v[f[7, 0]]}
    for i, x in bad.items():
        p[i] = x
    mesh = eng.mesh(T(v), T(f))
    w, alone = mesh.winding(T(p), shape=shape), mesh.winding(T(base), shape=shape)
    rows = np.array(sorted(bad))
    others = torch.from_numpy(np.setdiff1d(np.arange(len(p)), rows)).cuda()
    print(f'shape {shape}: rows {rows} -> {w[rows].cpu().numpy()}')
    assert bool(torch.isnan(w[rows]).all()) and bool(torch.isfinite(w[others]).all())
    same_bits('every other point as alone', w[others], alone[others])
    mesh.close()


def test_dropped_faces_contribute_nothing(eng):
    v, f = W.hull()
    p = T(W.point_sets('hull')['near'])
    bad = v.copy()
    bad[int(f[3, 0])] = np.nan
    keep = ~(f == f[3, 0]).any(1)
    a, b = eng.mesh(T(bad), T(f)), eng.mesh(T(v), T(f[keep]))
    wa, wb = a.winding(p), b.winding(p)
    e = (wa - wb).abs().max().item()
    print(f'{(~keep).sum()} faces dropped: max |with NaN vertex - without those faces| {e:.3e}')
    # the Morton order of the kept faces is the same, so is the sum
    same_bits('dropped faces', wa, wb)
    a.close(), b.close()


def test_empty_query_and_errors(eng):
    v, f = W.hull()
    L = eng.lib
    mesh = eng.mesh(T(v), T(f))
    p = T(W.point_sets('hull')['near'][:10])
    out = torch.empty(10, device='cuda:0')
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert L.ra_mesh_winding(eng.ctx, mesh._handle, None, 0, 0, None, eng.stream) == 0                   # n == 0: no pointer is read
    assert mesh.winding(torch.empty(0, 3)).shape == (0,)
    for args, word in (((None, mesh._handle, ptr(p), 10, 0, ptr(out)), 'null argument'), ((eng.ctx, None, ptr(p), 10, 0, ptr(out)), 'null argument'),
                       ((eng.ctx, mesh._handle, None, 10, 0, ptr(out)), 'null argument'), ((eng.ctx, mesh._handle, ptr(p), 10, 0, None), 'null argument'),
                       ((eng.ctx, mesh._handle, ptr(p), -1, 0, ptr(out)), 'bad sizes'), ((eng.ctx, mesh._handle, ptr(p), 1 << 30, 0, ptr(out)), 'bad sizes'),
                       ((eng.ctx, mesh._handle, ptr(p), 10, 4, ptr(out)), 'unknown flag'), ((eng.ctx, mesh._handle, ptr(p), 10, 3, ptr(out)), 'unknown flag'),
                       ((eng.ctx, C.c_void_p(out.data_ptr()), ptr(p), 10, 0, ptr(out)), 'not a mesh of this ctx')):
        assert L.ra_mesh_winding(*args, eng.stream) != 0
        msg = L.ra_last_error().decode()
        print(f'{word}: {msg}')
        assert word in msg
    other = eng.mesh(T(v), T(f))
    other.close()
    with pytest.raises(RaError, match='closed'):
        other.winding(p)
    with pytest.raises(ValueError):
        mesh.winding(p, shape='both')
    assert [L.ra_winding_tile(k) for k in range(4)] == [64, 1024, 2048, 0]
    # the context works afterwards
    parity('after the errors', mesh.winding(T(W.point_sets('hull')['near'])), restated('hull', 'near'), golden()['hull/near/w64'])
    mesh.close()


# ------------------------------------------------------------------------------------------------ mesh_utils
def test_winding_number_is_mesh_winding(eng):
    v, f = W.mesh_case('opened')
    p = T(W.point_sets('opened')['near'])
    mesh = eng.mesh(T(v), T(f))
    base = mesh.winding(p)
    mesh.close()
    same_bits('winding_number', mesh_utils.winding_number(p, T(v), torch.from_numpy(f), engine=eng), base)
    same_bits('winding_number_nooom', mesh_utils.winding_number_nooom(p, T(v), torch.from_numpy(f), quota_GB=0.001, engine=eng), base)
    same_bits('host inputs', mesh_utils.winding_number(p.cpu(), torch.from_numpy(v), torch.from_numpy(f), engine=eng), base)
    with pytest.raises(ValueError):
        mesh_utils.winding_number(p[None], T(v)[None], torch.from_numpy(f)[None], engine=eng)


@functools.lru_cache(None)
def distance_refs():
    """every third grid point against the opened hull: the plain distance in float64 and in the float32 restatement"""
    v, f = W.mesh_case('opened')
    p = W.point_sets('opened')['grid'][::3]
    return np.sqrt(M.closest_point(p, v, f, np.float64)[0]), np.sqrt(M.closest_point(p, v, f, np.float32)[0])


@pytest.mark.parametrize('th', W.THRESHOLDS)
def test_winding_distance(eng, th):
    """sign and clamp state exactly on every grid point whose float64 winding number is further from a threshold than the measured
    winding error; the magnitude under the 10 x rule (on every third point: the distance references are the slow part)"""
    v, f = W.mesh_case('opened')
    p = W.point_sets('opened')['grid']
    w64, r32 = golden()['opened/grid/w64'], restated('opened', 'grid')
    got = mesh_utils.winding_distance(T(p), T(v), torch.from_numpy(f), winding_th=th, engine=eng).cpu().numpy()
    mesh = eng.mesh(T(v), T(f))
    w, d = mesh.winding(T(p)).cpu().numpy(), mesh.closest(T(p), want=('d2',)).d2.sqrt().cpu().numpy()
    mesh.close()
    err = np.abs(w.astype(np.float64) - w64).max()
    margin = W.threshold_margin(w64, 0.5, th)
    keep = margin > err
    print(f'th {th}: measured winding error {err:.3e}; {(~keep).sum()} of {len(p)} points within it of a threshold (at most 1 %); '
          f'the reference alone: {(margin < 1e-4).sum()} within 1e-4, {(margin < 1e-3).sum()} within 1e-3')
    assert (~keep).sum() <= 0.01 * len(p)
    state = W.shift_state(w64, 0.5, th)
    got_state = np.where(np.abs(got) == d, np.sign(got), 0)               # clamped: exactly +-d
    free = keep & (state == 0)
    print(f'th {th}: clamped low {(state == -1).sum()}, free {(state == 0).sum()}, clamped high {(state == 1).sum()}')
    assert np.array_equal(got_state[keep & (state != 0)], state[keep & (state != 0)])
    assert (np.abs(got[free]) < d[free]).all() and np.array_equal(np.sign(got[free]), np.sign(w64[free] - 0.5))
    assert np.array_equal(np.sign(got[keep]), np.sign(W.winding_shift(w64, 0.5, th))[keep])
    # the composition itself: the library's own winding number through the shift's three lines, times its own distance
    assert np.array_equal(got, W.winding_shift(w, 0.5, th) * d)
    d64, d32 = distance_refs()
    sub = slice(None, None, 3)
    ref64 = W.winding_shift(w64[sub], 0.5, th) * d64
    ref32 = W.winding_shift(r32[sub], 0.5, th) * d32                     # float32 throughout
    parity(f'th {th}: |winding distance|', np.abs(got[sub]), np.abs(ref32), np.abs(ref64), keep=keep[sub])


@functools.lru_cache(None)
def remeshed(eng):
    v, f = W.mesh_case('opened')
    return mesh_utils.winding_distance_remesh(T(v), torch.from_numpy(f), engine=eng, return_cube=True, **REMESH)


def test_remesh_cube_and_result_by_hand(eng):
    v, f = W.mesh_case('opened')
    mv, mf, cube, wbounds = remeshed(eng)
    vs, th_v, th_t = REMESH['voxel_size'], REMESH['dist_th_verts'], REMESH['dist_th_tris']
    tv = T(v)
    pts, wb = mesh_utils.get_voxel_grid_and_update_bounds([vs] * 3, mesh_utils.get_bounds(tv[None], th_t))
    sh = pts.shape[1:-1]
    pts = pts.view(-1, 3)
    near_v = mesh_utils.sample_closest_points(pts[None], tv[None])[0, :, 0] < th_v
    mesh = eng.mesh(tv, T(f))
    d = mesh.closest(pts[near_v], want=('d2',)).d2.sqrt()
    near_t = d < th_t
    wd = mesh_utils.winding_shift(mesh.winding(pts[near_v][near_t]), 0.5, 0.75) * d[near_t]
    mesh.close()
    by_hand = torch.full((pts.shape[0],), -10.0, device='cuda:0')
    idx = torch.nonzero(near_v)[:, 0][near_t]
    by_hand[idx] = wd
    print(f'grid {tuple(sh)}: {int(near_v.sum())} past the vertex filter, {int(near_t.sum())} past the surface filter, {int((by_hand > 0).sum())} inside')
    assert tuple(sh) == tuple(cube.shape) == W.remesh_grid(v, vs, th_t).shape[:3] and torch.equal(wb[0], wbounds)
    same_bits('cube', cube.reshape(-1), by_hand)
    cv, cf = eng.largest_component(*eng.marching_cubes(cube, 0.0))
    same_bits('vertices', mv, cv * vs + wbounds[0])
    assert torch.equal(mf.cpu(), cf.cpu().to(mf.dtype)) and mf.dtype == torch.from_numpy(f).dtype and mv.dtype == torch.float32


def test_remesh_is_closed_one_component_and_inside_where_the_cube_is(eng):
    v, f = W.mesh_case('opened')
    mv, mf, cube, wbounds = remeshed(eng)
    faces = mf.cpu().numpy()
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    counts = np.unique(e, axis=0, return_counts=True)[1]
    labels = X.face_labels(faces)
    figures = X.mesh_figures(mv.cpu().numpy(), faces)
    print(f'{len(mv)} vertices, {len(faces)} faces, {len(counts)} edges, faces per edge {counts.min()} .. {counts.max()}, components {len(np.unique(labels))}, {figures}')
    assert len(faces) > 1000 and (counts == 2).all() and len(np.unique(labels)) == 1 and figures['unmatched'] == 0
    # its own winding number at the grid points at least one voxel from it rounds to the sign of the cube there; the shell of material
    # is at most two voxels thick (dist_th_tris), so its inside is held at half a voxel
    vs = REMESH['voxel_size']
    g = T(W.remesh_grid(v, vs, REMESH['dist_th_tris']).reshape(-1, 3))
    mesh = eng.mesh(mv, mf)
    dist, w = mesh.closest(g, want=('d2',)).d2.sqrt(), mesh.winding(g)
    mesh.close()
    inside = cube.reshape(-1) > 0
    voxel, half = dist >= vs, (dist >= vs / 2) & inside
    print(f'{int(voxel.sum())} grid points at least a voxel away ({int((voxel & inside).sum())} inside), {int(half.sum())} inside ones half a voxel away; '
          f'winding there {w[voxel].min().item():.5f} .. {w[voxel].max().item():.5f} and {w[half].min().item():.5f} .. {w[half].max().item():.5f}')
    assert int(voxel.sum()) > 1000 and int(half.sum()) > 100
    assert torch.equal(torch.round(w[voxel]), inside[voxel].float()) and bool((torch.round(w[half]) == 1).all())


def test_hierarchical_remesh_is_two_calls(eng):
    v, f = W.mesh_case('opened')
    tv, tf = T(v), torch.from_numpy(f)
    vs, th_v, th_t = 0.08, 0.4, 0.16
    got = mesh_utils.hierarchical_winding_distance_remesh(tv, tf, init_voxel_size=vs, init_dist_th_verts=th_v, init_dist_th_tris=th_t, steps=2, engine=eng)
    decay = np.power(th_t / (vs / 2 ** 0), 1 / 1)
    g1 = mesh_utils.winding_distance_remesh(tv, tf, tv, tf, vs, th_v, th_t, engine=eng)
    g2 = mesh_utils.winding_distance_remesh(tv, tf, g1[0], g1[1], vs / 2, th_v / decay, th_t / decay, engine=eng)
    print(f'decay {decay}: step 1 {len(g1[1])} faces at voxel {vs}, step 2 {len(g2[1])} faces at voxel {vs / 2}')
    same_bits('vertices', got[0], g2[0])
    assert torch.equal(got[1], g2[1]) and len(g2[1]) > len(g1[1]) > 100
    with pytest.raises(NotImplementedError):
        mesh_utils.sample_closest_points(torch.zeros(2, 4, 3), torch.zeros(2, 5, 3))

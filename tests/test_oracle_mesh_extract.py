"""Mesh extraction without a GPU: the numpy marching cubes and the component rule of tests/mesh_extract_ref.py are pinned on their own,
by properties that follow from the input volume alone and hold for any correct marching cubes (mcubes and trimesh are not installed:
no golden of either exists, and none is pretended).  tests/test_gpu_mesh_extract.py then holds the device to these restatements bit
for bit.  The two share one triangle table (relightableavatar_amd/mcubes_tables.py, derived by rule), so that equality says nothing
about the table: the property list below is what vouches for it.

The property list (mesh_extract_ref.check_properties and the tests below):
  1. the number of vertices equals the number of grid edges whose ends straddle iso;
  2. every vertex lies on such an edge at the float32 restatement's t, bit for bit;
  3. every undirected mesh edge belongs to exactly two faces, with opposite directions (closed, consistently oriented);
  4. sphere and torus: one component, Euler characteristic 2 and 0, positive signed volume within the linear-interpolation bound that
     mesh_extract_ref.sphere_volume_bounds / torus_volume_bounds derive from the voxel size;
  5. every face index is in range and no face repeats a vertex index;
  6. a volume without a crossing gives (0, 0);
  7. corners exactly equal to iso keep 1-3."""
import os
import re

import numpy as np
import pytest

from relightableavatar_amd import _lib
from relightableavatar_amd import mcubes_tables as T

import mesh_extract_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tables_header_is_the_generated_one():
    """csrc/ra_mcubes_tables.hpp is what the rule of mcubes_tables.py gives; no case needs more than five triangles and no diagonal of a
    case lies in a cube face (where it could coincide with the neighbour cell's)"""
    hdr = open(os.path.join(REPO, 'relightableavatar_amd', 'csrc', 'ra_mcubes_tables.hpp')).read()
    assert hdr == T.header_text()
    edge_table, n_tri, tri_table, bad = T.build_tables()
    print('triangles per case: max', int(n_tri.max()), 'total', int(n_tri.sum()), '; in-face diagonals', int(bad.sum()))
    assert T.MAX_TRI == 5 and n_tri[0] == n_tri[255] == 0 and bad.sum() == 0
    assert [bin(int(e)).count('1') for e in edge_table[[0, 1, 3, 255]]] == [0, 3, 4, 0]
    assert tri_table[1, :3].tolist() == [0, 8, 3]       # the classic numbering: corner 0 below cuts edges 0, 8, 3


def test_numpy_marching_cubes_all_256_patterns():
    total = dict(n_verts=0, n_faces=0, faces_leaning_back=0)
    for case in range(256):
        vol = R.pattern_volume(case)
        v, f = R.marching_cubes(vol, 0.0)
        fig = R.check_properties(vol, 0.0, v, f)
        wrong, leaning = R.normals_towards_smaller(vol, 0.0, v, f)
        assert wrong == 0, (case, wrong)
        total['faces_leaning_back'] += leaning
        if case == 255:
            assert (len(v), len(f)) == (0, 0)
        else:
            assert len(f) > 0 and R.signed_volume(v, f) > 0, case     # some corner is inside: the surface encloses it
        total['n_verts'] += fig['n_verts']
        total['n_faces'] += fig['n_faces']
    print('256 patterns:', total)
    v, f = R.marching_cubes(R.all_patterns_volume(), 0.0)
    assert (len(v), len(f)) == (total['n_verts'], total['n_faces'])


@pytest.mark.parametrize('name', ['sphere', 'torus'])
def test_numpy_marching_cubes_smooth_volumes(name):
    vol = R.sphere_volume() if name == 'sphere' else R.torus_volume()
    v, f = R.marching_cubes(vol, 0.0)
    fig = R.check_properties(vol, 0.0, v, f)
    n_comp = len(np.unique(R.face_labels(f)))
    chi, sv = R.euler(v, f), R.signed_volume(v, f)
    if name == 'sphere':
        lo, hi, exact, want_chi = *R.sphere_volume_bounds(R.SPHERE['R']), 4 / 3 * np.pi * R.SPHERE['R'] ** 3, 2
    else:
        lo, hi, exact, want_chi = *R.torus_volume_bounds(R.TORUS['R'], R.TORUS['r']), 2 * np.pi ** 2 * R.TORUS['R'] * R.TORUS['r'] ** 2, 0
    print(name, fig, 'components', n_comp, 'euler', chi, f'signed volume {sv:.2f} (analytic {exact:.2f}, bound [{lo:.2f}, {hi:.2f}])')
    assert n_comp == 1 and chi == want_chi
    assert sv > 0 and lo <= sv <= hi
    assert R.normals_towards_smaller(vol, 0.0, v, f)[0] == 0


def test_numpy_marching_cubes_random_volume():
    """uniform random values: every face of every cell ambiguous now and then.  The table draws the same segments on both sides of a
    cell face, so edge-manifoldness (property 3) is asserted here too, not only on the smooth volumes"""
    vol = R.random_volume()
    v, f = R.marching_cubes(vol, 0.0)
    fig = R.check_properties(vol, 0.0, v, f)
    print('random 9x10x11:', fig, 'components', len(np.unique(R.face_labels(f))))
    assert fig['n_faces'] > 500
    assert R.normals_towards_smaller(vol, 0.0, v, f)[0] == 0


def test_numpy_marching_cubes_no_crossing_and_exact_iso():
    for fill in (-1.0, 2.0):
        v, f = R.marching_cubes(np.full((3, 4, 5), fill, np.float32), 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3)                                       # 6
    vol = R.exact_iso_volume()
    v, f = R.marching_cubes(vol, 0.0)
    fig = R.check_properties(vol, 0.0, v, f)                                                 # 7
    coincident = len(v) - len(np.unique(v, axis=0))
    print('corners equal to iso:', fig, 'coincident vertices', coincident)
    assert coincident > 0, 'the volume is meant to put several vertices on one grid point'
    nan = R.pattern_volume(0)
    nan[1, 1, 1] = np.nan               # not below: inside, like the corner it replaces
    vn, fn = R.marching_cubes(nan, 0.0)
    v0, f0 = R.marching_cubes(R.pattern_volume(0), 0.0)
    assert np.array_equal(fn, f0) and np.isnan(vn).any()


def test_interp32_is_float32_step_by_step():
    a, b, iso = np.float32(-0.3), np.float32(0.7), np.float32(0.1)
    t = np.float32(np.float32(iso - a) / np.float32(b - a))
    assert R.interp32(5, a, b, iso) == np.float32(np.float32(5) + t)
    assert R.interp32(5, a, b, iso).dtype == np.float32


def test_numpy_largest_component_rule():
    big, small = R.sphere_mesh((0, 0, 0), 5.0), R.sphere_mesh((20, 0, 0), 3.0)
    nb, ns = len(big[0]), len(small[0])
    # the small one first: the largest is not the first
    v = np.concatenate([small[0], big[0]])
    f = np.concatenate([small[1], big[1] + ns])
    ov, of = R.largest_component(v, f)
    assert np.array_equal(ov, big[0]) and np.array_equal(of, big[1])
    # two equal ones: the one with the lowest face index, even when its vertices come second
    a, b = R.sphere_mesh((0, 0, 0), 4.0), R.sphere_mesh((20, 0, 0), 4.0)
    v = np.concatenate([b[0], a[0]])
    f = np.concatenate([a[1] + len(b[0]), b[1]])
    ov, of = R.largest_component(v, f)
    assert np.array_equal(ov, a[0]) and np.array_equal(of, a[1])
    # two triangles that share a vertex only are two components; sharing an edge, one
    tri = np.array([[0, 1, 2], [2, 3, 4]])
    assert len(np.unique(R.face_labels(tri))) == 2
    assert len(np.unique(R.face_labels(np.array([[0, 1, 2], [2, 1, 3]])))) == 1
    pts = np.arange(15, dtype=np.float32).reshape(5, 3)
    ov, of = R.largest_component(pts, tri)
    assert np.array_equal(ov, pts[:3]) and np.array_equal(of, tri[:1])
    ov, of = R.largest_component(np.zeros((0, 3)), np.zeros((0, 3)))
    assert ov.shape == (0, 3) and of.shape == (0, 3)
    print('largest component: vertices', nb, 'against', ns)


def test_mesh_grid_axes_are_the_reference_aranges():
    """bit for bit torch.arange(lo, hi + vs, vs) on the synthetic body's bounds: the axis lengths are arange's, not a re-derivation"""
    import torch
    from relightableavatar_amd import data_utils, synthetic
    body = synthetic.make_body(0, posed=True)
    tv = body.tverts[0]
    for name, b in (('tbounds', torch.stack([tv.min(0).values - 0.05, tv.max(0).values + 0.05])), ('wbounds', body.wbounds[0] if 'wbounds' in body else None)):
        if b is None:
            continue
        for vs in ([0.005] * 3, [0.03, 0.02, 0.025]):
            axes = data_utils.mesh_grid_axes(b, vs)
            want = [torch.arange(b[0, k], b[1, k] + vs[k], vs[k]) for k in range(3)]
            print(name, vs, [len(a) for a in axes])
            assert all(torch.equal(a, w) and a.dtype == w.dtype for a, w in zip(axes, want))
            if vs[0] > 0.01:
                pts = data_utils.mesh_grid_pts(axes)
                assert pts.shape == (len(axes[0]), len(axes[1]), len(axes[2]), 3) and pts.dtype == torch.float32
                assert torch.equal(pts[3, 2, 1], torch.stack([axes[0][3], axes[1][2], axes[2][1]]).float())
    assert all(torch.equal(a, w) for a, w in zip(data_utils.mesh_grid_axes(b.numpy(), vs), want))


def _read_ply(path):
    """a reader of its own: header by lines, then the two binary blocks"""
    raw = open(path, 'rb').read()
    head, body = raw.split(b'end_header\n', 1)
    lines = head.decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    nv = int(next(l for l in lines if l.startswith('element vertex')).split()[-1])
    nf = int(next(l for l in lines if l.startswith('element face')).split()[-1])
    assert [l for l in lines if l.startswith('property')] == ['property float x', 'property float y', 'property float z',
                                                             'property list uchar int vertex_indices']
    v = np.frombuffer(body[:12 * nv], '<f4').reshape(nv, 3)
    faces = []
    off = 12 * nv
    for _ in range(nf):
        assert body[off] == 3
        faces.append(np.frombuffer(body[off + 1:off + 13], '<i4'))
        off += 13
    assert off == len(body)
    return v, np.array(faces).reshape(nf, 3)


def test_mesh_visualizer_writes_ply_and_npz_under_the_reference_names(tmp_path):
    import torch
    from relightableavatar_amd import config
    from relightableavatar_amd.base_utils import dotdict
    from relightableavatar_amd.visualizers import mesh_visualizer
    v, f = R.marching_cubes(R.sphere_volume(), 0.0)
    out = dotdict(verts=torch.from_numpy(v), faces=torch.from_numpy(f), weights=torch.rand(len(v), 4))
    batch = dotdict(meta=dotdict(latent_index=torch.tensor([3]), frame_index=torch.tensor([17]), view_index=torch.tensor([0])))
    old = config.active_cfg()
    try:
        for switches, latent, want in ((dict(vis_can_mesh=True), 3, 'can_mesh'), (dict(vis_posed_mesh=True), 3, 'posed_mesh/0017'),
                                       (dict(vis_tpose_mesh=True), 3, 'tpose_mesh/0017'),
                                       (dict(vis_tpose_mesh=True, track_tpose_mesh=True), 3, 'track_mesh/0017'),
                                       (dict(vis_tpose_mesh=True, track_tpose_mesh=True), -1, 'can_mesh')):
            cfg = config.default_cfg()
            cfg.update(switches)
            config.set_active_cfg(cfg)
            batch.meta.latent_index = torch.tensor([latent])
            vis = mesh_visualizer.Visualizer(result_dir=str(tmp_path))
            npz, ply = vis.visualize(out, batch)
            assert (npz, ply) == (str(tmp_path / (want + '.npz')), str(tmp_path / (want + '.ply')))
            pv, pf = _read_ply(ply)
            assert np.array_equal(pv.view(np.uint32), v.view(np.uint32)) and np.array_equal(pf, f)
            z = np.load(npz)
            assert sorted(z.files) == ['faces', 'verts', 'weights'] and np.array_equal(z['verts'], v) and z['faces'].dtype == np.int32
        config.set_active_cfg(config.default_cfg())
        with pytest.raises(ValueError):
            mesh_visualizer.Visualizer(result_dir=str(tmp_path)).result_paths(batch)
    finally:
        config.set_active_cfg(old)
    print('ply:', os.path.getsize(ply), 'bytes for', len(v), 'vertices and', len(f), 'faces')


def test_config_refuses_mesh_simplification_and_selects_the_mesh_renderer():
    from relightableavatar_amd import config
    cfg = config.make_cfg('relight')
    config.check_supported(cfg)
    assert cfg.voxel_size == [0.005] * 3 and cfg.mesh_th == 0.5 and cfg.mesh_th_to_sdf is False and cfg.mesh_simp_face == -1
    assert cfg.surface_blend_weight is False and not (cfg.vis_can_mesh or cfg.vis_tpose_mesh or cfg.vis_posed_mesh or cfg.track_tpose_mesh)
    for key, value in (('mesh_simp_face', 16384), ('track_tpose_mesh', True)):
        with pytest.raises(NotImplementedError, match=key):
            config.check_supported(config.make_cfg('relight', **{key: value}))
    from relightableavatar_amd.renderer import make_renderer, mesh_renderer
    old = config.active_cfg()
    try:
        for key in ('vis_can_mesh', 'vis_tpose_mesh', 'vis_posed_mesh'):        # config.py:507: the mesh renderer is selected
            assert isinstance(make_renderer(config.make_cfg('relight', **{key: True}), None), mesh_renderer.Renderer)
        with pytest.raises(NotImplementedError, match='mesh_simp_face'):
            make_renderer(config.make_cfg('relight', vis_can_mesh=True, mesh_simp_face=16384), None)
    finally:
        config.set_active_cfg(old)
    assert abs(mesh_renderer.alpha2sdf(0.5, 0.1) - 0.1 * np.log(2 * 0.1 * (-np.log(0.5) / 0.005))) < 1e-12


def test_sample_blend_K_closest_points_restated():
    """against the reference's own lines restated on a brute-force K-NN in float64 (sample_utils.py:605-611,631-646): the plain
    distances are weighted, the weights sum to 1"""
    import torch
    from relightableavatar_amd import mesh_utils
    g = torch.Generator().manual_seed(0)
    src, ref, val = torch.randn(1, 257, 3, generator=g), torch.randn(1, 301, 3, generator=g), torch.rand(1, 301, 24, generator=g)
    ref[0, 7] = src[0, 5]                                   # a point on a vertex: distance 0, weight 1 / eps
    for K in (1, 3, 4):
        d = (src[0].double()[:, None] - ref[0].double()[None]).norm(dim=-1)
        top = torch.topk(d, K, dim=-1, largest=False)
        w = 1 / (top.values + 1e-8)
        w = w / w.sum(-1, keepdim=True)
        want_d, want_v = (top.values * w).sum(-1), torch.einsum('nkd,nk->nd', val[0].double()[top.indices], w)
        only = mesh_utils.sample_blend_K_closest_points(src, ref, K=K)
        got_v, got_d = mesh_utils.sample_blend_K_closest_points(src, ref, val, K=K)
        err_d, err_v = float((got_d[0, :, 0] - want_d).abs().max()), float((got_v[0] - want_v).abs().max())
        print('K', K, 'max |dist - ref|', err_d, 'max |values - ref|', err_v)
        assert only.shape == (1, 257, 1) and torch.equal(only, got_d) and got_v.shape == (1, 257, 24)
        assert err_d <= 16 * 2.0 ** -23 * float(want_d.max()) and err_v <= 16 * 2.0 ** -23          # a handful of float32 roundings of values <= 1
    with pytest.raises(NotImplementedError):
        mesh_utils.sample_blend_K_closest_points(src.expand(2, -1, -1), ref.expand(2, -1, -1))


@pytest.mark.parametrize('mode', ['tpose', 'posed'])
def test_oracle_volume_filter_stays_clear_of_the_threshold(mode):
    """the seed and voxel size of the GPU volume test: about 2 * 10^4 points, axis lengths no multiple of a wave, and at most 0.1 % of the
    cells with a t within 4 float32 roundings of the configuration's dist_th, from the oracle alone (canonical shares tpose's grid and vertices)"""
    body, axes, verts = R.volume_inputs(mode)
    pts, t = R.oracle_filter(axes, verts, 3)
    th = 0.125      # make_cfg('relight').dist_th
    share = float(R.borderline(t, th).double().mean())
    print(mode, [len(a) for a in axes], len(t), 'points; kept', int((t < th).sum()), '; borderline share', share)
    assert 1.5e4 <= len(t) <= 3e4 and all(len(a) % 64 for a in axes) and share <= 1e-3
    assert 0.2 < float((t < th).double().mean()) < 0.95, 'the filter must decide something'


def test_library_exports_the_mesh_extraction_symbols():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    hdr = open(os.path.join(REPO, 'include', 'relightableavatar.h')).read()
    for name in ('ra_marching_cubes', 'ra_mesh_largest_component', 'ra_mcubes_tile', 'ra_mesh_extract_stats', 'ra_sdf_volume'):
        assert hasattr(L, name) and name in _lib.SYMBOLS and re.search(r'^int\s+' + name + r'\s*\(', hdr, flags=re.M), name
    assert L.ra_abi_version() == _lib.ABI_VERSION == 9
    assert L.ra_mcubes_tile(0) > 0 and L.ra_mcubes_tile(0) % 64 == 0 and L.ra_mcubes_tile(1) >= 2 and L.ra_mcubes_tile(2) % 64 == 0 and L.ra_mcubes_tile(3) >= 3 and L.ra_mcubes_tile(4) == 0
    assert L.ra_mesh_extract_stats(None, 0) == -1

"""CPU tests of the mesh-distance feature: the numpy reference the GPU tests are held to (tests/mesh_distance_ref.py) is pinned on
analytic cases, on degenerate faces and against an independent dense barycentric grid; mesh_utils.sample_surface and load_obj; the
evaluator's refusal without an engine; the new entry points of the C ABI.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mesh_distance_ref as M
from relightableavatar_amd import _lib, mesh_utils, synthetic
from relightableavatar_amd.config import make_cfg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('ra_mesh_create', 'ra_mesh_destroy', 'ra_mesh_closest', 'ra_mesh_tile')


def hull(n_verts=301):
    """the synthetic body's template (a squashed Fibonacci sphere) and its convex-hull triangulation: 598 faces for 301 vertices"""
    b = synthetic.make_body(0, posed=False, n_verts=n_verts)
    tv = b.tverts[0].numpy().astype(np.float64)
    nrm = tv / (0.4 * np.array([0.8, 0.7, 1.1]))
    return b.tverts[0].numpy(), synthetic._template_faces(nrm)


TRI = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
ANALYTIC = {      # point -> d2, closest, bary
    'above the interior': ([0.25, 0.25, 2.0], 4.0, [0.25, 0.25, 0.0], [0.5, 0.25, 0.25]),
    'beyond edge ab': ([0.5, -1.0, 0.5], 1.25, [0.5, 0.0, 0.0], [0.5, 0.5, 0.0]),
    'beyond edge ac': ([-2.0, 0.25, 0.0], 4.0, [0.0, 0.25, 0.0], [0.75, 0.0, 0.25]),
    'beyond edge bc': ([1.0, 1.0, 0.0], 0.5, [0.5, 0.5, 0.0], [0.0, 0.5, 0.5]),
    'beyond vertex a': ([-1.0, -1.0, 1.0], 3.0, [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]),
    'beyond vertex b': ([2.0, -1.0, 0.0], 2.0, [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]),
    'beyond vertex c': ([-0.5, 3.0, 0.0], 4.25, [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]),
    'on the surface': ([0.25, 0.5, 0.0], 0.0, [0.25, 0.5, 0.0], [0.25, 0.25, 0.5]),
    'on a vertex': ([1.0, 0.0, 0.0], 0.0, [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]),
}


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('name', list(ANALYTIC))
def test_reference_analytic_cases(name, dtype):
    p, d2, q, bary = ANALYTIC[name]
    for shift in (0, 1, 2):          # every rotation of the vertex order: the regions are not symmetric in a, b, c
        order = np.roll(np.arange(3), shift)
        g2, gq, gf, gb = M.closest_point([p], TRI[order], [[0, 1, 2]], dtype)
        assert g2.dtype == dtype and gf[0] == 0
        np.testing.assert_allclose(g2[0], d2, rtol=0, atol=1e-6)
        np.testing.assert_allclose(gq[0], q, rtol=0, atol=1e-6)
        np.testing.assert_allclose(gb[0], np.asarray(bary)[order], rtol=0, atol=1e-6)


def _segment_d2(p, a, b):
    e = b - a
    l2 = (e * e).sum(-1)
    t = np.clip(((p - a) * e).sum(-1) / np.where(l2 > 0, l2, 1), 0, 1) * (l2 > 0)
    d = p - (a + t[..., None] * e)
    return (d * d).sum(-1)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_reference_degenerate_faces_act_as_segment_or_point(dtype):
    r = np.random.default_rng(0)
    n = 300
    a, b = r.uniform(-1, 1, (n, 3)), r.uniform(-1, 1, (n, 3))
    t = r.uniform(-1.5, 2.5, (n, 1))
    c = a + t * (b - a)                         # collinear, c before a, between and beyond b
    c[:50] = b[:50]                             # a repeated vertex
    b[50:100] = a[50:100]
    c[100:130] = b[100:130] = a[100:130]        # a point
    a, b, c = (x.astype(np.float32).astype(np.float64) for x in (a, b, c))
    p = r.uniform(-2, 2, (n, 3)).astype(np.float32).astype(np.float64)
    want = np.minimum(np.minimum(_segment_d2(p, a, b), _segment_d2(p, a, c)), _segment_d2(p, b, c))
    d2, q, bary = M.closest_on_triangles(p.astype(dtype), a.astype(dtype), b.astype(dtype), c.astype(dtype))
    assert np.isfinite(d2).all() and np.isfinite(q).all() and np.isfinite(bary).all()
    # c was rounded to float32, so the face is collinear only to 2^-24 of its size: the segment distance to that accuracy
    tol = 1e-6 if dtype == np.float64 else 1e-5
    err = np.abs(np.sqrt(d2.astype(np.float64)) - np.sqrt(want))
    print(f'degenerate faces, {np.dtype(dtype).name}: max |d - segment distance| {err.max():.2e}')
    assert err.max() <= tol
    assert np.abs(bary.sum(-1) - 1).max() <= 1e-6 and bary.min() >= -1e-6
    rebuilt = bary[:, :1] * a + bary[:, 1:2] * b + bary[:, 2:] * c
    assert np.abs(rebuilt - q).max() <= 1e-5
    # exactly collinear and exactly repeated: the analytic answers
    line = np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]])
    for pt, want2 in (([1.5, 1, 0], 1.0), ([3, 0, 1], 2.0), ([-1, 0, 0], 1.0), ([0.5, 0, 2], 4.0)):
        assert M.closest_point([pt], line, [[0, 1, 2]], dtype)[0][0] == want2
    assert M.closest_point([[1, 1, 3]], np.ones((3, 3)), [[0, 1, 2]], dtype)[0][0] == 4.0
    assert M.closest_point([[1, 0, 0.5]], np.array([[0.0, 0, 0], [0, 0, 0], [0, 0, 1]]), [[0, 1, 2]], dtype)[0][0] == 1.0


def test_reference_against_a_dense_barycentric_grid():
    """independent of the region logic: the minimum over a grid of barycentric points of every face is an upper bound of the
    distance to that face, and within the grid's spacing of it"""
    verts, faces = hull()
    verts = verts.astype(np.float64)
    tri = verts[faces]                                                    # (F,3,3)
    r = np.random.default_rng(1)
    cen = tri.mean(1)
    p = np.concatenate([cen[r.integers(0, len(faces), 24)] * r.uniform(0.5, 1.8, (24, 1)), verts[:4], r.uniform(-1, 1, (4, 3))])
    m = 24
    i, j = np.meshgrid(np.arange(m + 1), np.arange(m + 1), indexing='ij')
    keep = i + j <= m
    v, w = i[keep] / m, j[keep] / m
    grid = (1 - v - w)[None, :, None] * tri[:, None, 0] + v[None, :, None] * tri[:, None, 1] + w[None, :, None] * tri[:, None, 2]      # (F,G,3)
    dgrid = np.sqrt(((p[:, None, None] - grid[None]) ** 2).sum(-1)).min(-1)                                                            # (N,F)
    dref = np.sqrt(M.closest_on_triangles(p[:, None], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])[0])
    edge = np.sqrt(((tri - np.roll(tri, 1, 1)) ** 2).sum(-1)).max(1)
    print(f'grid minimum - reference: min {(dgrid - dref).min():.2e}, max {(dgrid - dref).max():.2e}, spacing {(edge / m).max():.2e}')
    assert (dgrid - dref >= -1e-12).all()
    assert (dgrid - dref <= edge[None] / m).all()
    d2, q, f, bary = M.closest_point(p, verts, faces)
    np.testing.assert_allclose(np.sqrt(d2), dref.min(1), rtol=0, atol=0)
    assert (f == dref.argmin(1)).all()


def test_reference_non_finite_inputs():
    verts, faces = hull()
    bad = verts.copy()
    bad[faces[7, 1]] = np.nan
    p = np.array([[0.0, 0, 1], [np.inf, 0, 0], [0, np.nan, 0]])
    d2, q, f, bary = M.closest_point(p, bad, faces)
    touched = (faces == faces[7, 1]).any(1)
    assert np.isfinite(d2[0]) and not touched[f[0]] and np.isnan(d2[1:]).all() and (f[1:] == -1).all() and np.isnan(q[1:]).all()
    d2, q, f, bary = M.closest_point(p, np.full_like(verts, np.nan), faces)
    assert d2[0] == np.inf and f[0] == -1 and np.isnan(d2[1:]).all()


# ------------------------------------------------------------------------------------------------ sample_surface, load_obj
def test_sample_surface_points_lie_on_their_faces():
    verts, faces = hull()
    v, f = torch.from_numpy(verts).double(), torch.from_numpy(faces)
    g = torch.Generator().manual_seed(0)
    pts, fid = mesh_utils.sample_surface(v, f, 4000, g)
    assert pts.shape == (4000, 3) and pts.dtype == torch.float64 and fid.dtype == torch.int64 and 0 <= int(fid.min()) and int(fid.max()) < len(faces)
    tri = verts.astype(np.float64)[faces[fid.numpy()]]
    # barycentrics by least squares in float64
    A = np.stack([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]], -1)                 # (n,3,2)
    vw = np.linalg.solve(A.transpose(0, 2, 1) @ A, (A.transpose(0, 2, 1) @ (pts.numpy() - tri[:, 0])[..., None]))[..., 0]
    resid = np.abs((A @ vw[..., None])[..., 0] + tri[:, 0] - pts.numpy()).max()
    print(f'sample_surface: residual off the face plane {resid:.2e}, min barycentric {min(vw.min(), (1 - vw.sum(1)).min()):.2e}')
    assert resid <= 1e-14 and vw.min() >= -1e-12 and (1 - vw.sum(1)).min() >= -1e-12
    assert M.distance_to_face(pts.numpy(), verts, faces, fid.numpy()).max() <= 1e-14
    # float32 vertices give float32 points, the same faces from the same generator state
    p32, f32 = mesh_utils.sample_surface(v.float(), f, 4000, torch.Generator().manual_seed(0))
    assert p32.dtype == torch.float32 and torch.equal(f32, fid) and torch.equal(p32, pts.float())


def _frequencies_follow(counts, prob):
    """every face within six binomial standard deviations (and one count) of its expectation, and the chi-square statistic within
    five standard deviations of its degrees of freedom: conditions a true draw from `prob` misses with probability below 1e-4"""
    n = counts.sum()
    mean, sd = n * prob, np.sqrt(n * prob * (1 - prob))
    chi2, dof = ((counts - mean) ** 2 / mean).sum(), len(prob) - 1
    return bool((np.abs(counts - mean) <= 6 * sd + 1).all()), float(chi2), dof, bool(abs(chi2 - dof) <= 5 * np.sqrt(2 * dof))


def test_sample_surface_face_frequencies_follow_the_areas():
    verts, faces = hull()
    tri = verts.astype(np.float64)[faces]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=-1)
    prob = area / area.sum()
    n = int(np.ceil(30 / prob.min()))              # at least 30 expected samples on the smallest face: the normal approximation's range
    ref_ok, ref_chi2, dof, ref_chi_ok = _frequencies_follow(np.random.default_rng(0).multinomial(n, prob), prob)
    assert ref_ok and ref_chi_ok, 'the condition rejects a true multinomial draw'
    _, fid = mesh_utils.sample_surface(torch.from_numpy(verts), torch.from_numpy(faces), n, torch.Generator().manual_seed(0))
    ok, chi2, dof, chi_ok = _frequencies_follow(np.bincount(fid.numpy(), minlength=len(faces)), prob)
    print(f'sample_surface: {n} samples on {len(faces)} faces, chi-square {chi2:.1f} (numpy multinomial: {ref_chi2:.1f}) for {dof} degrees of freedom')
    assert ok and chi_ok


def test_sample_surface_refuses_bad_shapes():
    with pytest.raises(ValueError, match='verts'):
        mesh_utils.sample_surface(torch.zeros(4, 2), torch.zeros(2, 3, dtype=torch.long), 3)


OBJ = """# a tetrahedron
mtllib none.mtl
o tet
v 0 0 0
v 1 0 0 1.0
v 0 1 0
v 0 0 1.5
vn 0 0 1
vt 0.5 0.5
s off
f 1 3 2
f 1/1 2/1 4/1
f 2//1 3//1 4//1
f 1/1/1 4/1/1 3/1/1
"""


def test_load_obj_round_trip(tmp_path):
    path = tmp_path / 'tet.obj'
    path.write_text(OBJ)
    v, f = mesh_utils.load_obj(str(path))
    assert v.dtype == torch.float32 and f.dtype == torch.int64
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]]
    assert f.tolist() == [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]
    # write what was read, read it again
    again = tmp_path / 'again.obj'
    again.write_text(''.join(f'v {x!r} {y!r} {z!r}\n' for x, y, z in v.tolist()) + ''.join(f'f {a + 1} {b + 1} {c + 1}\n' for a, b, c in f.tolist()))
    v2, f2 = mesh_utils.load_obj(again)
    assert torch.equal(v, v2) and torch.equal(f, f2)


@pytest.mark.parametrize('text, message', [
    ('v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nf 1 2 4 3\n', 'only triangles'),
    ('v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n', 'only triangles'),
    ('v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n', 'outside'),
    ('v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n', 'outside'),
    ('v 0 0 0\nv 1 0 0\nv 0 1 0\nf -3 -2 -1\n', 'outside'),
    ('v 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n', 'three coordinates'),
    ('v 0 0 0\nv 1 0 0\nv 0 1 0\n', 'no vertices or no faces'),
    ('# nothing\n', 'no vertices or no faces'),
])
def test_load_obj_refusals(tmp_path, text, message):
    path = tmp_path / 'bad.obj'
    path.write_text(text)
    with pytest.raises(ValueError, match=message):
        mesh_utils.load_obj(str(path))


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic on the host
def test_mesh_arithmetic_native(tmp_path):
    """tests/native/mesh_tri_main.cpp: a stand-alone program (its own main) around csrc/ra_mesh_tri.hpp — the per-triangle function and
    the box bounds the query kernel inlines, in the same IEEE fp32 operations — built with -fsanitize=address,undefined and run on the
    CPU: box bound <= computed d2 <= far-corner bound for 614 400 (point, face) pairs, a third of them on degenerate faces, and the
    identities of the GPU tests."""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'mesh_tri_main')
    static = ['-static-libasan'] if os.path.basename(cxx).startswith('g++') else []          # gcc's spelling; clang links its runtime statically already
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + static +
                       ['-I', os.path.join(REPO, 'relightableavatar_amd', 'csrc'), os.path.join(REPO, 'tests', 'native', 'mesh_tri_main.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and 'mesh arithmetic ok' in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------ the evaluator and the ABI
def test_mesh_evaluator_has_no_cpu_fallback():
    from relightableavatar_amd.evaluators import mesh_evaluator
    verts, faces = hull()
    mesh = {'verts': torch.from_numpy(verts)[None], 'faces': torch.from_numpy(faces)[None]}
    assert mesh_evaluator.Evaluator.engine is None
    ev = mesh_evaluator.Evaluator()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ev.evaluate({'mesh': mesh}, {'obj': [(verts, faces)]})
    with pytest.raises(RuntimeError, match='no frame'):
        ev.summarize()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        mesh_evaluator.MeshEvaluator().set_src_mesh(mesh)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        mesh_utils.bvh_distance(torch.zeros(2, 3), torch.from_numpy(verts), torch.from_numpy(faces))
    with pytest.raises(NotImplementedError, match='B > 1'):
        mesh_utils.sample_closest_points_on_surface(torch.zeros(2, 5, 3), torch.zeros(2, 4, 3), torch.zeros(2, 2, 3, dtype=torch.long))


def test_make_evaluator_selects_the_mesh_evaluator():
    from relightableavatar_amd.evaluators import make_evaluator, mesh_evaluator
    ev = make_evaluator(make_cfg('relight', evaluator_module='relightableavatar_amd.evaluators.mesh_evaluator'))
    assert type(ev) is mesh_evaluator.Evaluator


def test_mesh_inputs_are_recognised():
    from relightableavatar_amd.evaluators.mesh_evaluator import _as_mesh
    verts, faces = hull()

    class Tri:
        vertices, faces = verts, None
    Tri.faces = faces
    for m in (Tri(), {'verts': torch.from_numpy(verts)[None], 'faces': torch.from_numpy(faces)[None]}, (verts, faces)):
        v, f = _as_mesh(m, 'test')
        assert tuple(v.shape) == verts.shape and tuple(f.shape) == faces.shape
    with pytest.raises(TypeError, match='expected'):
        _as_mesh(3, 'test')
    with pytest.raises(ValueError, match='must be'):
        _as_mesh((verts[:, :2], faces), 'test')


def test_mesh_entry_points_are_exported_and_bound():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes == _lib.SYMBOLS[name][1]
    leaf, fan, unsorted = L.ra_mesh_tile(0), L.ra_mesh_tile(1), L.ra_mesh_tile(2)
    assert leaf >= 1 and fan >= 1 and unsorted >= 0 and L.ra_mesh_tile(99) == 0
    assert (_lib.RA_MESH_BRUTE, _lib.RA_MESH_UNSORTED) == (1, 2)
    # argument checks that need no device: a null context and a null output are refused with their messages
    import ctypes as C
    assert L.ra_mesh_create(None, None, 0, None, 0, None, None) == 1 and b'null argument' in L.ra_last_error()
    assert L.ra_mesh_closest(None, None, None, 0, 0, None, None, None, None, None) == 1 and b'null argument' in L.ra_last_error()
    assert L.ra_mesh_destroy(None, None) == 1 and b'null argument' in L.ra_last_error()

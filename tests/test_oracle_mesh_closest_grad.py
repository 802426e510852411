"""The backward of the closest-point query without a GPU:
    1. the float64 closed form of tests/mesh_closest_grad_ref.py against float64 central differences of mesh_distance_ref.closest_point,
       for L = sum g_i d2_i along random directions in verts and in pts, on points in face, edge and vertex regions;
    2. the float32 restatement in kernel order — what the device must equal bit for bit — against float64 at the restatement's own faces:
       the error that is the floor of the GPU test's 10 x rule, reported (a sanity bound is asserted);
    3. the run sum's edge cases: vertices with 0, 1, 63, 64, 65, 129 and 257 slots, dead rows between live ones, C in {0, 1, 3, 64};
    4. tests/native/mesh_closest_grad_rules_main.cpp: the header's functions on the CPU under -fsanitize=address,undefined give the
       restatement's bits, and every row's three vertex terms cancel its dpts to 8 x 2^-23;
    5. the exports, the Python layer and the argument errors raised before a context is touched.
Every test prints its figures before it asserts."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mesh_closest_grad_ref as G
import mesh_distance_ref as M
from mesh_closest_grad_ref import generic_points, hull

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -23


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def test_closed_form_against_central_differences():
    v, f = hull()
    p = generic_points()
    rng = np.random.default_rng(17)
    g = rng.uniform(0.5, 1.5, len(p))
    v64, p64 = v.astype(np.float64), p.astype(np.float64)
    d2, q, face, bary = M.closest_point(p64, v64, f, np.float64)
    reg = np.bincount(G.regions(bary), minlength=3)
    print(f'{len(p)} points: {reg[0]} in face regions, {reg[1]} in edge regions, {reg[2]} in vertex regions; distances {np.sqrt(d2.min()):.2e} .. {np.sqrt(d2.max()):.2e}')
    assert reg[0] > 0 and reg[1] > 0 and reg[2] > 0 and d2.min() > 0
    closed = G.backward64(p64, v64, f, face, g_d2=g)
    dv, dp = rng.standard_normal(v64.shape), rng.standard_normal(p64.shape)
    want_v, want_p = (closed['dverts'] * dv).sum(), (closed['dpts'] * dp).sum()
    worst = {}
    for h in (1e-6, 1e-7):
        fd_v = (G.weighted_d2(p64, v64 + h * dv, f, g) - G.weighted_d2(p64, v64 - h * dv, f, g)) / (2 * h)
        fd_p = (G.weighted_d2(p64 + h * dp, v64, f, g) - G.weighted_d2(p64 - h * dp, v64, f, g)) / (2 * h)
        worst[h] = (rel(want_v, fd_v), rel(want_p, fd_p))
        print(f'step {h:g}: d/dverts closed {want_v:.12e} differences {fd_v:.12e} mismatch {worst[h][0]:.2e}; '
              f'd/dpts closed {want_p:.12e} differences {fd_p:.12e} mismatch {worst[h][1]:.2e}')
    assert worst[1e-6][0] <= 1e-6 and worst[1e-6][1] <= 1e-6


def test_float32_restatement_against_float64_at_its_own_faces():
    """Reported: the error of the float32 restatement (the float32 forward's closest point and barycentrics, the kernel's operations)
    against the float64 closed form evaluated at the SAME faces.  It is the floor the GPU test's 10 x rule measures the kernel by.
    What is asserted is only a sanity bound: the float32 closest point of a face differs from the float64 one by the projection's
    conditioning — roundings of size 2^-23 |coord| amplified by at most (reach / shortest edge)^2, about 10^2 on this body — so 10^3
    roundings relative to the largest value is generous and a wrong formula (a factor, a sign, a corner) is 10^3 times beyond it."""
    v, f = hull()
    p = generic_points()
    rng = np.random.default_rng(18)
    g, ga = rng.uniform(0.5, 1.5, len(p)).astype(np.float32), rng.standard_normal((len(p), 3)).astype(np.float32)
    d2, q, face, bary = M.closest_point(p, v, f, np.float32)
    r32 = G.backward32(p, q, face, bary, f, len(v), g, ga)
    r64 = G.backward64(p, v, f, face, g, ga)
    run = np.bincount(f[face].reshape(-1), minlength=len(v)).max()
    for key in ('dpts', 'dverts', 'dattr'):
        err = np.abs(r32[key].astype(np.float64) - r64[key])
        top = np.abs(r64[key]).max()
        print(f'{key}: float32 restatement within max {err.max():.3e} median {np.median(err):.3e} of float64 (max |value| {top:.3e}: {err.max() / top:.2e} relative, '
              f'{err.max() / top / U:.1f} roundings); longest run {run} slots')
        assert err.max() <= 1e3 * U * top, key


@pytest.mark.parametrize('Cn', (0, 1, 3, 64))
def test_run_sum_edge_cases(Cn):
    c = G.run_case(Cn)
    r = G.backward32(c['pts'], c['closest'], c['face'], c['bary'], c['faces'], c['V'], c['g'], c['ga'])
    counts = np.bincount(c['faces'][c['face'][~c['dead']]].reshape(-1), minlength=c['V'])
    print(f'C {Cn}: {len(c["face"])} rows, {int(c["dead"].sum())} dead, slots per vertex {counts.tolist()}')
    assert tuple(counts[:len(G.RUN_COUNTS)]) == G.RUN_COUNTS and c['dead'].sum() == 4
    assert r['dpts'].shape == (len(c['face']), 3) and r['dverts'].shape == (c['V'], 3) and r['dattr'].shape == (c['V'], Cn)
    # the dead rows: +0 in dpts, and their NaN reaches nothing
    assert not r['dpts'][c['dead']].view(np.uint32).any() and np.isfinite(r['dpts'][~c['dead']]).all()
    assert np.isfinite(r['dverts']).all() and np.isfinite(r['dattr']).all()
    # no slot: +0; one slot: the term itself
    assert not r['dverts'][0].view(np.uint32).any() and not r['dattr'][0].view(np.uint32).any()
    one = int(np.flatnonzero(c['face'] == 1)[0])
    assert np.array_equal(r['dverts'][1], -(c['bary'][one, 0] * r['dpts'][one])) and np.array_equal(r['dattr'][1], c['bary'][one, 0] * c['ga'][one])
    # every run against the float64 sum of the same float32 terms: half a rounding per addition of a lane and of the tree
    live = np.flatnonzero(~c['dead'])
    for key, terms in (('dverts', -(c['bary'][live][:, :, None] * r['dpts'][live][:, None, :])), ('dattr', c['bary'][live][:, :, None] * c['ga'][live][:, None, :])):
        terms = terms.astype(np.float32).astype(np.float64)
        want, mag = np.zeros(r[key].shape), np.zeros(r[key].shape)
        for k in range(3):
            np.add.at(want, c['faces'][c['face'][live], k], terms[:, k])
            np.add.at(mag, c['faces'][c['face'][live], k], np.abs(terms[:, k]))
        err = np.abs(r[key] - want)
        allowed = (np.ceil(counts / 64) + 6)[:, None] * U * mag
        print(f'C {Cn}: {key} wave sums within {float((err / np.where(mag > 0, U * mag, 1)).max()) if err.size else 0.0:.2f} x 2^-23 sum|terms| of the float64 sums')
        assert (err <= allowed).all(), key


def _hex(a):
    return ' '.join(f'{v:08x}' for v in np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1).tolist())


def _ints(a):
    return ' '.join(str(int(v)) for v in np.asarray(a).reshape(-1))


@pytest.fixture(scope='module')
def native_exe(tmp_path_factory):
    """tests/native/mesh_closest_grad_rules_main.cpp built once with -fsanitize=address,undefined: a stand-alone program, its own main"""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('mesh_closest_grad_native') / 'mesh_closest_grad_rules_main')
    flags = ['-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    flags += ['-static-libasan'] if os.path.basename(cxx).startswith('g++') else []      # gcc's spelling; clang links its runtime statically already
    r = subprocess.run([cxx] + flags + ['-I', os.path.join(REPO, 'relightableavatar_amd', 'csrc'),
                                        os.path.join(REPO, 'tests', 'native', 'mesh_closest_grad_rules_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def _native_case(name):
    if name.startswith('run'):
        c = G.run_case(int(name[3:]))
        return c['faces'], c['V'], c['face'], c['pts'], c['closest'], c['bary'], c['g'], c['ga'], False
    v, f = hull()
    p = generic_points().copy()
    rng = np.random.default_rng(19)
    Cn = 0 if name == 'hull_c0' else 5
    g, ga = rng.standard_normal(len(p)).astype(np.float32), rng.standard_normal((len(p), Cn)).astype(np.float32)
    p[7], p[100] = np.nan, np.inf                                      # the forward answers face -1: dead rows
    _, q, face, bary = M.closest_point(p, v, f, np.float32)
    return f, len(v), face, p, q, bary, (None if name == 'hull_no_g' else g), ga, name != 'hull_no_g'


@pytest.mark.parametrize('name', ('hull', 'hull_c0', 'hull_no_g', 'run0', 'run1', 'run3', 'run64'))
def test_mesh_closest_grad_rules_native(tmp_path, native_exe, name):
    """the header's functions on the CPU under the sanitizers equal the float32 restatement bit for bit; on a real forward's rows the
    three vertex terms cancel the row's dpts to 8 x 2^-23 |dpts| (the program asserts it)"""
    faces, V, face, p, q, bary, g, ga, identity = _native_case(name)
    want = G.backward32(p, q, face, bary, faces, V, g, ga)
    n, Cn = len(face), ga.shape[1]
    path = str(tmp_path / 'case.txt')
    with open(path, 'w') as fh:
        fh.write(f'{len(faces)} {V} {n} {Cn} {int(g is not None)} {int(identity)}\n{_ints(faces)}\n{_ints(face)}\n{_hex(p)}\n{_hex(q)}\n{_hex(bary)}\n'
                 f'{_hex(g) if g is not None else ""}\n{_hex(ga)}\n')
    r = subprocess.run([native_exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines()}
    print(name, 'live rows', lines['live'], 'identity', lines.get('identity'))
    assert int(lines['live'][0]) == int(G.live_rows(face, faces, V)[0].sum())
    assert identity == ('identity' in lines)
    for key in ('dpts', 'dverts', 'dattr'):
        if want[key] is None:
            assert key not in lines
            continue
        got = np.array([int(t, 16) for t in lines[key]], np.uint32)
        ref = np.ascontiguousarray(want[key], np.float32).view(np.uint32).reshape(-1)
        diff = int((got != ref).sum()) if got.shape == ref.shape else -1
        print(name, key, got.size, 'values,', diff, 'differ')
        assert diff == 0, key


def test_exports_python_layer_and_refusals():
    from relightableavatar_amd import _lib, engine, mesh_utils
    from relightableavatar_amd.base_utils import dotdict
    hdr = open(os.path.join(REPO, 'include', 'relightableavatar.h')).read()
    assert 'ra_mesh_closest_backward' in _lib.SYMBOLS and re.search(r'^int\s+ra_mesh_closest_backward\s*\(', hdr, flags=re.M)
    assert len(_lib.SYMBOLS['ra_mesh_closest_backward'][1]) == 16
    assert re.search(r'#define\s+RA_ABI_VERSION\s+9\b', hdr) and _lib.ABI_VERSION == 9
    L = _lib.lib()
    assert L.ra_abi_version() == 9
    sig = inspect.signature(engine.Mesh.closest_backward)
    assert list(sig.parameters) == ['self', 'points', 'out', 'g_d2', 'g_attr', 'want'] and sig.parameters['want'].default == ('dpts', 'dverts', 'dattr')
    assert list(inspect.signature(engine.Mesh.__init__).parameters)[:4] == ['self', 'engine', 'handle', 'n_faces']
    assert list(inspect.signature(mesh_utils.point_mesh_distance).parameters) == ['points', 'verts', 'faces', 'engine']
    assert list(inspect.signature(mesh_utils.point_to_surface_loss).parameters) == ['verts', 'faces', 'points', 'squared', 'engine']
    assert list(inspect.signature(mesh_utils.chamfer_loss).parameters) == ['verts', 'faces', 'tgt_verts', 'tgt_faces', 'src_pts_bary', 'tgt_pts', 'engine']
    sig = inspect.signature(mesh_utils.point_cloud_fitting)
    assert list(sig.parameters) == ['src_verts', 'src_faces', 'tar_pts', 'param_lambda', 'opt_iter', 'chunk_size', 'lr', 'generator', 'engine']
    assert [sig.parameters[k].default for k in ('param_lambda', 'opt_iter', 'chunk_size', 'lr')] == [29, 100, None, 1e-3]
    for word in ('point_mesh_distance(points, verts, faces)', 'point_cloud_fitting(src_verts, src_faces, tar_pts', 'ra_mesh_closest_backward'):
        assert word in mesh_utils.__doc__, word
    assert 'never in the mesh.  With' not in mesh_utils.__doc__          # the old Autograd paragraph
    # the C entry with a null ctx: sizes first, then the arguments; nothing below reaches a device
    err = lambda: L.ra_last_error().decode()
    p = C.c_void_p(16)          # never dereferenced: every call below fails on its arguments
    call = lambda ctx, F, V, n, g, ga, Cn, dp, dv, da: L.ra_mesh_closest_backward(ctx, p, F, V, p, p, p, p, n, g, ga, Cn, dp, dv, da, None)
    for F, V, n, Cn in ((4, 3, -1, 0), (4, 3, 1 << 30, 0), (4, 0, 5, 0), (0, 3, 5, 0), ((1 << 24) + 1, 3, 5, 0), (4, 3, 5, -1), (4, 3, 5, 65)):
        assert call(None, F, V, n, p, p, Cn, p, p, p) != 0 and 'ra_mesh_closest_backward: bad sizes' in err(), (F, V, n, Cn)
    assert call(None, 4, 3, 5, p, p, 3, p, p, p) != 0 and 'ra_mesh_closest_backward: null argument' in err()            # no ctx
    # the refusals that need a ctx (no output, an output without its upstream gradient) are held on the device, with a real one
    # the Python layer refuses before it touches a context: this Mesh has none
    mesh = engine.Mesh.__new__(engine.Mesh)
    out = dotdict(closest=torch.zeros(5, 3), face=torch.zeros(5, dtype=torch.int32), bary=torch.zeros(5, 3))
    pts, g, ga = torch.zeros(5, 3), torch.zeros(5), torch.zeros(5, 3)
    for kwargs in (dict(want=()), dict(want=('dfaces',)), dict(g_d2=None, g_attr=ga), dict(g_d2=g, g_attr=None), dict(g_d2=g, want=('dpts', 'dattr')),
                   dict(g_d2=g[:4], want=('dpts',)), dict(g_d2=g, g_attr=torch.zeros(5, 65)), dict(g_d2=g, g_attr=torch.zeros(4, 3))):
        with pytest.raises(ValueError):
            mesh.closest_backward(pts, out, **kwargs)
    with pytest.raises(ValueError):
        mesh.closest_backward(pts, dotdict(closest=out.closest, face=out.face), g_d2=g, want=('dpts',))
    with pytest.raises(ValueError):
        mesh.closest_backward(torch.zeros(6, 3), out, g_d2=torch.zeros(6), want=('dpts',))
    with pytest.raises(ValueError):
        mesh_utils.point_mesh_distance(torch.zeros(1, 5, 3), torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64))

"""The mesh-fitting restatement (tests/fit_ref.py) against the reference's own outputs (tests/golden/icp.npz, made by
tests/golden/make_golden_icp.py) and against the plain definitions, on the CPU:

    1. the golden's inputs regenerate by seed, and its fixtures keep the margin the maker asserted;
    2. normals, areas and edge lengths: the float64 restatement reproduces the reference's float64 run, and the kernel-order
       restatement (float32 in and out) stays within 10 x the reference's own float32 error;
    3. the ICP residual from the exhaustive closest point: the kept mask equals the golden's exactly, loss and gradient under the
       same 10 x rule;
    4. M = I + lambda L from the neighbour lists against the dense definition, self-edges and isolated vertices included;
    5. the restated conjugate gradients against scipy's spsolve under the 10 x rule (float32 spsolve on the same system);
    6. AdamUniform against a literal transcription of its definition;
    7. the fitting loop's loss decreases and every row keeps its margin from both filters;
    8. tests/native/fit_rules_main.cpp: csrc/ra_fit_rules.hpp compiled for the host with sanitizers against the restatement.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import fit_ref as Ft
import mesh_distance_ref as R
import topology_ref as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden', 'icp.npz')
EPS32 = 2.0 ** -23
NORMAL_MESHES = ('octa', 'sphere66', 'patch5', 'fin', 'two', 'fan40', 'unref', 'repeat')
ICP_CASES = ('s66_on_258', 's258_on_66', 'patch_on_fin', 'none_kept')
SOLVE_MESHES = ('octa', 'unref', 'repeat', 'sphere66', 'sphere258', 'sphere1026', 'patch5', 'fin', 'two', 'fan40')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def rel(a, ref):
    """max |a - ref| / max |ref|"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)) if a.size else 0.0


def within_ten(err, ref_err):
    return err <= 10 * max(ref_err, EPS32)


def test_golden_inputs_regenerate(golden):
    assert tuple(golden['normal_meshes']) == NORMAL_MESHES and tuple(golden['icp_cases']) == ICP_CASES
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert float(golden['angle_th']) == float(np.cos(np.deg2rad(45.0)))
    for name, src, dst in (('s66_on_258', 'sphere66', 'sphere258'), ('s258_on_66', 'sphere258', 'sphere66'), ('patch_on_fin', 'patch5', 'fin'),
                           ('none_kept', 'sphere66', 'sphere258')):
        tv, tf = T.mesh(dst)
        assert np.array_equal(golden[f'{name}/verts'], tv) and np.array_equal(golden[f'{name}/faces'], tf), name
        assert golden[f'{name}/points'].shape == T.mesh(src)[0].shape and np.abs(golden[f'{name}/points'] - T.mesh(src)[0]).max() < 0.5, name
    # the margins the maker asserted, from the float64 definition
    for name in ICP_CASES:
        n1 = Ft.normals64(golden[f'{name}/verts'], golden[f'{name}/faces'], None)[0]
        dist_th = float(golden[f'{name}/dist_th'])
        _, _, keep, d2, dot = Ft.truth_icp(golden[f'{name}/points'], golden[f'{name}/point_normals'], golden[f'{name}/verts'], golden[f'{name}/faces'], n1,
                                           dist_th, float(golden['angle_th']))
        assert np.abs(d2 / dist_th ** 2 - 1).min() > 1e-4 and np.abs(dot / float(golden['angle_th']) - 1).min() > 1e-4, name
        assert np.array_equal(keep, golden[f'{name}/keep']), name


@pytest.mark.parametrize('name', NORMAL_MESHES)
def test_normals_against_the_reference(golden, name):
    v, f = T.mesh(name)
    t = T.topo(name)
    fn64, ar64, vn64 = Ft.normals64(v, f, t)
    assert rel(fn64, golden[f'{name}/face_normals64']) <= 1e-14 and rel(ar64, golden[f'{name}/face_areas64']) <= 1e-14
    assert np.array_equal(vn64, golden[f'{name}/vert_normals64'])
    assert rel(Ft.edge_length(v, t['edges']), golden[f'{name}/edge_length64']) <= 1e-14
    # kernel order, float32 in and out, against the float64 truth ON THE SAME float32 vertices
    v32 = v.astype(np.float32)
    fn, ar, vn = Ft.normals(v32, f, t)
    tn, ta, tvn = Ft.normals64(v32.astype(np.float64), f, t)
    g32n, g32a = golden[f'{name}/face_normals32'], golden[f'{name}/face_areas32']
    en, ea, evn = rel(fn, tn), rel(ar, ta), rel(vn, tvn)
    rn, ra = rel(g32n, tn), rel(g32a, ta)
    print(f'{name}: face normals {en:.3e} (reference float32 {rn:.3e}), areas {ea:.3e} ({ra:.3e}), vertex normals {evn:.3e}')
    assert fn.dtype == ar.dtype == vn.dtype == np.float32 and np.isfinite(fn).all() and np.isfinite(vn).all()
    assert within_ten(en, rn) and within_ten(ea, ra) and evn <= 10 * EPS32
    if name == 'unref':
        assert not vn[3].any() and not vn[7].any(), 'a vertex no face uses has the normal 0'
    if name == 'repeat':
        assert not fn[5].any() and ar[5] == 0, 'a face with a repeated index has no area and the normal 0 / 1e-8'


@pytest.mark.parametrize('name', ICP_CASES)
def test_icp_against_the_reference(golden, name):
    p, n0, tv, tf = (golden[f'{name}/{k}'] for k in ('points', 'point_normals', 'verts', 'faces'))
    dist_th, angle_th = float(golden[f'{name}/dist_th']), float(golden['angle_th'])
    p32, tv32 = p.astype(np.float32), tv.astype(np.float32)
    topo = T.halfedge_build(tf, len(tv))
    n1 = Ft.normals(tv32, tf, topo)[0]
    d2, closest, face, _ = R.closest_point(p32, tv32, tf, np.float32)
    sums, grad, keep = Ft.icp_residual(p32, n0.astype(np.float32), n1, d2, closest, face, dist_th, angle_th)
    assert np.array_equal(keep, golden[f'{name}/keep']), 'the kept mask equals the reference\'s, no row excused'
    g64, g32 = golden[f'{name}/grad64'], golden[f'{name}/grad32']
    if name == 'none_kept':
        assert sums[1] == 0 and not grad.any() and np.isnan(golden[f'{name}/loss64']) and np.isnan(golden[f'{name}/loss32']) and not g32.any()
        with np.errstate(all='ignore'):
            assert np.isnan(sums[0] / sums[1])
        return
    loss = sums[0] / sums[1]
    l64, l32 = float(golden[f'{name}/loss64']), float(golden[f'{name}/loss32'])
    el, rl, eg, rg = abs(loss - l64) / l64, abs(l32 - l64) / l64, rel(grad, g64), rel(g32, g64)
    print(f'{name}: kept {int(sums[1])} of {len(p)}; loss {el:.3e} (reference float32 {rl:.3e}); gradient {eg:.3e} ({rg:.3e})')
    assert within_ten(el, rl) and within_ten(eg, rg)


@pytest.mark.parametrize('name', SOLVE_MESHES)
def test_operator_against_the_dense_definition(name):
    v, f = T.mesh(name)
    V = len(v)
    A = np.zeros((V, V))
    for a, b, c in f:
        for i, j in ((a, b), (b, c), (c, a)):
            if i != j:
                A[i, j] = A[j, i] = 1
    lam = 19.0
    M = np.eye(V) + lam * (np.diag(A.sum(1)) - A)
    assert np.array_equal(Ft.truth_matrix(f, V, lam).toarray(), M)
    assert np.allclose(M, M.T) and np.linalg.eigvalsh(M).min() >= 1 - 1e-9, 'symmetric positive definite'
    x = np.random.default_rng(3).standard_normal((V, 3)).astype(np.float32)
    got = Ft.apply(x, T.topo(name), lam)
    want = M @ x.astype(np.float64)
    err = rel(got, want)
    print(f'{name}: V {V} M x {err:.3e}')
    assert err <= 4 * EPS32
    deg = A.sum(1)
    for k in np.flatnonzero(deg == 0):
        assert np.array_equal(got[k], x[k]), 'an isolated vertex has the row x = b'


@pytest.mark.parametrize('lam', (0, 9, 29))
@pytest.mark.parametrize('name', SOLVE_MESHES)
def test_restated_solve_against_spsolve(name, lam):
    v, f = T.mesh(name)
    b = Ft.apply(v.astype(np.float32), T.topo(name), lam)          # a smooth right-hand side, as the fitting has
    want = Ft.truth_solve(f, len(v), lam, b.astype(np.float64))
    f32 = Ft.truth_solve(f, len(v), lam, b, np.float32)
    x, iters, stop, res = Ft.solve(b, T.topo(name), lam)
    err, ref = rel(x, want), rel(f32, want)
    print(f'{name} lambda {lam}: iterations {iters.tolist()} residual {res.max():.3e}; error {err:.3e}, float32 spsolve {ref:.3e}')
    assert (stop == Ft.STOP_CONVERGED).all() and (res <= 1e-9).all() and iters.max() <= 128
    assert within_ten(err, ref)
    if lam == 0:
        assert (iters <= 1).all() and np.array_equal(x, b)
    # a channel alone gives the same bits
    alone = Ft.solve(b[:, 1], T.topo(name), lam)[0]
    assert np.array_equal(alone[:, 0].view(np.int32), x[:, 1].view(np.int32))


def test_solve_control_cases():
    name, lam = 'sphere66', 29
    t, (v, f) = T.topo(name), T.mesh(name)
    b = Ft.apply(v.astype(np.float32), t, lam)
    x, iters, stop, res = Ft.solve(b, t, lam)
    x0, i0, s0, _ = Ft.solve(b, t, lam, max_iter=0)
    assert not x0.any() and (i0 == 0).all() and (s0 == Ft.STOP_NONE).all()
    xs, i3, s3, r3 = Ft.solve(b, t, lam, max_iter=3)
    assert (i3 == 3).all() and (s3 == Ft.STOP_NONE).all() and (r3 > 1e-9).all(), 'too few iterations are reported'
    # float32 rounding of the solution leaves a residual of about cond x 2^-24: a warm start passes only a tolerance above that
    xw, iw, sw, rw = Ft.solve(b, t, lam, x0_32=x, tol=1e-3)
    print(f'warm start: residual {rw.max():.3e}')
    assert (iw == 0).all() and (sw == Ft.STOP_CONVERGED).all() and np.array_equal(xw.view(np.int32), x.view(np.int32))
    xz, iz, sz, _ = Ft.solve(np.zeros_like(b), t, lam, x0_32=x)
    assert not xz.any() and (sz == Ft.STOP_ZERO).all()
    bad = b.copy()
    bad[5, 1] = np.nan
    xn, _, sn, _ = Ft.solve(bad, t, lam)
    assert np.isnan(xn[:, 1]).all() and sn[1] == Ft.STOP_NAN and np.array_equal(xn[:, [0, 2]].view(np.int32), x[:, [0, 2]].view(np.int32))


def test_adam_uniform_against_the_definition():
    rng = np.random.default_rng(5)
    p = rng.standard_normal((40, 3)).astype(np.float32)
    q, g1, g2 = p.copy(), np.zeros_like(p), np.float32(0)
    lp, l1, l2 = p.astype(np.float64), np.zeros((40, 3)), 0.0
    b1, b2, lr = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(3e-2))
    for t in range(1, 4):
        g = (rng.standard_normal((40, 3)) * 10.0 ** -t).astype(np.float32)
        q, g1, g2 = Ft.adam_step(q, g, g1, g2, t, 3e-2)
        lp, l1, l2 = Ft.adam_literal(lp, g.astype(np.float64), l1, l2, t, lr, b1, b2)
        err = rel(q, lp)
        print(f'step {t}: {err:.3e}; g2 {g2:.6e} against {l2:.6e}')
        assert q.dtype == np.float32 and err <= 4 * EPS32 and abs(g2 - l2) <= 2 * EPS32 * l2
    assert g1.shape == p.shape and np.ndim(g2) == 0, 'ONE second-moment scalar per tensor'


@pytest.fixture(scope='module')
def fitted():
    v0, v1, f = Ft.fit_pair()
    out = {}
    for focus in (False, True):
        sel = Ft.boundary_rows(f, len(v0), 1) if focus else None
        margins = []
        out[focus] = Ft.fit(v0, f, v1, f, 29, Ft.FIT_ITERS, Ft.FIT_LR, sel, sel, margins=margins) + (margins, sel)
    return out


@pytest.mark.parametrize('focus', (False, True))
def test_fitting_loss_decreases_with_margin(fitted, focus):
    w0, w1, losses, margins, sel = fitted[focus]
    print(f'boundary_focus {focus}: rows {81 if sel is None else len(sel)}; loss {losses[0]:.4e} -> {losses[-1]:.4e}; smallest margin {min(margins):.3f}')
    assert len(losses) == 20 and losses[-1] < 0.5 * losses[0] and (np.diff(losses) < 0).all()
    assert min(margins) > 0.05, 'every row stays inside both filters, away from their thresholds, in every iteration'


def test_fit_rules_native(tmp_path):
    """tests/native/fit_rules_main.cpp: a stand-alone program (its own main) around csrc/ra_fit_rules.hpp, built with
    -fsanitize=address,undefined and run on the CPU against the restatement's values."""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    cases = tmp_path / 'cases.bin'
    i4, f4 = (lambda a: np.ascontiguousarray(a, dtype='<i4').tobytes()), (lambda a: np.ascontiguousarray(a, dtype='<f4').tobytes())
    rng = np.random.default_rng(9)
    with open(cases, 'wb') as fh:
        for name, C, lam in (('octa', 3, 9.0), ('repeat', 3, 29.0), ('unref', 1, 29.0), ('fan40', 4, 19.0), ('fin', 64, 9.0), ('sphere66', 3, 29.0)):
            t, (v, f) = T.topo(name), T.mesh(name)
            V, F = len(v), len(f)
            x = np.concatenate([v, rng.standard_normal((V, max(C - 3, 0)))], axis=1)[:, :C].astype(np.float32)
            v32 = v.astype(np.float32)
            fn, ar, vn = Ft.normals(v32, f, t)
            p = (v + rng.uniform(-0.05, 0.05, v.shape)).astype(np.float32)
            n0 = vn.copy()
            n0[::3] = -n0[::3]
            d2, closest, face, _ = R.closest_point(p, v32, f, np.float32)
            dist_th, angle_th = 0.05, float(np.cos(np.deg2rad(45.0)))
            sums, grad, keep = Ft.icp_residual(p, n0, fn, d2, closest, face, dist_th, angle_th)
            NA, steps = 3 * V, 3
            param = v32.reshape(-1).copy()
            grads = (rng.standard_normal((steps, NA)) * 0.01).astype(np.float32)
            q, g1, g2 = param.copy(), np.zeros(NA, dtype=np.float32), np.float32(0)
            for s in range(steps):
                q, g1, g2 = Ft.adam_step(q, grads[s], g1, g2, s + 1, 3e-2)
            fh.write(struct.pack('<7i6f', V, F, C, len(t['nbr']), V, NA, steps, lam, dist_th, angle_th, 3e-2, 0.9, 0.999))
            fh.write(i4(t['nbr_start']) + i4(t['nbr']) + i4(f) + i4(t['out_start']) + i4(t['out_he']))
            fh.write(f4(x) + f4(Ft.apply(x, t, lam)) + f4(v32) + f4(fn) + f4(ar) + f4(vn))
            fh.write(f4(p) + f4(closest) + f4(d2) + i4(face) + f4(n0) + f4(fn) + keep.astype(np.uint8).tobytes() + struct.pack('<d', sums[1]) + f4(grad))
            fh.write(f4(param) + f4(grads) + f4(q) + f4(g1) + struct.pack('<f', g2))
    exe = str(tmp_path / 'fit_rules_main')
    static = ['-static-libasan'] if os.path.basename(cxx).startswith('g++') else []          # gcc's spelling; clang links its runtime statically already
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + static +
                       ['-I', os.path.join(REPO, 'relightableavatar_amd', 'csrc'), os.path.join(REPO, 'tests', 'native', 'fit_rules_main.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and 'fit rules ok: 6 cases' in r.stdout, r.stdout + r.stderr


def test_python_layer_and_abi():
    import re
    from relightableavatar_amd import _lib, engine, largesteps, mesh_utils
    hdr = open(os.path.join(REPO, 'include', 'relightableavatar.h')).read()
    for sym in ('ra_topo_diffuse_apply', 'ra_topo_diffuse_solve', 'ra_mesh_normals', 'ra_icp_residual', 'ra_adam_uniform_step', 'ra_fit_tile'):
        assert sym in _lib.SYMBOLS and re.search(r'^int\s+' + sym + r'\s*\(', hdr, flags=re.M), sym
    L = _lib.lib()
    assert L.ra_abi_version() == 9
    assert L.ra_fit_tile(0) == Ft.TILE and L.ra_fit_tile(1) == Ft.TILE and L.ra_fit_tile(2) == 0
    for fn in ('face_normals', 'get_face_areas', 'get_edge_length', 'icp_loss', 'bidirectional_icp_fitting'):
        assert callable(getattr(mesh_utils, fn))
    for fn in ('compute_matrix', 'to_differential', 'from_differential', 'AdamUniform'):
        assert callable(getattr(largesteps, fn))
    for m in ('diffuse_apply', 'diffuse_solve', 'normals'):
        assert hasattr(engine.Topology, m)
    assert hasattr(engine.Mesh, 'icp_residual') and hasattr(engine.Engine, 'adam_uniform_step')
    with pytest.raises(ValueError, match='method'):
        largesteps.from_differential(None, None, 'LU')
    import torch
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 2, 0]])
    assert torch.allclose(mesh_utils.get_edge_length(v, torch.tensor([[0, 1], [1, 2]])), torch.tensor([1.0, 5 ** 0.5]))

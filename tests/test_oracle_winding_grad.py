"""The references of the winding-gradient tests, checked on the CPU.

    1. tests/winding_grad_ref.py's float64 oracle — the closed form — against the golden the reference's own float64 autograd wrote
       (tests/golden/winding_grad.npz), relative to max |g64| of the case.  The margins are what tests/golden/
       make_golden_winding_grad.py measures, with the measured figure beside each: at most 2.9e-9 on the grid sets (bound 1e-8) and
       at most 1.9e-4 on the near sets (bound 5e-4).  They are the REFERENCE's conditioning, not the oracle's: next to a face its
       L'Huilier product of half-angle tangents loses digits even in float64, which the half-angle form does not.  No row is left out:
       the golden is finite on every row.
    2. the float32 restatement of the kernel's operations: its value is winding_ref.winding_number_kernel32's bit for bit, and its
       gradient stays under the reference's own float32 autograd error (stored in the golden; 7e-3 to 6.3 x max |g| on the near sets);
    3. the rules both share: NaN rows, dropped faces, det == 0;
    4. tests/native/winding_grad_tri_main.cpp: the per-pair function of the kernel, compiled for the host with sanitizers;
    5. the python layer: the shift under autograd, no CPU fallback.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import winding_grad_ref as G
import winding_ref as W

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden', 'winding_grad.npz')
# measured by make_golden_winding_grad.py, |oracle - g64| / max |g64|: grid 2.877e-09 (hull, two, degenerate), 2.741e-09 (far), 1.0e-11
# (opened), 2.8e-11 (flipped), 5.2e-15 (single); near 1.872e-04 (far), 8.572e-05 (hull, two, degenerate), 1.6e-05 (opened), 1.2e-05
# (flipped), 4.6e-12 (single)
MARGIN = {'grid': 1e-8, 'near': 5e-4}
STRIDE = {'near': 1, 'grid': 5}


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def points(name, group):
    return W.point_sets(name)[group][::STRIDE[group]]


def test_golden_inputs_regenerate(golden):
    assert tuple(golden['meshes']) == W.MESHES and tuple(golden['sets']) == W.SETS and tuple(golden['stride']) == tuple(STRIDE[s] for s in W.SETS)
    for name in W.MESHES:
        for group in W.SETS:
            assert np.array_equal(golden[f'{name}/{group}/checksum'], W.checksum(name, group)), (name, group)
            assert golden[f'{name}/{group}/g64'].shape == golden[f'{name}/{group}/g32'].shape == (len(points(name, group)), 3)
            # the reference's autograd is finite on every row, in either precision: nothing is left out below
            assert tuple(golden[f'{name}/{group}/nonfinite']) == (0, 0), (name, group)
            assert np.isfinite(golden[f'{name}/{group}/g64']).all()
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(REPO, 'tests', 'golden', 'winding.npz'))


@pytest.mark.parametrize('name', W.MESHES)
def test_oracle_matches_the_references_float64_autograd(golden, name):
    v, f = W.mesh_case(name)
    for group in W.SETS:
        g64 = golden[f'{name}/{group}/g64']
        w, g = G.winding_grad(points(name, group), v, f)
        e = np.abs(g - g64).max() / np.abs(g64).max()
        # the value: where a point lies in a face's plane the reference's sign is rounding noise and brings 2 * 4 sqrt(eps) / (4 pi) =
        # 6.4e-6 per such pair with it (test_oracle_winding.py, item 1), where the oracle has det == 0 and adds 0: printed, not held
        ew = np.abs(w - W.winding_number(points(name, group), v, f)).max()
        print(f'{name}/{group}: max |oracle - g64| / max |g64| {e:.3e} ({MARGIN[group]:.0e}), {len(g)} rows, none left out; its value against winding_ref float64 {ew:.3e}')
        assert e <= MARGIN[group], (name, group)


@pytest.mark.parametrize('name', W.MESHES)
def test_float32_restatement(golden, name):
    v, f = W.mesh_case(name)
    for group in W.SETS:
        p = points(name, group)
        g64 = G.winding_grad(p, v, f)[1]
        w32, g32 = G.winding_grad_kernel32(p, v, f)
        scale = np.abs(g64).max()
        e, own = np.abs(g32 - g64) / scale, np.abs(golden[f'{name}/{group}/g32'] - g64) / scale
        print(f'{name}/{group}: restatement max {e.max():.3e} median {np.median(e):.3e} of max |g|; the reference in float32 max {own.max():.3e} median {np.median(own):.3e}')
        assert w32.dtype == g32.dtype == np.float32 and np.isfinite(g32).all()
        assert np.array_equal(w32.view(np.int32), W.winding_number_kernel32(p, v, f).view(np.int32)), (name, group)
        assert e.max() <= own.max(), (name, group)


def test_nan_rules_of_the_references():
    v, f = W.hull()
    gv, gf, mid = G.edge_gadget()
    v2, f2 = np.concatenate([v, gv]), np.concatenate([f, gf + len(v)])
    p = np.float32([[0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], v[5], mid, [0.1, 0.1, 0.1]])
    for fn in (G.winding_grad, G.winding_grad_kernel32):
        w, g = fn(p, v2, f2)
        alone = fn(p[[0, 5]], v2, f2)
        assert np.isnan(g[1:5]).all() and np.isnan(w[1:4]).all() and np.isfinite(g[[0, 5]]).all() and np.isfinite(w[[0, 4, 5]]).all(), (w, g)
        assert np.array_equal(g[[0, 5]], alone[1]) and np.array_equal(w[[0, 5]], alone[0])
    bad = v.copy()
    bad[int(f[3, 0])] = np.nan                               # every face at that vertex is dropped
    keep = ~(f == f[3, 0]).any(1)
    for fn in (G.winding_grad, G.winding_grad_kernel32):
        a, b = fn(p[[0, 5]], bad, f), fn(p[[0, 5]], v, f[keep])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_flat_pairs_contribute_zero():
    """det == 0: a point in a face's plane, a face of three equal vertices"""
    a, b, c = np.float32([0, 0, 0]), np.float32([0.7, 0, 0]), np.float32([0, 0.7, 0])
    p = np.float32([[0.9, 0.9, 0.0], [-0.2, 0.1, 0.0]])
    q = np.float32([0.3, 0.2, 0.1])
    for pair, dt in ((G.solid_angle_grad64, np.float64), (G.solid_angle_grad32, np.float32)):
        w, g = pair(p.astype(dt), a.astype(dt), b.astype(dt), c.astype(dt))
        assert (w == 0).all() and (g == 0).all(), (w, g)
        w, g = pair(q.astype(dt), a.astype(dt), a.astype(dt), a.astype(dt))
        assert w == 0 and (g == 0).all()
    # one triangle, 1 mm off its centroid on either side: w(x, y, -z) = -w(x, y, z), so the normal component of the gradient is the same
    # on both sides — positive: away from the face |w| falls from 1 / 2, above it from -1 / 2 — and the tangential ones are opposite
    v, f = np.stack([a, b, c]), np.array([[0, 1, 2]])
    cen = v.mean(0, dtype=np.float64)
    for fn in (G.winding_grad, G.winding_grad_kernel32):
        w, g = fn(np.stack([cen + [0, 0, 1e-3], cen - [0, 0, 1e-3]]), v, f)
        print(f'{fn.__name__}: w {w}, g {g}')
        assert w[0] < 0 < w[1] and (g[:, 2] > 0).all() and (np.abs(g[:, :2]) < 1e-2 * np.abs(g[:, 2:])).all()
        assert abs(g[0, 2] - g[1, 2]) < 1e-4 * np.abs(g).max() and np.abs(g[0, :2] + g[1, :2]).max() < 1e-4 * np.abs(g).max()


def test_compositions():
    """distance_grad is the unit vector from the closest point; the winding term of winding_distance_grad is 0 in the snapped zone"""
    v, f = W.mesh_case('opened')
    p = W.point_sets('opened')['grid'][::97]
    d, gd = G.distance_grad(p, v, f)
    assert np.abs(np.linalg.norm(gd[d > 0], axis=1) - 1).max() < 1e-12
    wg = G.winding_grad(p, v, f)
    for th in W.THRESHOLDS:
        val, grad, term = G.winding_distance_grad(p, v, f, th, wg=wg, dg=(d, gd))
        state = W.shift_state(wg[0], 0.5, th)
        assert (term[state != 0] == 0).all() and (state == 0).any() and (state != 0).any()
        assert np.array_equal(val, W.winding_shift(wg[0], 0.5, th) * d)
        free = state == 0
        assert np.allclose(grad[free], (2 * d[free])[:, None] * wg[1][free] + ((wg[0][free] - 0.5) * 2)[:, None] * gd[free], rtol=0, atol=1e-15)


def test_winding_grad_arithmetic_native(tmp_path):
    """tests/native/winding_grad_tri_main.cpp: a stand-alone program (its own main) around csrc/ra_winding_grad_tri.hpp — the per-pair
    function the gradient kernels inline, in the same IEEE fp32 operations — built with -fsanitize=address,undefined and run on the
    CPU: 144 000 seeded pairs; the value's bits against winding_tri, the NaN and det == 0 rules, a long-double evaluation of the
    closed form."""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'winding_grad_tri_main')
    static = ['-static-libasan'] if os.path.basename(cxx).startswith('g++') else []          # gcc's spelling; clang links its runtime statically already
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + static +
                       ['-I', os.path.join(REPO, 'relightableavatar_amd', 'csrc'), os.path.join(REPO, 'tests', 'native', 'winding_grad_tri_main.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and 'winding gradient arithmetic ok' in r.stdout, r.stdout + r.stderr


def test_python_layer():
    from relightableavatar_amd import mesh_utils
    from relightableavatar_amd.evaluators import mesh_evaluator
    v, f = W.hull()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    assert mesh_evaluator.Evaluator.engine is None
    p = torch.zeros(4, 3, requires_grad=True)
    for call in (lambda: mesh_utils.winding_number(p, tv, tf), lambda: mesh_utils.bvh_distance(p, tv, tf), lambda: mesh_utils.winding_distance(p, tv, tf),
                 lambda: mesh_utils.isosurface_fitting(tv, tf, tv, tf, opt_iter=1)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    # the shift's in-place lines under autograd: slope 2 where it is neither clipped nor snapped, exactly 0 elsewhere; the values are the same
    w = torch.tensor([0.0, 0.2249, 0.2251, 0.5, 0.7749, 0.7751, 1.0, 1.3], requires_grad=True)
    s = mesh_utils.winding_shift(w, 0.5, 0.45)
    s.sum().backward()
    assert torch.equal(w.grad, torch.tensor([0.0, 0.0, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0]))
    assert torch.equal(s.detach(), mesh_utils.winding_shift(w.detach(), 0.5, 0.45))
    assert np.array_equal(G.shift_slope(w.detach().numpy().astype(np.float64), 0.5, 0.45), w.grad.numpy())
    header = open(os.path.join(REPO, 'include', 'relightableavatar.h')).read()
    assert 'ra_mesh_winding_grad' in header and 'RA_ABI_VERSION 9' in header.replace('  ', ' ')

"""The references of the ray-casting tests, checked on the CPU.

    1. tests/raycast_ref.py's inputs regenerate by seed (the golden's checksums);
    2. its float64 restatement of the reference's moller_trumbore matches what the reference itself wrote (tests/golden/raycast.npz) to
       rounding, and its float32 restatement stays within the 10 x rule of the reference's own float32 result;
    3. the float32 restatement of the KERNEL's operations is held to the reference's own float32 error on u, v, t: the 10 x rule on
       maximum and median of every golden pair set, the ceiling "no worse than the reference in float32" on the MEDIAN of all pairs
       (ratios 0.91 .. 0.98: fused multiply-adds replace some of the reference's roundings) and on the MAXIMUM over the pairs near
       their face (float64 |u|, |v| <= 2, every accepted pair among them), with one float32 ulp of the largest value there as the
       allowance for the final rounding (raycast_ref.check_pairs).  The maximum over ALL pairs sits on one ray parallel to a face to
       rounding, |u| about 2e4, where the error is a rounding of det times 1 / det^2 in either arithmetic (measured ratios 0.28 on
       hull, 1.74 on far): that pair is held to the 10 x rule;
    4. exhaustive nearest hit and count against analytic cases, a cube and a single triangle, in all three vertex orders;
    5. the classification: the reference's own float32 predicate agrees with float64 on every decided pair, at most 2 % of the rays of
       the non-degenerate sets are undecided, and the kernel's restatement (guard and slab clause included) returns the float64 face and
       count on every decided ray;
    6. tests/native/raycast_tri_main.cpp: the per-pair header compiled for the host with sanitizers, the lemma asserted pair by pair.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import raycast_ref as R
from frame_stage_ref import parity

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden', 'raycast.npz')
F32 = np.float32


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def test_golden_inputs_regenerate(golden):
    assert tuple(golden['meshes']) == R.MESHES and tuple(golden['sets']) == R.SETS + (R.GRAZE,) and tuple(golden['golden_meshes']) == R.GOLDEN_MESHES
    for name in R.MESHES:
        for group in R.SETS + (R.GRAZE,):
            assert np.array_equal(golden[f'{name}/{group}/checksum'], R.checksum(name, group)), (name, group)
            o, d = R.ray_sets(name)[group]
            assert o.shape == d.shape == (R.SIZES[group], 3) and o.dtype == d.dtype == F32 and np.isfinite(o).all() and np.isfinite(d).all()
    o, d = R.ray_sets('hull')[R.GRAZE]
    assert (d == 0).all(1).sum() == 26                                   # the rays with d = 0
    o, d = R.ray_sets('hull')['km']
    assert (np.linalg.norm(o, axis=-1) > 900).all()                      # 1 km away
    lens = np.linalg.norm(R.ray_sets('hull')['outside'][1], axis=-1)
    assert lens.min() < 0.5 and lens.max() > 5                           # d is not normalised


@pytest.mark.parametrize('name', R.GOLDEN_MESHES)
def test_restatements_reproduce_the_golden(golden, name):
    o, d, tris = R.golden_pairs(name)
    r64 = R.moller_trumbore(o, d, tris, np.float64)
    r32 = R.moller_trumbore(o, d, tris, F32)
    for i, k in enumerate('uvt'):
        g64, g32 = golden[f'{name}/{k}64'], golden[f'{name}/{k}32']
        assert g64.shape == (84, len(tris)) and g64.dtype == np.float64 and g32.dtype == F32
        e = (np.abs(r64[i] - g64) / np.maximum(1, np.abs(g64))).max()
        print(f'{name}/{k}: max |float64 restatement - golden float64| {e:.3e} relative (1e-9); float32 restatement bit-equal on {(r32[i] == g32).mean():.3f} of the pairs')
        assert e <= 1e-9, (name, k)
        parity(f'{name}/{k} float32 restatement', r32[i], g32, g64)
        parity(f'{name}/{k} float32 restatement, per element', r32[i], g32, g64, relative=True)


@pytest.mark.parametrize('name', R.GOLDEN_MESHES)
def test_kernel_restatement_under_the_references_own_error(golden, name):
    o, d, tris = R.golden_pairs(name)
    k32 = R.kernel32(o, d, tris)
    near = R.near_pairs(golden[f'{name}/u64'], golden[f'{name}/v64'])
    assert R.accept_ref(*(golden[f'{name}/{k}64'] for k in 'uvt'))[~near].sum() == 0
    for i, k in enumerate('uvt'):
        g64, g32 = golden[f'{name}/{k}64'], golden[f'{name}/{k}32']
        R.check_pairs(f'{name}/{k} kernel restatement', k32[i], g32, g64, near)


def rotations(tris):
    return [tris[:, [k, (k + 1) % 3, (k + 2) % 3]] for k in range(3)]


def cube():
    """the unit cube [0, 1]^3 as 12 triangles; each face split along the diagonal from its lowest to its highest corner"""
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=F32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])
    return v[f]


def both(o, d, tris):
    """exhaustive nearest / count: float64 on the reference's predicate, float32 on the kernel's"""
    u, v, t, _ = R.moller_trumbore(o, d, tris, np.float64)
    truth = R.nearest_count(R.accept_ref(u, v, t), u, v, t)
    uk, vk, tk, dk = R.kernel32(o, d, tris)
    return truth, R.nearest_count(R.accept_kernel32(o, d, tris, uk, vk, tk, dk), uk, vk, tk)


def test_cube_and_triangle_analytic():
    o = F32([[0.3, 0.4, -2.0], [0.3, 0.4, 0.5], [0.3, 0.4, 3.0], [2.0, 0.4, 0.7], [0.3, 0.4, -2.0], [5.0, 5.0, 5.0], [0.3, 0.4, -2.0]])
    d = F32([[0, 0, 1], [0, 0, 2], [0, 0, -0.5], [-1, 0, 0], [0, 0, -1], [1, 0, 0], [0, 0, 0]])
    want_t, want_n = [2.0, 0.25, 4.0, 1.0, np.inf, np.inf, np.inf], [2, 1, 2, 2, 0, 0, 0]
    for tris in rotations(cube()):
        truth, kern = both(o, d, tris)
        for tag, (t, face, uv, count) in (('float64', truth), ('kernel restatement', kern)):
            if tag == 'float64':                     # the reference "hits" with d = 0: invdet = -1e8 and u = v = -0
                t, face, count = t[:6], face[:6], count[:6]
            n = len(t)
            assert np.allclose(t, want_t[:n], rtol=1e-6) and list(count) == want_n[:n], (tag, t, count)
            assert ((face >= 0) == np.isfinite(want_t[:n])).all()
            for i in range(n):                       # the face answered holds the hit point
                if face[i] >= 0:
                    p = o[i] + t[i] * d[i].astype(np.float64)
                    a, b, c = tris[face[i]].astype(np.float64)
                    assert np.allclose((1 - uv[i, 0] - uv[i, 1]) * a + uv[i, 0] * b + uv[i, 1] * c, p, atol=1e-5), (tag, i)
    # one triangle: inside, outside past each edge, behind, parallel above it, in its plane
    tri = F32([[[0, 0, 0], [0.7, 0, 0], [0, 0.7, 0]]])
    o = F32([[0.2, 0.2, 1], [0.6, 0.6, 1], [-0.1, 0.2, 1], [0.2, -0.1, 1], [0.2, 0.2, 1], [0.2, 0.2, -1], [-1, 0.2, 0.5], [-1, 0.2, 0]])
    d = F32([[0, 0, -2], [0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, 1], [0, 0, -1], [1, 0, 0], [1, 0, 0]])
    for k, tris in enumerate(rotations(tri)):
        truth, kern = both(o, d, tris)
        for tag, (t, face, uv, count) in (('float64', truth), ('kernel restatement', kern)):
            if tag == 'kernel restatement':
                assert list(count) == [1, 0, 0, 0, 0, 0, 0, 0] and list(face) == [0, -1, -1, -1, -1, -1, -1, -1], (tag, k, count, face)
            else:                                    # the last ray lies in the plane: the reference's answer there is its eps
                assert list(count[:7]) == [1, 0, 0, 0, 0, 0, 0], (tag, k, count)
            assert abs(t[0] - 0.5) < 1e-6 and np.isnan(uv[1]).all()
            bary = {0: (0.2 / 0.7, 0.2 / 0.7), 1: (0.2 / 0.7, 1 - 0.4 / 0.7), 2: (1 - 0.4 / 0.7, 0.2 / 0.7)}[k]      # of b and c in this order
            assert np.allclose(uv[0], bary, atol=1e-6), (tag, k, uv[0], bary)


def test_ties_take_the_lowest_face_and_duplicates_count_twice():
    tri = F32([[[0, 0, 0], [0.7, 0, 0], [0, 0.7, 0]]])
    tris = np.concatenate([tri, tri, tri + F32([0, 0, 0.5])])
    o, d = F32([[0.2, 0.2, 1]]), F32([[0, 0, -1]])
    for res in both(o, d, tris):
        assert res[1][0] == 2 and res[3][0] == 3 and abs(res[0][0] - 0.5) < 1e-6
    for res in both(o, -d, tris):
        assert res[1][0] == -1 and res[3][0] == 0
    for res in both(F32([[0.2, 0.2, 0.25]]), d, tris):
        assert res[1][0] == 0 and res[3][0] == 2 and abs(res[0][0] - 0.25) < 1e-6


def test_classification_margin_and_undecided_share():
    """the reference alone, and the kernel's restatement, against float64 on the decided pairs and rays; the cap on the undecided"""
    total = undecided = 0
    for name in R.MESHES:
        for group in R.SETS + (R.GRAZE,):
            e = R.evaluate(name, group)
            pd, dec = e['pair_decided'], e['decided']
            flips32, flipsk = int(((e['acc32'] != e['acc64']) & pd).sum()), int(((e['acck'] != e['acc64']) & pd).sum())
            print(f"{name}/{group}: fp32 error on well-conditioned hits {e['measured']:.3e}, margin {e['margin']:.3e}; {int((~dec).sum())} of {len(dec)} rays undecided; "
                  f"on decided pairs the reference in float32 flips {flips32}, the kernel's predicate {flipsk}; hits float64 {int(e['acc64'].sum())} kernel {int(e['acck'].sum())}")
            assert 2.0 ** -24 <= e['measured'] and e['margin'] == 10 * e['measured']
            assert flips32 == 0 and flipsk == 0, (name, group)
            truth, rest = e['truth'], e['restated']
            assert np.array_equal(truth[1][dec], rest[1][dec]) and np.array_equal(truth[3][dec], rest[3][dec]), (name, group)
            assert np.isfinite(rest[0][rest[1] >= 0]).all() and np.isfinite(rest[2][rest[1] >= 0]).all()
            if group in R.SETS and name != 'degenerate':         # 'degenerate' holds a face with N = 0: no ray is decided there, by the definition
                total += len(dec)
                undecided += int((~dec).sum())
            if name == 'degenerate':
                assert not dec.any()
    print(f'undecided: {undecided} of {total} rays of the non-degenerate sets ({undecided / total:.4f}; cap {R.UNDECIDED_CAP})')
    assert undecided <= R.UNDECIDED_CAP * total
    # the sets do what their names say
    for name in ('hull', 'far', 'flipped'):
        assert (R.evaluate(name, 'outside')['truth'][3] == 2).mean() > 0.95 and (R.evaluate(name, 'inside')['truth'][3] == 1).mean() > 0.95
        assert (R.evaluate(name, 'miss')['truth'][3] == 0).all() and (R.evaluate(name, 'km')['truth'][3] == 2).all()
    # the guard: rays with d = 0 "hit" in the reference and never in the kernel's predicate
    e = R.evaluate('hull', R.GRAZE)
    zero = (e['d'] == 0).all(1)
    assert e['truth'][3][zero].min() > 0 and (e['restated'][3][zero] == 0).all()


def test_raycast_arithmetic_native(tmp_path):
    """tests/native/raycast_tri_main.cpp: a stand-alone program (its own main) around csrc/ra_raycast_tri.hpp — the per-pair function,
    predicate and slab test the kernel inlines, in the same IEEE fp32 operations — built with -fsanitize=address,undefined and run on
    the CPU: 460 800 seeded pairs; the lemma for every accepted pair, no clean hit lost to the guard or the slab clause."""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'raycast_tri_main')
    static = ['-static-libasan'] if os.path.basename(cxx).startswith('g++') else []          # gcc's spelling; clang links its runtime statically already
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + static +
                       ['-I', os.path.join(REPO, 'relightableavatar_amd', 'csrc'), os.path.join(REPO, 'tests', 'native', 'raycast_tri_main.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and 'raycast arithmetic ok' in r.stdout, r.stdout + r.stderr


def test_python_layer_has_no_cpu_fallback_and_refuses_batches():
    import torch
    from relightableavatar_amd import _lib, mesh_utils
    from relightableavatar_amd.evaluators import mesh_evaluator
    v, f = R.mesh_case('hull')
    tv, tf, p = torch.from_numpy(v), torch.from_numpy(f), torch.zeros(4, 3)
    assert mesh_evaluator.Evaluator.engine is None
    for call in (lambda: mesh_utils.ray_stabbing(p, tv, tf), lambda: mesh_utils.moller_trumbore(p, p, tv[tf]),
                 lambda: mesh_utils.raycast_maps(p, p, tv, tf)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    with pytest.raises(NotImplementedError):
        mesh_utils.moller_trumbore(torch.zeros(2, 4, 3), torch.zeros(2, 4, 3), torch.zeros(2, 5, 3, 3))
    with pytest.raises(ValueError):
        mesh_utils.moller_trumbore(p, p[:2], tv[tf])
    with pytest.raises(ValueError):
        mesh_utils.ray_stabbing(p[None], tv[None], tf[None])
    L = _lib.lib()
    assert L.ra_raycast_tile(0) == 64 and L.ra_raycast_tile(1) == 256 and L.ra_raycast_tile(2) == L.ra_mesh_tile(2) and L.ra_raycast_tile(3) == 0
    assert (_lib.RA_RAYCAST_BRUTE, _lib.RA_RAYCAST_UNSORTED) == (1, 2)
    hdr = open(os.path.join(REPO, 'include', 'relightableavatar.h')).read()
    assert all(s in hdr for s in ('ra_mesh_raycast', 'ra_ray_tri_pairs', 'ra_raycast_tile', 'RA_RAYCAST_BRUTE = 1', 'RA_RAYCAST_UNSORTED = 2'))

"""CPU tests of the cloth energies (no GPU):

    1. tests/golden/physx.npz regenerates its inputs by seed, holds finite outputs and positive rest areas, and records the reference's
       two quirks: the det + 2^-23 of Dm_inv (a rest-state stretch energy above 0) and get_vertex_mass's non-accumulating `+=`.
    2. tests/physx_ref.py, the float64 numpy restatement with analytic gradients, against the reference's float64 run at 1e-10 relative,
       and against central finite differences.
    3. The material coefficients of the Python layer and of the library (ra_cloth_material_derive, host only) against the golden's.
    4. tests/native/cloth_rules_main.cpp: csrc/ra_cloth_rules.hpp compiled for the host, plain and with sanitizers; its float
       evaluation — the kernels' arithmetic — is held to the golden under the project's 10 x float32 rule.
    5. The Python layer's names, the ABI additions and the XPBD stubs.

The Garment arrays and get_vertex_mass need the device (there is no CPU fallback): tests/test_gpu_physx.py holds them.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import physx_ref as P
import topology_ref as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden', 'physx.npz')
EPS32 = 2.0 ** -23
CASES = P.FIXTURE_MESHES + ('patch5_shared',)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def rel(a, ref):
    """max |a - ref| / max |ref|"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)) if a.size else 0.0


def bound(golden, key):
    """the project's 10 x float32 rule: 10 x the error of the reference's own float32 run against its float64 run, floored at eps"""
    return 10 * max(rel(golden[key + '32'], golden[key + '64']), EPS32)


def case_garment(golden, name):
    return P.garment(golden[f'{name}/v'], golden[f'{name}/f'], golden[f'{name}/vm'], golden[f'{name}/fm'])


def test_golden_inputs_regenerate(golden):
    assert tuple(golden['cases']) == CASES
    seen_B = set()
    for i, name in enumerate(CASES):
        mesh = 'patch5' if name == 'patch5_shared' else name
        v, f = T.mesh(mesh)
        assert np.array_equal(golden[f'{name}/v'], v) and np.array_equal(golden[f'{name}/f'], f)
        if name != 'patch5_shared':
            vm, fm = P.flatten_faces(v, f)
            assert np.array_equal(golden[f'{name}/vm'], vm) and np.array_equal(golden[f'{name}/fm'], fm)
            assert np.array_equal(golden[f'{name}/x'], P.perturbed(v, 100 + i, 1 + i % 3))
        else:
            assert np.array_equal(golden[f'{name}/vm'], v[:, :2]) and np.array_equal(golden[f'{name}/fm'], f)
        seen_B.add(golden[f'{name}/x'].shape[0])
        assert golden[f'{name}/f_area64'].min() > 0
        for k in golden.files:
            if k.startswith(name + '/') and golden[k].dtype.kind == 'f' and 'inv_mass' not in k:
                assert np.isfinite(golden[k]).all(), k
    assert seen_B == {1, 2, 3}
    assert len(golden['fin/f_connectivity']) == 39 and len(golden['patch5/f_connectivity']) == 40      # the edge of three faces makes no hinge
    assert np.isinf(golden['unref/inv_mass64']).sum() == 2 and (golden['unref/v_mass64'] == 0).sum() == 2


def test_recorded_quirks(golden):
    for name in P.FIXTURE_MESHES:
        assert 0 < float(golden[f'{name}/rest_stretch64']) < 1e-7, name        # det + eps at work: not exactly 0
    # the reference's vertex mass keeps ONE share per corner slot; the file's v_mass is the sum
    for name in CASES:
        ref, summed = golden[f'{name}/v_mass_reference64'], golden[f'{name}/v_mass64']
        assert (ref <= summed * (1 + 1e-12)).all()
        f, share = golden[f'{name}/f'], 426 * 0.00047 * golden[f'{name}/f_area64'] / 3
        last = np.zeros_like(ref)
        for k in range(3):
            slot = np.zeros_like(ref)
            slot[f[:, k]] = share                     # the last write wins, as in the reference
            last += slot
        assert rel(last, ref) < 1e-12, name
    assert (golden['sphere66/v_mass_reference64'] < 0.7 * golden['sphere66/v_mass64']).any()


@pytest.mark.parametrize('name', CASES)
def test_restatement_against_the_reference(golden, name):
    g, x = case_garment(golden, name), golden[f'{name}/x']
    B = len(x)
    for k in ('f_area', 'v_mass', 'Dm', 'Dm_inv'):
        assert rel(g[k], golden[f'{name}/{k}64']) < 1e-10, k
    assert np.array_equal(np.isinf(g['inv_mass']), np.isinf(golden[f'{name}/inv_mass64']))
    # the reference orders a pair by an unstable argsort: compare as sets of sorted pairs
    pairs = lambda a: sorted(tuple(sorted(r)) for r in np.asarray(a).tolist())
    assert pairs(g['f_connectivity']) == pairs(golden[f'{name}/f_connectivity'])
    assert pairs(g['f_connectivity_edges']) == pairs(golden[f'{name}/f_connectivity_edges'])
    es, gs = P.stretch(x, g)
    eb, gb = P.bending(x, g)
    eg, _ = P.gravity(x, g['v_mass'], float(golden['g']))
    assert abs(es.sum() / B - golden[f'{name}/stretch64']) <= 1e-10 * abs(golden[f'{name}/stretch64'])
    assert abs(eb.sum() / B - golden[f'{name}/bending64']) <= 1e-10 * abs(golden[f'{name}/bending64'])
    assert abs(eg.sum() / B - golden[f'{name}/gravity64']) <= 1e-10 * abs(golden[f'{name}/gravity64'])
    assert rel(gs / B, golden[f'{name}/stretch_grad64']) < 1e-10
    assert rel(gb / B, golden[f'{name}/bending_grad64']) < 1e-10
    # the rest value is what the strain's cancellation leaves of 2^-23 / det, squared: 1e-6 of it is 1e-13 of the strain's terms
    assert abs(P.stretch(golden[f'{name}/v'][None], g)[0][0] - golden[f'{name}/rest_stretch64']) <= 1e-6 * golden[f'{name}/rest_stretch64']


@pytest.mark.parametrize('name', ('sphere66', 'fin', 'unref'))
def test_restatement_against_finite_differences(golden, name):
    g, x = case_garment(golden, name), golden[f'{name}/x']
    for fun in (P.stretch, P.bending):
        idx, fd = P.finite_difference(lambda y: fun(y, g), x)
        grad = fun(x, g)[1]
        got = np.asarray([grad[i] for i in idx])
        assert np.abs(got - fd).max() <= 1e-6 * np.abs(grad).max(), fun.__name__


@pytest.mark.parametrize('name', ('sphere66', 'unref'))
def test_inertia_restatement(golden, name):
    seq, dt, mass = golden[f'{name}/seq'], float(golden['delta_t']), golden[f'{name}/v_mass64']
    xn, xc, vc = seq[:, 2], seq[:, 1], (seq[:, 1] - seq[:, 0]) / dt
    for term, accel in (('inertia', None), ('dynamic', [0, -9.81, 0])):
        val, gn, gc, gv = P.inertia(xn, xc, vc, mass, dt, accel)
        assert abs(val.sum() / 2 - golden[f'{name}/{term}64']) <= 1e-10 * golden[f'{name}/{term}64']
        for got, key in ((gn, 'g_next'), (gc, 'g_curr'), (gv, 'g_vel')):
            assert rel(got / 2, golden[f'{name}/{term}_{key}64']) < 1e-10
    a, b, c = P.sequence_parts(seq[:1], dt)
    val = P.inertia(a, b, c, mass, dt)[0]
    assert abs(val.sum() / len(a) - golden[f'{name}/sequence64']) <= 1e-10 * golden[f'{name}/sequence64']


def test_material_coefficients(golden):
    import ctypes as C
    from relightableavatar_amd import _lib, physx_utils
    m = physx_utils.StVKMaterial()
    want = golden['material']
    got = np.asarray([m.A, m.stretch_coeff, m.bending_coeff, m.lame_mu, m.lame_lambda])
    assert np.array_equal(got, want)
    r = P.material()
    assert rel([r['A'], r['stretch_coeff'], r['bending_coeff'], r['lame_mu'], r['lame_lambda']], want) < 1e-15
    for mults in ((50.0, 1.0, 1.0), (5.0, 2.0, 0.5)):
        cm = _lib.ra_cloth_material(*[d for _, d in _lib.CLOTH_MATERIAL_DEFAULTS])
        cm.bending_multiplier, cm.stretch_multiplier, cm.material_multiplier = mults
        out = (C.c_double * 5)()
        assert _lib.lib().ra_cloth_material_derive(C.byref(cm), out) == 0
        p = physx_utils.StVKMaterial(bending_multiplier=mults[0], stretch_multiplier=mults[1], material_multiplier=mults[2])
        assert rel(list(out), [p.A, p.stretch_coeff, p.bending_coeff, p.lame_mu, p.lame_lambda]) < 1e-15
    assert _lib.lib().ra_cloth_material_derive(None, None) != 0


def _native_cases(golden, path):
    i4, f4 = (lambda a: np.ascontiguousarray(a, dtype='<i4').tobytes()), (lambda a: np.ascontiguousarray(a, dtype='<f4').tobytes())
    mat = P.material()
    shapes = []
    with open(path, 'wb') as fh:
        for name in CASES:
            g, x = case_garment(golden, name), golden[f'{name}/x']
            f, ef, ev = g['f'], g['f_connectivity'], g['f_connectivity_edges']
            k0 = np.asarray([list(f[a]).index(v) for a, v in zip(ef[:, 0], ev[:, 0])], dtype=np.int64)
            k1 = np.asarray([list(f[a]).index(v) for a, v in zip(ef[:, 1], ev[:, 1])], dtype=np.int64)
            hinge = np.stack([ef[:, 0], ef[:, 1], k0, k1], axis=1)
            B, V = x.shape[:2]
            tol = [bound(golden, f'{name}/stretch'), bound(golden, f'{name}/bending'), bound(golden, f'{name}/stretch_grad'), bound(golden, f'{name}/bending_grad')]
            fh.write(struct.pack('<4i4f4d', V, len(f), len(ef), B, mat['thickness'], mat['lame_mu'], mat['lame_lambda'], mat['bending_coeff'], *tol))
            # Dm_inv and the areas as the float32 reference holds them
            fh.write(i4(f) + i4(hinge) + f4(golden[f'{name}/Dm_inv32']) + f4(golden[f'{name}/f_area32']) + f4(x))
            shapes.append((name, B, V))
    return shapes


@pytest.mark.parametrize('sanitize', (False, True), ids=('plain', 'sanitized'))
def test_cloth_rules_native(golden, tmp_path, sanitize):
    """tests/native/cloth_rules_main.cpp: a stand-alone program (its own main) around csrc/ra_cloth_rules.hpp, built plain and with
    -fsanitize=address,undefined, run on the CPU.  Its float evaluation against the golden under the 10 x float32 rule."""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    cases, out = tmp_path / 'cases.bin', tmp_path / 'out.bin'
    shapes = _native_cases(golden, cases)
    exe = str(tmp_path / 'cloth_rules_main')
    flags = ['-std=c++17', '-O1', '-g', '-ffp-contract=off']
    if sanitize:
        flags += ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
        flags += ['-static-libasan'] if os.path.basename(cxx).startswith('g++') else []      # gcc's spelling; clang links its runtime statically already
    r = subprocess.run([cxx] + flags + ['-I', os.path.join(REPO, 'relightableavatar_amd', 'csrc'), os.path.join(REPO, 'tests', 'native', 'cloth_rules_main.cpp'),
                                        '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, str(cases), str(out)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and f'cloth rules ok: {len(CASES)} cases' in r.stdout, r.stdout + r.stderr
    raw = open(out, 'rb').read()
    at = 0
    for name, B, V in shapes:
        es, eb = np.frombuffer(raw, '<f8', B, at), np.frombuffer(raw, '<f8', B, at + 8 * B)
        at += 16 * B
        gs = np.frombuffer(raw, '<f4', B * V * 3, at).reshape(B, V, 3)
        gb = np.frombuffer(raw, '<f4', B * V * 3, at + 4 * B * V * 3).reshape(B, V, 3)
        at += 8 * B * V * 3
        figures = {'stretch': abs(es.sum() / B - golden[f'{name}/stretch64']) / abs(golden[f'{name}/stretch64']),
                   'bending': abs(eb.sum() / B - golden[f'{name}/bending64']) / abs(golden[f'{name}/bending64']),
                   'stretch_grad': rel(gs / B, golden[f'{name}/stretch_grad64']), 'bending_grad': rel(gb / B, golden[f'{name}/bending_grad64'])}
        for k, err in figures.items():
            b = bound(golden, f'{name}/{k}')
            print(f'{name} {k}: error {err:.2e}, bound {b:.2e} (ratio to the reference\'s own float32 error {err / (b / 10):.2f})')
            assert err <= b, (name, k, err, b)
    assert at == len(raw)


def test_python_layer_and_abi():
    import re
    from relightableavatar_amd import _lib, engine, mesh_utils, physx_utils
    hdr = open(os.path.join(REPO, 'include', 'relightableavatar.h')).read()
    for sym in ('ra_cloth_material_derive', 'ra_cloth_create', 'ra_cloth_destroy', 'ra_cloth_array', 'ra_cloth_energy', 'ra_cloth_inertia', 'ra_cloth_tile'):
        assert sym in _lib.SYMBOLS and re.search(r'^int\s+' + sym + r'\s*\(', hdr, flags=re.M), sym
    L = _lib.lib()
    assert L.ra_abi_version() == 9
    assert [L.ra_cloth_tile(k) for k in range(5)] == [256, 256, 256, 2048, 0]
    for fn in ('StVKMaterial', 'Garment', 'get_shape_matrix', 'deformation_gradient', 'green_strain_tensor', 'stretch_energy', 'bending_energy',
               'gravity_energy', 'inertia_term', 'dynamic_term', 'inertia_term_sequence', 'cloth_energy'):
        assert callable(getattr(physx_utils, fn)), fn
    assert callable(mesh_utils.get_vertex_mass) and hasattr(engine.Engine, 'cloth') and hasattr(engine.Cloth, 'energy')
    for fn in ('stretch_energy_constraints', 'bending_energy_constraints', 'xpbd_constraints'):
        with pytest.raises(NotImplementedError, match='no working behaviour'):
            getattr(physx_utils, fn)(None, None)
    import torch
    tris = torch.tensor([[[1.0, 0, 0], [0, 2.0, 0], [0, 0, 0]]])
    Ds = physx_utils.get_shape_matrix(tris)
    assert Ds.shape == (1, 3, 2) and torch.equal(Ds[0, :, 0], tris[0, 0]) and torch.equal(Ds[0, :, 1], tris[0, 1])
    Fm = physx_utils.deformation_gradient(tris, torch.tensor([[[1.0, 0], [0, 0.5]]]))
    assert torch.allclose(physx_utils.green_strain_tensor(Fm), torch.zeros(1, 2, 2))
    x = torch.tensor([[[0.0, 2.0, 0.0], [0.0, -1.0, 0.0]]])
    assert float(physx_utils.gravity_energy(x, torch.tensor([0.5, 1.0]), 10.0)) == 0.0

"""The backward of marching cubes without a GPU:
    1. the float64 closed forms of tests/mcubes_grad_ref.py (dvolume, dattrs, the attribute forward) equal float64 autograd through
       t = (iso - a) / (b - a) at fixed topology;
    2. the float32 restatement in kernel order — what the device must equal bit for bit — is held to float64 under the 10 x float32 rule,
       the baseline being torch float32 autograd through the plain formula;
    3. sum(dvolume) = -sum(s): the two ends of an edge receive (t - 1) s and -t s;
    4. float64 central differences on the random volume, the step chosen so that no corner changes side;
    5. on a plane sdf = n . x - c with |n| = 1 and g = lambda n per vertex the reference's normal rule and the grid rule of
       differentiable_marching_cubes give the same d / dc and d / dn;
    6. tests/native/mcubes_grad_rules_main.cpp: the header's functions on the CPU under -fsanitize=address,undefined give the restatement's bits;
    7. the exports, the Python layer and the argument errors raised before a context is touched.
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

import mcubes_grad_ref as G
from frame_stage_ref import parity

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Both sides evaluate the same few operations per edge in float64 (eps 2.2e-16) and add at most six terms per grid point (1 + C per
# vertex for gt): a few hundred eps at the very most, relative to the largest entry.
CLOSED_FORM_TOL = 1e-12


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


@pytest.mark.parametrize('C_', (0, 3, 5))
@pytest.mark.parametrize('name', G.CPU_VOLUMES)
def test_closed_forms_equal_float64_autograd(name, C_):
    c = G.case(name, C_)
    dvol, dA, va = G.reference(name, C_, G.F64)
    gv, gA, gva = G.autograd(c['vol'], c['iso'], c['dverts'], c['attrs'], c['dattr'])
    fig = dict(dvolume=rel(dvol, gv))
    if C_:
        fig.update(dattrs=rel(dA, gA), vattrs=rel(va, gva))
    print(name, 'C', C_, 'verts', c['n_verts'], fig)
    assert c['n_verts'] > 0 and all(v <= CLOSED_FORM_TOL for v in fig.values()), fig


@pytest.mark.parametrize('name', G.CPU_VOLUMES)
def test_float32_restatement_under_the_10x_rule(name):
    c = G.case(name, 3)
    dvol, dA, va = G.reference(name, 3, G.F32)
    assert dvol.dtype == np.float32 and dA.dtype == np.float32 and va.dtype == np.float32
    r32 = G.autograd(c['vol'], c['iso'], c['dverts'], c['attrs'], c['dattr'], dtype=torch.float32)
    r64 = G.autograd(c['vol'], c['iso'], c['dverts'], c['attrs'], c['dattr'])
    for label, got, a, b in zip(('dvolume', 'dattrs', 'vattrs'), (dvol, dA.reshape(r64[1].shape), va), r32, r64):
        parity(f'{name} {label}', got.copy(), a, b)         # the shared reference is read-only


@pytest.mark.parametrize('name', G.CPU_VOLUMES)
def test_sum_identity(name):
    c = G.case(name, 3)
    dvol, _, s = G.backward(c['vol'], c['iso'], c['dverts'], c['attrs'], c['dattr'], G.F64, with_s=True)
    lhs, rhs, scale = float(dvol.sum()), -float(s.sum()), float(np.abs(s).sum())
    print(name, 'sum(dvolume)', lhs, '-sum(s)', rhs, 'sum|s|', scale)
    assert abs(lhs - rhs) <= 1e-12 * scale      # 2 V + n additions of float64 terms bounded by |s|


def test_central_differences_on_the_random_volume():
    """a and b of a crossed edge lie on two sides of iso, so |d| >= 2 m with m the smallest |value - iso|; a step h = 1e-3 m changes d by at
    most 5e-4 of itself and no corner's side.  t is a rational function of (a, b) whose third derivatives are O(t / d^3), so the central
    difference is off by O((h / d)^2) <= 2.5e-7 of the term, plus rounding eps / (h / d) ~ 1e-12: held to 1e-5 of the largest entry."""
    c = G.case('random', 3)
    vol64, iso = c['vol'].astype(np.float64), float(np.float32(c['iso']))
    m = float(np.abs(vol64 - iso).min())
    h = 1e-3 * m
    topo = c['topo']
    dv, da = torch.from_numpy(c['dverts']).double(), torch.from_numpy(c['dattr']).double()
    A = torch.from_numpy(c['attrs']).double()

    def loss(v):
        verts, va = G.torch_forward(torch.from_numpy(v), iso, topo, A)
        return float((verts * dv).sum() + (va * da).sum())

    dvol, _ = G.backward(vol64, iso, c['dverts'], c['attrs'], c['dattr'], G.F64)
    touched = np.flatnonzero(dvol.reshape(-1))
    picks = np.random.default_rng(0).choice(touched, 60, replace=False)
    worst = 0.0
    for p in picks:
        up, dn = vol64.copy().reshape(-1), vol64.copy().reshape(-1)
        up[p] += h
        dn[p] -= h
        assert np.array_equal(up < iso, vol64.reshape(-1) < iso) and np.array_equal(dn < iso, vol64.reshape(-1) < iso)
        fd = (loss(up.reshape(vol64.shape)) - loss(dn.reshape(vol64.shape))) / (2 * h)
        worst = max(worst, abs(fd - dvol.reshape(-1)[p]))
    scale = float(np.abs(dvol).max())
    print(f'central differences: m {m:.3e} h {h:.3e}, {len(picks)} of {len(touched)} touched grid points, worst |fd - closed| / max {worst / scale:.3e}')
    assert worst <= 1e-5 * scale


def test_normal_and_grid_rules_agree_on_a_plane():
    """a unit-gradient linear field: the grid rule moves a vertex along its edge by dc / n_k, which along the normal is dc — the normal rule"""
    shape = (7, 8, 9)
    pts = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in shape], indexing='ij'), -1)
    n = torch.nn.functional.normalize(torch.tensor([0.3, -0.5, 0.8], dtype=torch.float64), dim=0).requires_grad_()
    cc = (n.detach() @ torch.tensor([3.0, 3.5, 4.0], dtype=torch.float64) + 0.123).requires_grad_()
    decoder = lambda x: x @ n - cc
    vol = (-decoder(pts.reshape(-1, 3))).detach().reshape(shape).numpy()
    topo = G.topology(vol, 0.0)
    verts = G.torch_forward(torch.from_numpy(vol), 0.0, topo)[0]
    lam = torch.from_numpy(np.random.default_rng(1).standard_normal(topo['n_verts']))
    g = lam[:, None] * n.detach()
    dn_normal, dc_normal = G.normal_rule_grads(decoder, (n, cc), verts, g)
    dvolume = G.backward(vol, 0.0, g.numpy(), F=G.F64)[0]
    dn_grid, dc_grid = G.grid_rule_grads(decoder, (n, cc), pts, dvolume)
    fig = dict(verts=topo['n_verts'], dc=(float(dc_normal), float(dc_grid)), dn=rel(dn_grid, dn_normal))
    print('plane:', fig, 'residual of the vertices', float(decoder(verts).detach().abs().max()))
    assert topo['n_verts'] > 50
    assert abs(float(dc_normal) - float(dc_grid)) <= 1e-12 * abs(float(dc_normal)) and fig['dn'] <= 1e-12


def _hex(a):
    return ' '.join(f'{v:08x}' for v in np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1).tolist())


@pytest.fixture(scope='module')
def native_exe(tmp_path_factory):
    """tests/native/mcubes_grad_rules_main.cpp built once with -fsanitize=address,undefined: a stand-alone program, its own main"""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('mcubes_grad_native') / 'mcubes_grad_rules_main')
    flags = ['-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    flags += ['-static-libasan'] if os.path.basename(cxx).startswith('g++') else []      # gcc's spelling; clang links its runtime statically already
    r = subprocess.run([cxx] + flags + ['-I', os.path.join(REPO, 'relightableavatar_amd', 'csrc'),
                                        os.path.join(REPO, 'tests', 'native', 'mcubes_grad_rules_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.mark.parametrize('name,C_,with_dverts', [('random', 3, True), ('exact_iso', 4, True), ('2x2x2', 1, True), ('random', 0, True), ('random', 5, False)])
def test_mcubes_grad_rules_native(tmp_path, native_exe, name, C_, with_dverts):
    """the header's functions on the CPU under the sanitizers: the gather and the attribute forward equal the float32 restatement bit for bit"""
    exe = native_exe
    c = G.case(name, C_)
    vol, V = c['vol'], c['n_verts']
    dverts = c['dverts'] if with_dverts else None
    want_dvol, want_dA = G.backward(vol, c['iso'], dverts, c['attrs'], c['dattr'], G.F32)
    want_attr = G.attrs_forward(vol, c['iso'], c['attrs'], G.F32) if C_ else np.zeros((V, 0), np.float32)
    path = str(tmp_path / 'case.txt')
    empty = np.zeros(0, np.float32)
    with open(path, 'w') as fh:
        fh.write(f'{vol.shape[0]} {vol.shape[1]} {vol.shape[2]} {C_} {V} {int(with_dverts)} {_hex(np.float32(c["iso"]))}\n{_hex(vol)}\n'
                 f'{_hex(dverts if with_dverts else empty)}\n{_hex(c["attrs"] if C_ else empty)}\n{_hex(c["dattr"] if C_ else empty)}\n')
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines()}
    assert lines['verts'] == [str(V)]
    for key, want in (('dvol', want_dvol), ('dA', want_dA if C_ else empty), ('attr', want_attr)):
        got = np.array([int(t, 16) for t in lines[key]], np.uint32)
        ref = np.ascontiguousarray(want, np.float32).view(np.uint32).reshape(-1)
        diff = int((got != ref).sum()) if got.shape == ref.shape else -1
        print(name, 'C', C_, key, got.size, 'values,', diff, 'differ')
        assert diff == 0, key


def test_exports_python_layer_and_null_arguments():
    from relightableavatar_amd import _lib, engine, mesh_utils
    hdr = open(os.path.join(REPO, 'include', 'relightableavatar.h')).read()
    for sym in ('ra_marching_cubes_attrs', 'ra_marching_cubes_backward'):
        assert sym in _lib.SYMBOLS and re.search(r'^int\s+' + sym + r'\s*\(', hdr, flags=re.M), sym
    assert re.search(r'#define\s+RA_ABI_VERSION\s+9\b', hdr) and _lib.ABI_VERSION == 9
    L = _lib.lib()
    assert L.ra_abi_version() == 9
    assert list(inspect.signature(engine.Engine.marching_cubes_attrs).parameters) == ['self', 'volume', 'iso', 'attrs', 'n_verts']
    sig = inspect.signature(engine.Engine.marching_cubes_backward)
    assert list(sig.parameters) == ['self', 'volume', 'iso', 'n_verts', 'dverts', 'attrs', 'dattr', 'want'] and sig.parameters['want'].default == ('dvolume', 'dattrs')
    assert list(inspect.signature(mesh_utils.marching_cubes).parameters) == ['volume', 'iso', 'attrs', 'engine']
    sig = inspect.signature(mesh_utils.differentiable_marching_cubes)
    assert list(sig.parameters) == ['points', 'decoder', 'chunk_size', 'engine', 'gradient']
    assert sig.parameters['chunk_size'].default == 65536 and sig.parameters['gradient'].default == 'normal'
    for word in ('marching_cubes(volume, iso', 'differentiable_marching_cubes(points, decoder'):
        assert word in mesh_utils.__doc__, word
    err = lambda: L.ra_last_error().decode()
    p = C.c_void_p(16)          # never dereferenced: every call below fails on its arguments
    assert L.ra_marching_cubes_attrs(None, p, 4, 4, 4, 0.0, p, 3, 8, p, None) != 0 and 'ra_marching_cubes_attrs: null argument' in err()
    assert L.ra_marching_cubes_backward(None, p, 4, 4, 4, 0.0, p, 8, p, p, 3, p, p, None) != 0 and 'ra_marching_cubes_backward: null argument' in err()
    with pytest.raises(ValueError):
        mesh_utils.differentiable_marching_cubes(torch.zeros(2, 2, 2, 3), lambda x: x[:, 0], gradient='both')

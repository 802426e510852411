"""Silhouette antialiasing without a GPU:
    1. the float64 closed-form gradients the kernels use (tests/antialias_ref.py) equal float64 autograd through the rule;
    2. the float32 restatement in kernel order — what ra_antialias must equal bit for bit on the device — and the float64 restatement choose
       the same (pair, own pixel, edge) on every decided pair; the cases that are compared by value hold at least 100 active pairs and at
       most 2 % undecided ones, and there the kernel-order restatement stays under the 10 x float32 rule;
    3. on an axis-aligned rectangle with varying w the antialiased coverage is closer to the exact area than the plain one at five shifts;
    4. tests/native/antialias_rules_main.cpp: the header's functions on the CPU under -fsanitize=address,undefined give the restatement's
       bits;
    5. the Python layer, and argument errors of the two entry points that are raised before any launch.
Every test prints its figures before it asserts."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import antialias_ref as A
import raster_ref as R
from frame_stage_ref import parity

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_VALUE = ('two_triangles_32x32', 'open_37x53', 'sphere2_136x200', 'tri012_130x70')
# float64 closed forms against float64 autograd: both evaluate the same formulas in float64 (eps 2.2e-16) over sums of at most a few
# hundred terms, so they agree to a small multiple of eps relative to the largest value; 1e-12 leaves three orders for the sums and the
# divisions by an edge coefficient, and a wrong formula is off by orders of one.
CLOSED_FORM_BOUND = 1e-12


@pytest.mark.parametrize('name', A.CASES)
def test_case_classification(name):
    c = A.case(name)
    n = A.counts(c)
    share = n['undecided'] / max(n['candidates'], 1)
    print(f'{name}: {c["H"]} x {c["W"]}, {c["pos"].shape[0]} view(s), {n["candidates"]} pairs, active {n["active64"]} (float64) {n["active32"]} (float32), '
          f'undecided {n["undecided"]} ({share:.2%}), decided pairs on which the precisions differ {n["differ"]}')
    assert n['differ'] == 0
    for p32, p64 in zip(c['p32'], c['p64']):
        assert not (p64['active'] & ~p64['candidate']).any() and not (p32['active'] & ~p32['candidate']).any()
        assert np.array_equal(p32['slot'], np.sort(p32['slot'])) and len(np.unique(p32['slot'])) == len(p32['slot'])
    if name in BY_VALUE:
        assert n['active64'] >= A.MIN_ACTIVE and share <= A.UNDECIDED_CAP, name
    if name == 'two_triangles_32x32':       # both faces present: the own pixel is chosen by depth on pairs of two covered pixels
        p = c['p32'][0]
        face = c['face'][0].reshape(-1)
        both = p['active'] & (face[p['p0']] >= 0) & (face[p['p1']] >= 0)
        print(f'{name}: {int(both.sum())} active pairs between two covered pixels, own faces {np.unique(p["he"][both] // 3).tolist()}')
        assert int(both.sum()) > 50 and np.unique(p['he'][both] // 3).tolist() == [0]
    if name == 'tri012_130x70':             # a run longer than a wave on one half-edge
        runs = np.bincount(c['p32'][0]['he'][c['p32'][0]['active']])
        print(f'{name}: pairs per half-edge {runs.tolist()}')
        assert int(runs.max()) > 64
    if name in ('sphere_1x1', 'empty_8x8'):
        assert n['candidates'] == 0
    if name in ('two_triangles_1x9', 'two_triangles_9x1'):
        assert n['active32'] > 0 and len(np.unique(c['p32'][0]['vertical'])) == 1
    if name == 'degenerate_32x32':
        assert n['active32'] > 0 and not np.isfinite(c['pos']).all()
    if name == 'sphere2_136x200':           # silhouettes between a front and a back face, not only boundaries
        tw = A.twins(c['faces'])
        he = np.concatenate([p['he'][p['active']] for p in c['p32']])
        assert (tw[he] >= 0).all() and c['pos'].shape[0] == 2
    if name == 'open_37x53':
        tw = A.twins(c['faces'])
        he = c['p32'][0]['he'][c['p32'][0]['active']]
        assert (tw[he] < 0).any()


@pytest.mark.parametrize('name', BY_VALUE)
def test_closed_form_equals_autograd_and_parity(name):
    c, r = A.case(name), A.reference(name, 4)
    col64 = r['color'].astype(np.float64)
    c64 = A.grads(col64, c['pos'], c['faces'], c['p64'], r['dout'])
    o64 = A.blend(col64, c['p64'])
    t64, t32 = r['t64'], r['t32']
    rels = {'out': float(np.abs(o64 - t64['out']).max() / np.abs(t64['out']).max())}
    for k in ('dcolor', 'dpos'):
        rels[k] = float(np.abs(c64[k] - t64[k]).max() / max(float(np.abs(t64[k]).max()), 1e-300))
    for k, rel in rels.items():
        print(f'{name} {k}: float64 closed form against float64 autograd, relative {rel:.2e}')
    for k, rel in rels.items():
        assert rel <= CLOSED_FORM_BOUND, (name, k)
    keep_pix = np.broadcast_to(r['keep_pix'][..., None], r['out'].shape).copy()
    keep_vert = np.broadcast_to(r['keep_vert'][..., None], r['kernel']['dpos'].shape).copy()
    print(f'{name}: compared on {int(r["keep_pix"].sum())} of {r["keep_pix"].size} pixels and {int(r["keep_vert"].sum())} of {r["keep_vert"].size} vertices')
    parity(f'{name} out kernel order', r['out'], t32['out'], t64['out'], keep=keep_pix)
    parity(f'{name} dcolor kernel order', r['kernel']['dcolor'], t32['dcolor'], t64['dcolor'], keep=keep_pix)
    assert keep_pix.any()
    if name == 'tri012_130x70':         # all three vertices touch an undecided pair: nothing of dpos is left to compare by value
        assert not keep_vert.any()
    else:
        assert keep_vert.any()
        parity(f'{name} dpos kernel order', r['kernel']['dpos'], t32['dpos'], t64['dpos'], keep=keep_vert)
    pos, faces = c['pos'], c['faces']
    used = np.zeros(pos.shape[1], bool)
    used[faces.reshape(-1)] = True
    assert not r['kernel']['dpos'][:, ~used].any() and not r['kernel']['dpos'][..., 2].any()
    assert np.array_equal(r['kernel3']['dcolor'], r['kernel']['dcolor']) and np.array_equal(r['kernel3']['dpos'], r['kernel']['dpos'] * np.float32(3))


def test_rectangle_coverage():
    """antialiased coverage of the mask is closer to the exact area than plain coverage at each of five sub-pixel shifts"""
    for s in A.RECT_SHIFTS:
        pos, f, area = A.rectangle(s)
        r = R.raster(pos, f, 24, 32, np.float32)
        mask = (r['face'] >= 0).astype(np.float32)[..., None]
        prs = A.pairs(r['face'], r['zw'].astype(np.float32), pos[None], f, np.float32)
        plain, aa = float(mask.sum(dtype=np.float64)), float(A.blend(mask, prs).sum(dtype=np.float64))
        print(f'shift {s}: exact {area:.3f} px, plain {plain:.1f}, antialiased {aa:.3f}')
        assert abs(aa - area) < abs(plain - area), s


def _hex(a):
    return ' '.join(f'{v:08x}' for v in np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1).tolist())


@pytest.mark.parametrize('name', ['two_triangles_32x32', 'degenerate_32x32', 'open_37x53'])
def test_antialias_rules_native(tmp_path, name):
    """tests/native/antialias_rules_main.cpp: a stand-alone program (its own main) around csrc/ra_antialias_rules.hpp, built with
    -fsanitize=address,undefined and run on the CPU; its pairs, their gradients and the forward equal the float32 restatement bit for bit"""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'antialias_rules_main')
    flags = ['-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    flags += ['-static-libasan'] if os.path.basename(cxx).startswith('g++') else []      # gcc's spelling; clang links its runtime statically already
    r = subprocess.run([cxx] + flags + ['-I', os.path.join(REPO, 'relightableavatar_amd', 'csrc'), os.path.join(REPO, 'tests', 'native', 'antialias_rules_main.cpp'),
                                        '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    c, ref = A.case(name), A.reference(name, 4)
    B, V = c['pos'].shape[:2]
    H, W, faces = c['H'], c['W'], c['faces']
    path = str(tmp_path / 'case.txt')
    with open(path, 'w') as fh:
        fh.write(f'{B} {V} {len(faces)} {H} {W} 4\n{_hex(c["pos"])}\n{" ".join(map(str, faces.reshape(-1).tolist()))}\n'
                 f'{" ".join(map(str, c["face"].reshape(-1).tolist()))}\n{_hex(c["zw"])}\n{_hex(ref["color"])}\n{_hex(ref["dout"])}\n')
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == 'flags 0', lines[0]
    got_pairs = [l.split()[1:] for l in lines if l.startswith('pair ')]
    got_out = {tuple(int(t) for t in l.split()[1:4]): l.split()[4] for l in lines if l.startswith('out ')}
    u32 = lambda x: f'{int(np.asarray(x, np.float32).view(np.uint32)):08x}'
    want_pairs = []
    for b, p in enumerate(c['p32']):
        i, dc = A.pair_dc(ref['color'], ref['dout'], p, b, H, W)
        for n, q in enumerate(i):
            he = int(p['he'][q])
            f, k = he // 3, he % 3
            tail, head = int(faces[f, k]), int(faces[f, (k + 1) % 3])
            a, bb = c['pos'][b, min(tail, head)][[0, 1, 3]], c['pos'][b, max(tail, head)][[0, 1, 3]]
            with np.errstate(all='ignore'):
                da, db = A._cross(bb, dc[n]), A._cross(dc[n], a)
            want_pairs.append([str(b), str(int(p['slot'][q])), str(int(p['own'][q])), str(int(p['k'][q])), str(he), u32(p['alpha'][q])] +
                              [u32(v) for v in p['c'][q]] + [u32(p['cross'][q])] + [u32(v) for v in dc[n]] + [u32(v) for v in da] + [u32(v) for v in db])
    changed = ref['out'].view(np.uint32) != ref['color'].view(np.uint32)
    want_out = {(int(b), int(y) * W + int(x), int(ch)): u32(ref['out'][b, y, x, ch]) for b, y, x, ch in zip(*np.nonzero(changed))}
    print(f'{name}: {lines[-1]}; the restatement has {len(want_pairs)} active pairs and {len(want_out)} changed values')
    assert lines[-1] == f'done {len(want_pairs)} {len(want_out)}'
    assert got_pairs == want_pairs
    assert got_out == want_out


def test_python_layer_and_argument_errors():
    import inspect
    import re
    from relightableavatar_amd import _lib, engine, raster_utils
    hdr = open(os.path.join(REPO, 'include', 'relightableavatar.h')).read()
    for sym in ('ra_antialias', 'ra_antialias_backward'):
        assert sym in _lib.SYMBOLS and re.search(r'^int\s+' + sym + r'\s*\(', hdr, flags=re.M), sym
    L = _lib.lib()
    assert L.ra_abi_version() == 9
    assert all(hasattr(engine.Engine, k) for k in ('antialias', 'antialias_backward')) and callable(raster_utils.antialias)
    sig = inspect.signature(raster_utils.antialias)
    assert list(sig.parameters)[:6] == ['color', 'rast', 'pos', 'tri', 'topology_hash', 'pos_gradient_boost']
    assert inspect.signature(raster_utils.render_nvdiffrast).parameters['antialias'].default is False
    err = lambda: L.ra_last_error().decode()
    p = C.c_void_p(16)          # never dereferenced: every call below fails on its arguments
    # ra_antialias(ctx, topo, color, C, pos, B, V, zw, face, H, W, out, stream)
    for Cn, B, H, W in ((0, 1, 8, 8), (1, -1, 8, 8), (1, 1, -1, 8), (4, 1, 1 << 15, 1 << 15), (1, 2, 1 << 15, 1 << 15)):
        assert L.ra_antialias(None, p, p, Cn, p, B, 4, p, p, H, W, p, None) != 0 and 'ra_antialias: bad sizes' in err(), (Cn, B, H, W)
        assert L.ra_antialias_backward(None, p, p, Cn, p, B, 4, p, p, H, W, p, 1.0, p, p, None) != 0 and 'ra_antialias_backward: bad sizes' in err()
    assert L.ra_antialias(None, p, p, 4, p, 1, 4, p, p, 8, 8, p, None) != 0 and 'ra_antialias: null argument' in err()
    assert L.ra_antialias_backward(None, p, p, 4, p, 1, 4, p, p, 8, 8, p, 1.0, p, p, None) != 0 and 'ra_antialias_backward: null argument' in err()
    with pytest.raises(ValueError):
        raster_utils.antialias(torch.zeros(1, 2, 2, 1), torch.zeros(1, 2, 2, 4), torch.zeros(3, 4), torch.zeros(1, 3, dtype=torch.int32))

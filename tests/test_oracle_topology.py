"""Mesh connectivity and Taubin smoothing against the reference's own outputs (tests/golden/topology.npz, made by
tests/golden/make_golden_topology.py), on the CPU:

    1. the seed-built meshes regenerate;
    2. the restatement (tests/topology_ref.py) reproduces every integer array of the golden exactly;
    3. get_edges: the restatement's TRUE edges equal the reference's rows wherever the true max is not faces.max(), and on those rows
       the reference's equal (min + 1, 0): the one deliberate deviation, asserted;
    4. face connectivity as unordered pairs per edge (the reference leaves the order inside a pair to an unstable argsort);
    5. smoothing under the 10 x float32 rule: the float32 restatement's distance from the float64 restatement, max and median
       normalised by max |ref|, is at most 10 x the reference's float32 golden's distance from the same float64 restatement;
    6. tests/native/topo_rules_main.cpp: csrc/ra_topo_rules.hpp compiled for the host with sanitizers against the restatement;
    7. Loop subdivision: the child-topology arithmetic reproduces the reference's half-edge arrays and faces after 1 and 2 steps
       exactly; positions, as corner positions verts[faces], under the same 10 x rule, the float64 restatement (float64 coefficients)
       being closer to the reference's float64 run than the reference's float32 run is; the library's coefficient table within one
       fp32 ulp of numpy's float64 formula.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import topology_ref as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden', 'topology.npz')
NAMES = tuple(T.MESHES)
EPS32 = 2.0 ** -23


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def test_golden_inputs_regenerate(golden):
    assert tuple(golden['meshes']) == NAMES
    for name in NAMES:
        v, f = T.mesh(name)
        assert np.array_equal(golden[f'{name}/verts'], v) and np.array_equal(golden[f'{name}/faces'], f), name
    assert os.path.getsize(GOLDEN) < 1 << 20
    sizes = {len(T.mesh(n)[0]) for n in NAMES}
    assert {6, 63, 64, 65, 66, 255, 256, 257, 258, 1026} <= sizes


@pytest.mark.parametrize('name', NAMES)
def test_restatement_reproduces_the_goldens_integers(golden, name):
    t = T.topo(name)
    assert t['E'] == int(golden[f'{name}/he_E'])
    for k in ('twin', 'vert', 'edge'):
        assert np.array_equal(t[k], golden[f'{name}/he_{k}']), k
    assert np.array_equal(t['edge'], golden[f'{name}/ge_i']) and np.array_equal(t['edge_counts'], golden[f'{name}/ge_c'])
    # the structure's own invariants
    tw = t['twin']
    pair = tw >= 0
    assert np.array_equal(tw[tw[pair]], np.flatnonzero(pair)), 'the pairing is symmetric'
    assert np.array_equal(t['edge'][tw[pair]], t['edge'][pair])
    assert np.array_equal(-tw[~pair], t['edge_counts'][t['edge'][~pair]])
    e = t['edges']
    assert np.all(e[:, 0] <= e[:, 1]) and np.all(np.diff(e[:, 0] * (1 << 32) + e[:, 1]) > 0), 'true (min, max), lexicographic'
    for start, lst in ((t['nbr_start'], t['nbr']), (t['out_start'], t['out_he']), (t['edge_he_start'], t['edge_he'])):
        for a, b in zip(start[:-1], start[1:]):
            assert np.all(np.diff(lst[a:b]) >= 0)


@pytest.mark.parametrize('name', NAMES)
def test_get_edges_deviation_is_exactly_the_last_vertex(golden, name):
    t, (v, f) = T.topo(name), T.mesh(name)
    ref, true = golden[f'{name}/ge_e'], t['edges']
    last = true[:, 1] == f.max()
    assert last.any()
    assert np.array_equal(ref[~last], true[~last])
    assert np.array_equal(ref[last], np.stack([true[last, 0] + 1, np.zeros(last.sum(), dtype=np.int64)], axis=1))
    assert np.array_equal(T.reference_decoded_edges(true, f), ref)


@pytest.mark.parametrize('name', NAMES)
def test_face_connectivity_as_unordered_pairs(golden, name):
    t, (v, f) = T.topo(name), T.mesh(name)
    ev, cf = T.face_connectivity(t)
    rv, rf = golden[f'{name}/fc_edges'], golden[f'{name}/fc_faces']
    assert ev.shape == rv.shape and cf.shape == rf.shape == (int((t['edge_counts'] == 2).sum()), 2)
    big = len(f) + 1
    assert np.array_equal(np.sort(ev * big + cf, axis=1), np.sort(rv * big + rf, axis=1))
    assert np.all(cf[:, 0] <= cf[:, 1])


def _err(a, ref):
    d = np.abs(np.asarray(a, dtype=np.float64) - ref) / np.abs(ref).max()
    return d.max(), np.median(d)


# the largest mesh runs the long case only: the numpy loop over its passes is the slow part
SMOOTH_CASES = [(n, c) for n in NAMES for c in ('1', '2', '90', '90_inds') if len(T.smooth_iters(n)) > 1 or c == '90']


@pytest.mark.parametrize('name,case', SMOOTH_CASES)
def test_smoothing_under_the_ten_times_float32_rule(golden, name, case):
    t, (v, f) = T.topo(name), T.mesh(name)
    iters = int(case.split('_')[0])
    inds = T.smooth_inds(name) if case.endswith('inds') else None
    v32 = v.astype(np.float32)
    r64 = T.taubin(v32, t, inds, 0.33, iters, np.float64)
    r32 = T.taubin(v32, t, inds, 0.33, iters, np.float32)
    assert r32.dtype == np.float32
    gold = golden[f'{name}/smooth{case}']
    (gmax, gmed), (rmax, rmed) = _err(gold, r64), _err(r32, r64)
    print(f'{name}/{case}: reference float32 vs float64 restatement max {gmax:.3e} median {gmed:.3e}; float32 restatement max {rmax:.3e} median {rmed:.3e}')
    assert rmax <= 10 * (gmax if gmax > 0 else EPS32) and rmed <= 10 * (gmed if gmed > 0 else EPS32)
    # the float64 restatement is the reference's arithmetic: what separates them is the reference's float32 rounding, at most
    # deg + 4 roundings of 2^-24 max |v| per row and pass (sum, 1 / deg, product, difference, scaling, update) added up over the
    # passes, times 2 for the anti-diffusive pass, which may enlarge an error by up to 1 + 2 x 0.34 before the next pass shrinks it
    assert gmax <= 2 * (2 * iters) * (t['max_valence'] + 4) * 2.0 ** -24
    if inds is not None:
        still = np.ones(len(v), dtype=bool)
        still[inds] = False
        assert np.array_equal(r32[still], v32[still]) and np.array_equal(gold[still], v32[still])


def test_unconnected_vertex_shrinks_like_the_references(golden):
    v, f = T.mesh('unref')
    r = T.taubin(v.astype(np.float32), T.topo('unref'), None, 0.33, 1, np.float64)
    for k in (3, 7):
        assert np.allclose(r[k], v[k].astype(np.float32) * (1 - 0.33) * (1 + 0.34), rtol=1e-6)
        assert np.allclose(golden['unref/smooth1'][k], r[k], rtol=1e-5)


def test_topo_rules_native(tmp_path):
    """tests/native/topo_rules_main.cpp: a stand-alone program (its own main) around csrc/ra_topo_rules.hpp — the edge key, the twin
    rule and the Taubin step the kernels inline, in the same IEEE fp32 operations — built with -fsanitize=address,undefined and run
    on the CPU against the restatement's values."""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    cases = tmp_path / 'cases.bin'
    with open(cases, 'wb') as fh:
        for name, C, iters in (('octa', 3, 2), ('patch5', 1, 3), ('fin', 4, 2), ('repeat', 3, 2), ('unref', 3, 1), ('fan40', 3, 5), ('v65', 3, 90), ('two', 55, 1)):
            t, (v, f) = T.topo(name), T.mesh(name)
            rng = np.random.default_rng(11)
            vals = np.concatenate([v, rng.standard_normal((len(v), max(C - 3, 0)))], axis=1)[:, :C].astype(np.float32)
            want = T.taubin(vals, t, None, 0.33, iters, np.float32)
            fh.write(struct.pack('<5if', len(f), len(v), t['E'], C, iters, 0.33))
            for a in (f, t['edge'], t['twin'], t['nbr_start'], t['nbr']):
                fh.write(np.ascontiguousarray(a, dtype='<i4').tobytes())
            fh.write(vals.astype('<f4').tobytes())
            fh.write(want.astype('<f4').tobytes())
            table = T.loop_table(max(t['max_outgoing'], 1), np.float32)
            child = T.child_topology(t, len(v))
            fh.write(struct.pack('<i', len(table) - 1))
            fh.write(table.astype('<f4').tobytes())
            for a in (t['out_start'], t['out_he'], t['edge_he_start'], t['edge_he']):
                fh.write(np.ascontiguousarray(a, dtype='<i4').tobytes())
            fh.write(T.loop_step(vals, t, table, np.float32).astype('<f4').tobytes())
            for a in (child['twin'], child['edge'], child['vert']):
                fh.write(np.ascontiguousarray(a, dtype='<i4').tobytes())
    exe = str(tmp_path / 'topo_rules_main')
    static = ['-static-libasan'] if os.path.basename(cxx).startswith('g++') else []          # gcc's spelling; clang links its runtime statically already
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + static +
                       ['-I', os.path.join(REPO, 'relightableavatar_amd', 'csrc'), os.path.join(REPO, 'tests', 'native', 'topo_rules_main.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and 'topo rules ok: 8 cases' in r.stdout, r.stdout + r.stderr


LOOP_CASES = [(n, k) for n in NAMES for k in T.loop_steps(n)]


@pytest.mark.parametrize('name,steps', LOOP_CASES)
def test_loop_topology_reproduces_the_goldens_integers(golden, name, steps):
    v, f = T.mesh(name)
    _, faces, t = T.subdivide(v, T.topo(name), steps, np.float64)
    for k in ('twin', 'vert', 'edge'):
        assert np.array_equal(t[k], golden[f'{name}/loop{steps}_{k}']), k
    assert np.array_equal(faces, golden[f'{name}/loop{steps}_faces']) and len(faces) == 4 ** steps * len(f)


@pytest.mark.parametrize('name,steps', LOOP_CASES)
def test_loop_positions_under_the_ten_times_float32_rule(golden, name, steps):
    v, f = T.mesh(name)
    v32 = v.astype(np.float32)
    r64, faces, _ = T.subdivide(v32, T.topo(name), steps, np.float64)
    r32, _, _ = T.subdivide(v32, T.topo(name), steps, np.float32)
    assert r32.dtype == np.float32
    g32, g64 = golden[f'{name}/loop{steps}_v32'], golden[f'{name}/loop{steps}_v64']
    # the golden ran on the float64 vertices for its float64 result: restate that input too for the comparison with it
    q64, _, _ = T.subdivide(v, T.topo(name), steps, np.float64)
    own = _err(q64[faces], g64[faces])[0]
    (gmax, gmed), (rmax, rmed) = _err(g32[faces], r64[faces]), _err(r32[faces], r64[faces])
    print(f'{name}/{steps}: float64 restatement vs the reference in float64 {own:.3e}; reference float32 vs float64 restatement max {gmax:.3e} median {gmed:.3e}; '
          f'float32 restatement max {rmax:.3e} median {rmed:.3e}')
    assert rmax <= 10 * (gmax if gmax > 0 else EPS32) and rmed <= 10 * (gmed if gmed > 0 else EPS32)
    assert own <= gmax or own <= EPS32, 'the float64 restatement is nearer the reference than the reference\'s own float32 run'


def test_loop_quirks_kept(golden):
    """an ear gets half its stencil, an unreferenced vertex moves to the origin"""
    v = np.array([[x, y, 0.0] for y in range(3) for x in range(3)], dtype=np.float64)
    f = T.patch(3)[1]
    assert (f == 2).sum() == 1 and [1, 2, 5] in f.tolist()       # corner (2, 0) belongs to the face (1, 2, 5) alone
    out = T.loop_step(v, T.halfedge_build(f, 9), T.loop_table(6), np.float64)
    # only its outgoing boundary half-edge 2 -> 5 contributes, 3 / 8 of itself and 1 / 8 of (2, 1): the arriving one, 1 -> 2, has no
    # twin to be mirrored through.  The full boundary rule would give 3 / 4 (2, 0) + 1 / 8 ((1, 0) + (2, 1)) = (1.875, 0.125)
    assert np.allclose(out[2], [1.0, 0.125, 0.0]), out[2]
    assert np.allclose(out[1], 0.75 * v[1] + 0.125 * (v[0] + v[2])), 'a boundary vertex of two faces gets the whole rule'
    r, _, _ = T.subdivide(T.mesh('unref')[0], T.topo('unref'), 1, np.float64)
    assert np.all(r[3] == 0) and np.all(r[7] == 0) and np.all(golden['unref/loop1_v64'][[3, 7]] == 0)
    w = T.loop_table(64)
    assert np.allclose((w[1:, 0] + w[1:, 1]) * np.arange(1, 65), 1.0), 'the interior stencil sums to 1: n contributions of w_self + beta'


def test_loop_weights_of_the_library():
    import ctypes as C
    from relightableavatar_amd import _lib
    L = _lib.lib()
    want = T.loop_table(64, np.float64)
    for n in range(1, 65):
        w, b = C.c_float(), C.c_float()
        assert L.ra_loop_weights(n, C.byref(w), C.byref(b)) == 0
        for got, ref in ((w.value, want[n, 0]), (b.value, want[n, 1])):
            assert abs(got - ref) <= np.spacing(np.float32(abs(ref))), (n, got, ref)
    assert L.ra_loop_weights(0, C.byref(w), C.byref(b)) != 0 and b'bad sizes' in L.ra_last_error()
    assert L.ra_loop_weights(3, None, C.byref(b)) != 0 and b'null argument' in L.ra_last_error()


def test_python_layer_and_abi():
    import re
    from relightableavatar_amd import _lib, engine, mesh_utils
    hdr = open(os.path.join(REPO, 'include', 'relightableavatar.h')).read()
    for sym in ('ra_topo_create', 'ra_topo_destroy', 'ra_topo_sizes', 'ra_topo_array', 'ra_topo_tile', 'ra_mesh_smooth', 'ra_topo_dilate', 'ra_mesh_subdivide', 'ra_loop_weights'):
        assert sym in _lib.SYMBOLS and re.search(r'\b' + sym + r'\(', hdr), sym
    enum = re.search(r'enum \{ (RA_TOPO_VERT.*?) \};', hdr, re.S).group(1)
    names = [n.split('=')[0].strip() for n in enum.split(',')]
    assert [n[len('RA_TOPO_'):].lower() for n in names] == list(_lib.RA_TOPO_ARRAYS)
    L = _lib.lib()
    assert L.ra_topo_tile(0) > 0 and L.ra_topo_tile(1) > 0 and L.ra_topo_tile(2) == 64 and L.ra_topo_tile(3) == 0
    for fn in ('get_edges', 'laplacian_smoothing', 'triangle_to_halfedge', 'get_face_connectivity', 'halfedge_loop_subdivision', 'multiple_halfedge_loop_subdivision',
               'halfedge_to_triangle', 'loop_subdivision'):
        assert callable(getattr(mesh_utils, fn))
    import torch
    with pytest.raises(ValueError, match='get_edges returned'):
        mesh_utils.laplacian_smoothing(torch.zeros(4, 3), torch.zeros(3, 2, dtype=torch.long))
    assert hasattr(engine.Engine, 'topology') and hasattr(engine.Topology, 'smooth') and hasattr(engine.Topology, 'dilate')

"""The texture path without a GPU:
    1. the float64 closed-form duv and dtex (tests/texture_ref.py) equal float64 autograd through the torch restatement;
    2. independent yardsticks: linear + clamp at level 0 is F.grid_sample(bilinear, border, align_corners=False), the mip chain is repeated
       F.avg_pool2d(2), rast_db is the central difference of the float64 barycentrics of raster_ref;
    3. the float32 restatement in kernel order — what the device must equal bit for bit — against float64 under the 10 x float32 rule,
       the plain baseline using numpy's own float32 log2; the share of undecided pixels is at most 2 %;
    4. the header's log2 polynomial against float64 log2 over a dense sweep;
    5. tests/native/texture_rules_main.cpp: the header's functions on the CPU under -fsanitize=address,undefined give the restatement's bits;
    6. the Python layer, and the argument errors of the new entry points, raised before any launch.
Every test prints its figures before it asserts."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import raster_ref as R
import texture_ref as X
from frame_stage_ref import parity

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# float64 closed forms against float64 autograd: both evaluate the same formulas in float64 (eps 2.2e-16) over sums of at most a few
# thousand terms, so they agree to a small multiple of eps relative to the largest value — the bound and the argument of
# test_oracle_antialias.CLOSED_FORM_BOUND
CLOSED_FORM_BOUND = 1e-12
# texture_log2 = e + fraction.  The polynomial's truncation (the s^11 term, below 1e-9) is far under float32 rounding; its rounded
# operations (a division, nine products and sums on values of at most 2.9, the last product) leave a few ulp of the fraction (|fraction|
# <= 0.5, ulp 6e-8): four of those, 2.4e-7.  The last sum e + fraction rounds to the result's own spacing: half an ulp of the result.
LOG2_FRACTION_BOUND = 2.4e-7
MODES = [(f, b) for f in X.FILTERS for b in X.BOUNDARIES]


def _rel(a, b):
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-300))


@pytest.mark.parametrize('name', X.CASES)
def test_case_classification(name):
    c = X.case(name)
    for filt, bnd in MODES:
        r = X.reference(name, filt, bnd)
        und = r['undecided']
        share = float(und.mean())
        runs = r['runs']
        print(f'{name} {filt} {bnd}: {und.size} pixels, undecided {int(und.sum())} ({share:.2%}), levels {len(r["px32"]["hs"])}, '
              f'l0 used {np.unique(r["px32"]["l0"][r["px32"]["ok"]]).tolist()}, runs {len(runs)} (longest {int(runs.max()) if len(runs) else 0})')
        assert share <= X.UNDECIDED_CAP, (name, filt, bnd)
        if c['kind'] == 'boundary':
            assert not und.any()
    hs, ws, _ = X.levels(c['TH'], c['TW'], c['max_mip_level'])
    if name.startswith('t8x2'):
        assert (hs[-1], ws[-1]) == (4, 1)
    if name.startswith('t5x3') or name.startswith('t1x1'):
        assert len(hs) == 1
    if name.startswith('t16_mm8'):
        assert (hs[-1], ws[-1]) == (1, 1) and len(hs) == 5
    if name.startswith('t16_mm2'):
        assert len(hs) == 3
    if c['kind'] == 'runs':
        runs = np.sort(X.reference(name, X.NEAREST, 'wrap')['runs']).tolist()
        print(f'{name}: pixels per texel {runs}')
        assert runs == list(X.RUN_LENGTHS)
    if c['kind'] == 'magnify':
        assert int(X.reference(name, X.LINEAR, 'wrap')['runs'].max()) > 1000
    if c['kind'] == 'boundary':
        px = X.reference(name, X.TRILINEAR, 'wrap')['px32']
        print(f'{name}: l0 {np.bincount(px["l0"].reshape(-1)).tolist()}, pixels with a second level {int(px["two"].sum())}')
        assert len(np.unique(px['l0'])) >= 3 and not px['two'].any() and int(px['l0'].max()) == c['Lmax']
        lin = X.reference(name, X.LINEAR, 'wrap')['px32']
        assert (lin['fx'][0] == 0).any() and (lin['fx'][0] == 0.5).any()          # uv on texel centres and on texel boundaries
    if c['kind'] == 'zero_da':
        px = X.reference(name, X.TRILINEAR, 'wrap')['px32']
        assert not px['l0'].any() and not px['two'].any()
    if c['kind'] == 'random' and c['H'] * c['W'] > 2:
        px = X.reference(name, X.TRILINEAR, 'wrap')['px32']
        assert int((~px['ok']).sum()) == 3
        if c['Lmax'] >= 2:
            assert len(np.unique(px['l0'][px['ok']])) >= 3 and px['two'].any()


@pytest.mark.parametrize('name', X.BY_VALUE)
def test_closed_form_equals_autograd_and_parity(name):
    c = X.case(name)
    mm = c['max_mip_level']
    for filt, bnd in MODES:
        r = X.reference(name, filt, bnd)
        tag = f'{name} {filt} {bnd}'
        tex = torch.tensor(c['tex'], dtype=torch.float64, requires_grad=True)
        uv = torch.tensor(np.where(np.isfinite(c['uv']), c['uv'], 0), dtype=torch.float64, requires_grad=True)
        out = X.texture_torch(tex, uv, r['px64'], mm)
        dtex, duv = torch.autograd.grad((out * torch.tensor(c['dout'], dtype=torch.float64)).sum(), (tex, uv), allow_unused=True)
        rels = {'out': _rel(r['out64'], out.detach().numpy()), 'dtex': _rel(r['dtex64'], dtex.numpy())}
        if filt != X.NEAREST:
            rels['duv'] = _rel(r['duv64'], duv.numpy())
        else:
            assert duv is None or not bool(duv.any())
            assert not r['duv64'].any()
        for k, rel in rels.items():
            print(f'{tag} {k}: float64 closed form against float64 autograd, relative {rel:.2e}')
        for k, rel in rels.items():
            assert rel <= CLOSED_FORM_BOUND, (tag, k)
        und = r['undecided']
        keep = ~und
        print(f'{tag}: undecided {int(und.sum())} of {und.size} pixels ({float(und.mean()):.2%})')
        assert float(und.mean()) <= X.UNDECIDED_CAP
        if filt == X.NEAREST:
            parity(f'{tag} out kernel order', r['out32'], r['outplain'], r['out64'], keep=np.broadcast_to(keep[..., None], r['out32'].shape).copy())
        else:
            parity(f'{tag} out kernel order', r['out32'], r['outplain'], r['out64'])
            parity(f'{tag} duv kernel order', r['duv32'], r['duvplain'], r['duv64'], keep=np.broadcast_to(keep[..., None], r['duv32'].shape).copy())
        keep_tex = np.broadcast_to(r['keep_texels'][..., None], r['dtex32'].shape).copy()
        print(f'{tag}: dtex compared on {int(r["keep_texels"].sum())} of {r["keep_texels"].size} texels')
        parity(f'{tag} dtex kernel order', r['dtex32'], r['dtexplain'], r['dtex64'], keep=keep_tex)


def test_linear_clamp_is_grid_sample():
    for name in ('t5x3_c5_9x7_perview3', 't16_mm8_c3_37x53', 't8x2_c4_9x7_shared3'):
        c = X.case(name)
        r = X.reference(name, X.LINEAR, 'clamp')
        ok = r['px64']['ok']
        tex = torch.tensor(c['tex'], dtype=torch.float64).permute(0, 3, 1, 2).expand(c['B'], -1, -1, -1)
        grid = torch.tensor(np.where(np.isfinite(c['uv']), c['uv'], 0), dtype=torch.float64) * 2 - 1
        want = F.grid_sample(tex, grid, mode='bilinear', padding_mode='border', align_corners=False).permute(0, 2, 3, 1).numpy()
        err = float(np.abs(r['out64'] - want)[ok].max() / np.abs(want).max())
        print(f'{name}: linear + clamp at level 0 against F.grid_sample(bilinear, border) in float64 on {int(ok.sum())} pixels, relative {err:.2e}')
        assert err <= 1e-12
        assert not r['out64'][~ok].any()


def test_mip_chain_is_avg_pool():
    for name in ('t16_mm8_c3_37x53', 't8x2_c4_9x7_shared3', 't16_mm2_c64_9x7', 't5x3_c5_9x7_perview3'):
        c = X.case(name)
        chain = X.mips(c['tex'], c['max_mip_level'], np.float64)
        t = torch.tensor(c['tex'], dtype=torch.float64).permute(0, 3, 1, 2)
        worst = 0.0
        for l in chain[1:]:
            t = F.avg_pool2d(t, 2)
            worst = max(worst, float(np.abs(l - t.permute(0, 2, 3, 1).numpy()).max()))
        chain32 = X.mips(c['tex'], c['max_mip_level'], np.float32)
        err32 = max(float(np.abs(a - b).max()) for a, b in zip(chain32, chain))
        print(f'{name}: {len(chain)} levels, float64 chain against avg_pool2d {worst:.2e}, float32 chain against float64 {err32:.2e}')
        assert worst <= 1e-14 and err32 <= 1e-6 and [l.shape[1:3] for l in chain] == list(zip(*X.levels(c['TH'], c['TW'], c['max_mip_level'])[:2]))


def test_rast_db_is_the_central_difference():
    H, W = 37, 53
    s = X.sphere_scene(H, W, 2)
    face, pos, faces = s['r32']['face'], s['pos'], s['faces']
    db64, db32 = X.rast_db(pos, faces, face, H, W, np.float64), X.rast_db(pos, faces, face, H, W, np.float32)
    same_face = (s['r64']['face'] == face) & s['r64']['decided'] & (face >= 0)
    step = 1e-4                     # pixels: truncation ~ step^2, rounding ~ 1e-16 / step
    cd = np.zeros_like(db64)
    ix, iy = np.meshgrid(np.arange(W), np.arange(H))
    px, py = R.centre(ix, W, np.float64), R.centre(iy, H, np.float64)
    for b in range(pos.shape[0]):
        for f in np.unique(face[b][same_face[b]]):
            m = same_face[b] & (face[b] == f)
            p = pos[b].astype(np.float64)
            for a, (dx, dy) in enumerate(((2 * step / W, 0.0), (0.0, 2 * step / H))):
                up, um = X.bary64(p, faces[f], px[m] + dx, py[m] + dy), X.bary64(p, faces[f], px[m] - dx, py[m] - dy)
                cd[b, ..., a][m] = (up[0] - um[0]) / (2 * step)
                cd[b, ..., 2 + a][m] = (up[1] - um[1]) / (2 * step)
    scale = float(np.abs(db64[same_face]).max())
    err = float(np.abs(db64 - cd)[same_face].max() / scale)
    print(f'rast_db: {int(same_face.sum())} pixels, float64 closed form against central differences relative {err:.2e} (largest value {scale:.3f})')
    assert err <= 1e-6 and int(same_face.sum()) > 500
    assert not db32[face < 0].any() and not db64[face < 0].any()
    # the 10 x rule: the plain float32 baseline is torch autograd in float32 through plain barycentrics (oriented cross products, no
    # named order) with respect to the sample point
    plain = np.zeros_like(db32)
    pt = torch.tensor(np.stack([px, py, np.ones_like(px)], -1), dtype=torch.float32, requires_grad=True)
    for b in range(pos.shape[0]):
        tri = torch.tensor(pos[b][faces[np.maximum(face[b], 0)]][..., [0, 1, 3]], dtype=torch.float32)         # (H,W,3,3)
        lam = [(torch.linalg.cross(tri[..., (k + 1) % 3, :], tri[..., (k + 2) % 3, :]) * pt).sum(-1) for k in range(3)]
        tot = lam[0] + lam[1] + lam[2]
        for i in range(2):
            g, = torch.autograd.grad((lam[i] / tot).sum(), pt, retain_graph=True)
            plain[b, ..., 2 * i], plain[b, ..., 2 * i + 1] = g[..., 0].numpy() * np.float32(2 / W), g[..., 1].numpy() * np.float32(2 / H)
    keep = np.broadcast_to(same_face[..., None], db32.shape).copy()
    parity('rast_db kernel order', db32, plain, db64, keep=keep)
    attr = np.random.default_rng(3).standard_normal((pos.shape[1], 5)).astype(np.float32)
    da64 = X.attr_da(attr, faces, face, db64, [4, 0], np.float64)
    want = np.zeros_like(da64)
    o = R.interp(attr, faces, s['r64']['uv'], face, np.float64)
    # d out / d X by the chain rule through (u, v): the same identity through raster_ref.interp's corner differences
    corner = attr.astype(np.float64)[faces[np.maximum(face, 0)]]
    for k, ch in enumerate((4, 0)):
        for a in range(2):
            want[..., 2 * k + a] = db64[..., a] * (corner[..., 0, ch] - corner[..., 2, ch]) + db64[..., 2 + a] * (corner[..., 1, ch] - corner[..., 2, ch])
    want[face < 0] = 0
    err = float(np.abs(da64 - want).max())
    print(f'attr_da: against the chain rule {err:.2e}; out {o.shape}')
    assert err <= 1e-12


def test_log2_polynomial():
    """the largest error of texture_log2 against float64 log2: every seventh float32 of four binades, and exact powers of two"""
    n, rows = 0, []
    for lo in (0.5, 1.0, 2.0 ** 20, 2.0 ** -20):
        bits = np.arange(np.float32(lo).view(np.uint32), np.float32(2 * lo).view(np.uint32), 7, dtype=np.uint32)
        x = bits.view(np.float32)
        truth = np.log2(x.astype(np.float64))
        err = np.abs(X.log2_poly(x).astype(np.float64) - truth)
        allowed = LOG2_FRACTION_BOUND + 0.5 * np.spacing(np.abs(truth).astype(np.float32)).astype(np.float64)
        n += len(x)
        rows.append((lo, float(err.max()), float(x[int(err.argmax())]), float((err / allowed).max())))
    for lo, worst, where, ratio in rows:
        print(f'texture_log2 on [{lo!r}, {2 * lo!r}): largest |error| against float64 log2 {worst:.3e} at x = {where!r} ({ratio:.2f} of the bound), ')
    print(f'{n} arguments')
    assert all(ratio <= 1.0 for _, _, _, ratio in rows)
    exact = np.array([1.0, 2.0, 4.0, 0.5, 2.0 ** 100, 2.0 ** -126], np.float32)
    assert np.array_equal(X.log2_poly(exact), np.array([0, 1, 2, -1, 100, -126], np.float32))


def _hex(a):
    return ' '.join(f'{v:08x}' for v in np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1).tolist())


@pytest.fixture(scope='module')
def native_exe(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('texture_native') / 'texture_rules_main')
    flags = ['-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    flags += ['-static-libasan'] if os.path.basename(cxx).startswith('g++') else []      # gcc's spelling; clang links its runtime statically already
    r = subprocess.run([cxx] + flags + ['-I', os.path.join(REPO, 'relightableavatar_amd', 'csrc'), os.path.join(REPO, 'tests', 'native', 'texture_rules_main.cpp'),
                                        '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.mark.parametrize('name,filt,bnd', [('t16_mm8_c3_37x53', X.TRILINEAR, 'wrap'), ('t8x2_c4_9x7_shared3', X.TRILINEAR, 'clamp'),
                                           ('t16_boundary_16x24', X.TRILINEAR, 'wrap'), ('t5x3_c5_9x7_perview3', X.LINEAR, 'wrap'),
                                           ('t8x2_runs_7x46', X.NEAREST, 'clamp')])
def test_texture_rules_native(native_exe, tmp_path, name, filt, bnd):
    """tests/native/texture_rules_main.cpp: a stand-alone program (its own main) around csrc/ra_texture_rules.hpp, built with
    -fsanitize=address,undefined and run on the CPU; its levels, log2, lod, taps, weights, outputs and duv equal the float32 restatement
    bit for bit"""
    c, r = X.case(name), X.reference(name, filt, bnd)
    px = r['px32']
    path = str(tmp_path / 'case.txt')
    with open(path, 'w') as fh:
        fh.write(f'{c["Bt"]} {c["TH"]} {c["TW"]} {c["C"]} {c["B"]} {c["H"]} {c["W"]} {X.FILTERS.index(filt)} {X.BOUNDARIES.index(bnd)} {c["max_mip_level"]}\n'
                 f'{_hex(c["tex"])}\n{_hex(c["uv"])}\n{_hex(c["uv_da"])}\n{_hex(c["dout"])}\n')
    run = subprocess.run([native_exe, path], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    u32 = lambda x: f'{int(np.asarray(x, np.float32).view(np.uint32)):08x}'
    hs, ws, off = px['hs'], px['ws'], px['off']
    assert lines[0] == f'levels {len(hs)} ' + ' '.join(f'{h} {w} {o}' for h, w, o in zip(hs, ws, off.tolist()))
    probes = np.array([1.0, 1.41421354, 1.41421366, 2.0, 3.0, 1.17549435e-38, 65536.5, 3.0e38], np.float32)
    assert lines[1:9] == [f'log2 {u32(x)} {u32(y)}' for x, y in zip(probes, X.log2_poly(probes))]
    want = []
    HW = c['H'] * c['W']
    for b in range(c['B']):
        for q in range(HW):
            y, x = divmod(q, c['W'])
            ok = bool(px['ok'][b, y, x])
            row = ['px', str(b), str(q), str(int(ok)), str(int(px['l0'][b, y, x]) if ok else 0), str(int(px['two'][b, y, x])),
                   u32(px['f'][b, y, x] if ok and filt == X.TRILINEAR else 0)]
            if ok and filt == X.NEAREST:
                row.append(str(int(px['gidx'][0, 0, b, y, x])))
            elif ok:
                for k in range(2 if px['two'][b, y, x] else 1):
                    base = int(off[px['lev'][k][b, y, x]])
                    row += [str(int(px['gidx'][k][t, b, y, x]) - base) for t in range(4)] + [u32(px['w'][k][t, b, y, x]) for t in range(4)]
            row += ['out'] + [u32(v) for v in r['out32'][b, y, x]] + ['duv'] + [u32(v) for v in r['duv32'][b, y, x]]
            want.append(' '.join(row))
    got = lines[9:-1]
    differ = [i for i, (a, bb) in enumerate(zip(got, want)) if a != bb]
    print(f'{name} {filt} {bnd}: {lines[-1]}; {len(differ)} of {len(want)} pixel lines differ' + (f'; first:\n{got[differ[0]]}\n{want[differ[0]]}' if differ else ''))
    assert lines[-1] == f'done {c["B"] * HW}'
    assert got == want


def test_python_layer_and_argument_errors():
    import inspect
    import re
    from relightableavatar_amd import _lib, engine, raster_utils
    hdr = open(os.path.join(REPO, 'include', 'relightableavatar.h')).read()
    for sym in ('ra_raster_db', 'ra_interpolate_da', 'ra_texture_mips', 'ra_texture', 'ra_texture_backward', 'ra_texture_tile'):
        assert sym in _lib.SYMBOLS and re.search(r'^int\s+' + sym + r'\s*\(', hdr, flags=re.M), sym
    L = _lib.lib()
    assert L.ra_abi_version() == 9
    assert [L.ra_texture_tile(k) for k in range(3)] == [X.MAX_CHANNELS, X.MAX_LEVELS, 1 << 15]
    assert all(hasattr(engine.Engine, k) for k in ('raster_db', 'interpolate_da', 'texture', 'texture_backward', 'texture_mips'))
    assert all(callable(getattr(raster_utils, k)) for k in ('rasterize_db', 'interpolate_db', 'texture', 'render_textured'))
    assert list(inspect.signature(raster_utils.texture).parameters)[:8] == ['tex', 'uv', 'uv_da', 'mip_level_bias', 'mip', 'filter_mode', 'boundary_mode',
                                                                            'max_mip_level']
    sig = inspect.signature(raster_utils.render_textured)
    assert sig.parameters['antialias'].default is False and list(sig.parameters)[:5] == ['verts', 'faces', 'attrs', 'uv', 'img']
    # the older calls keep their signatures and their refusals
    assert list(inspect.signature(raster_utils.interpolate).parameters) == ['attrs', 'rast', 'faces', 'rast_db', 'diff_attrs', 'engine', 'topology']
    with pytest.raises(NotImplementedError, match='interpolate_db'):
        raster_utils.interpolate(torch.zeros(3, 1), torch.zeros(1, 2, 2, 4), torch.zeros(1, 3, dtype=torch.int32), rast_db=torch.zeros(1, 2, 2, 4))
    with pytest.raises(NotImplementedError, match='render_textured'):
        raster_utils.render_nvdiffrast(torch.zeros(1, 3, 3), torch.zeros(1, 3, dtype=torch.int32), uv=torch.zeros(3, 2), img=torch.zeros(1, 2, 2, 3))
    tex, uv = torch.zeros(1, 4, 4, 3), torch.zeros(1, 2, 2, 2)
    for kw in (dict(filter_mode='linear-mipmap-nearest'), dict(boundary_mode='zero'), dict(boundary_mode='cube'), dict(mip_level_bias=torch.zeros(1, 2, 2)),
               dict(mip=[tex]), dict(filter_mode='cubic')):
        with pytest.raises(NotImplementedError):
            raster_utils.texture(tex, uv, **kw)
    with pytest.raises(ValueError):
        raster_utils.texture(tex[0], uv)
    err = lambda: L.ra_last_error().decode()
    p = C.c_void_p(16)          # never dereferenced: every call below fails on its arguments
    ch = (C.c_int * 2)(0, 1)
    # ra_raster_db(ctx, pos, B, V, faces, F, face, H, W, rast_db, stream)
    for B, H, W, Fn in ((0, 8, 8, 1), (1, -1, 8, 1), (1, 8, 8, 1 << 24), (1, 1 << 15, 1 << 15, 1)):
        assert L.ra_raster_db(None, p, B, 4, p, Fn, p, H, W, p, None) != 0 and 'ra_raster_db: bad sizes' in err(), (B, H, W, Fn)
    assert L.ra_raster_db(None, p, 1, 4, p, 1, p, 8, 8, p, None) != 0 and 'ra_raster_db: null argument' in err()
    # ra_interpolate_da(ctx, attr, per_view, V, A, faces, F, face, rast_db, B, H, W, channels, n, out_da, stream)
    for A, n, B in ((0, 1, 1), (3, 0, 1), (3, 65, 1), (3, 2, 0)):
        assert L.ra_interpolate_da(None, p, 0, 4, A, p, 1, p, p, B, 8, 8, ch, n, p, None) != 0 and 'ra_interpolate_da: bad sizes' in err(), (A, n, B)
    assert L.ra_interpolate_da(None, p, 0, 4, 1, p, 1, p, p, 1, 8, 8, ch, 2, p, None) != 0 and 'a selected channel outside' in err()
    assert L.ra_interpolate_da(None, p, 0, 4, 3, p, 1, p, p, 1, 8, 8, ch, 2, p, None) != 0 and 'ra_interpolate_da: null argument' in err()
    # ra_texture_mips(ctx, tex, Bt, TH, TW, C, max_mip_level, mips, lmax, offsets, stream): the sizes alone need neither a ctx nor a texture
    lmax, off = C.c_int(-1), (C.c_longlong * 17)()
    assert L.ra_texture_mips(None, None, 1, 8, 2, 3, 8, None, C.byref(lmax), off, None) == 0 and lmax.value == 1 and list(off)[:3] == [0, 16, 20]
    assert L.ra_texture_mips(None, None, 1, 16, 16, 3, 2, None, C.byref(lmax), off, None) == 0 and lmax.value == 2
    assert L.ra_texture_mips(None, None, 1, 5, 3, 3, 8, None, C.byref(lmax), off, None) == 0 and lmax.value == 0
    for Bt, TH, Cn, mm in ((0, 8, 3, 8), (1, 0, 3, 8), (1, (1 << 15) + 1, 3, 8), (1, 8, 0, 8), (1, 8, 65, 8), (1, 8, 3, -1)):
        assert L.ra_texture_mips(None, p, Bt, TH, 8, Cn, mm, p, C.byref(lmax), off, None) != 0 and 'ra_texture_mips: bad sizes' in err(), (Bt, TH, Cn, mm)
    assert L.ra_texture_mips(None, p, 1, 8, 8, 3, 8, p, C.byref(lmax), off, None) != 0 and 'ra_texture_mips: null argument' in err()
    # ra_texture(ctx, tex, Bt, TH, TW, C, uv, uv_da, B, H, W, filter, boundary, max_mip_level, out, stream) and its backward
    fwd = lambda Bt, TH, Cn, B, H, flt, bnd, mm: L.ra_texture(None, p, Bt, TH, 8, Cn, p, p, B, H, 8, flt, bnd, mm, p, None)
    bwd = lambda Bt, TH, Cn, B, H, flt, bnd, mm: L.ra_texture_backward(None, p, Bt, TH, 8, Cn, p, p, B, H, 8, flt, bnd, mm, p, p, p, None)
    for args in ((2, 8, 3, 3, 8, 1, 0, 8), (1, 0, 3, 1, 8, 1, 0, 8), (1, 8, 65, 1, 8, 1, 0, 8), (1, 8, 3, 0, 8, 1, 0, 8), (1, 8, 3, 1, 8, 1, 0, -1),
                 (1, 8, 64, 1, 1 << 23, 1, 0, 8)):
        assert fwd(*args) != 0 and 'ra_texture: bad sizes' in err(), args
        assert bwd(*args) != 0 and 'ra_texture_backward: bad sizes' in err(), args
    # the tap-count limit of dtex: 2^25 x 8 pixels x 8 taps = 2^31
    assert bwd(1, 8, 1, 1, 1 << 25, 2, 0, 8) != 0 and 'ra_texture_backward: bad sizes' in err() and 'taps' in err()
    for flt, bnd in ((3, 0), (-1, 0), (1, 2), (1, -1)):
        assert fwd(1, 8, 3, 1, 8, flt, bnd, 8) != 0 and 'ra_texture: unknown mode' in err()
        assert bwd(1, 8, 3, 1, 8, flt, bnd, 8) != 0 and 'ra_texture_backward: unknown mode' in err()
    assert fwd(1, 8, 3, 1, 8, 2, 1, 8) != 0 and 'ra_texture: null argument' in err()
    assert bwd(1, 8, 3, 1, 8, 2, 1, 8) != 0 and 'ra_texture_backward: null argument' in err()

"""The texture path on the device: ra_raster_db, ra_interpolate_da, ra_texture_mips, ra_texture and
ra_texture_backward.  Run with `-m gpu` on an MI355X.

Exactness is bit equality: rast_db, out_da, the mip chain, out in all three filter modes and both boundary modes, duv and dtex equal the
kernel-order numpy restatement (tests/texture_ref.py); a repeat gives the same bits; a view of a batch equals the call of that view alone;
the halves of `want` equal the full call.  By value the outputs are held to the project's 10 x float32 rule (frame_stage_ref.parity)
against float64, duv on the decided pixels and dtex on the texels no undecided pixel reaches.  Every test prints its figures before it
asserts."""
import numpy as np
import pytest
import torch

import texture_ref as X
from frame_stage_ref import parity
from relightableavatar_amd import raster_utils
from relightableavatar_amd.base_utils import dotdict
from relightableavatar_amd.config import make_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MODES = [(f, b) for f in X.FILTERS for b in X.BOUNDARIES]


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from relightableavatar_amd.engine import Engine
    return Engine(make_cfg('relight'), device=DEV)          # any context will do: no weights are read


def T(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)          # a copy: the shared references are read-only


def bits(t):
    t = torch.as_tensor(t).cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(tag, got, want, quiet=False):
    x, y = bits(got), bits(torch.as_tensor(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want)
    ok = x.shape == y.shape and bool(torch.equal(x, y))
    if not quiet or not ok:
        print(f'{tag}: bit-equal {ok} ({x.numel()} values, {int((x != y).sum()) if x.shape == y.shape else -1} differ)')
    assert ok, tag


def run(eng, c, filt, bnd, views=slice(None), tex_views=slice(None), **kw):
    tex, uv, da, dout = T(c['tex'][tex_views]), T(c['uv'][views]), T(c['uv_da'][views]), T(c['dout'][views])
    mm = c['max_mip_level']
    return eng.texture(tex, uv, da, filt, bnd, mm), eng.texture_backward(tex, uv, dout, da, filt, bnd, mm, **kw)


@pytest.mark.parametrize('name', X.CASES)
def test_bits(eng, name):
    """out, duv and dtex in the three filter modes and both boundary modes, and the mip chain, equal the float32 restatement in kernel order
    and themselves on a repeat; the halves of `want` equal the full call; a non-finite uv gives 0 and no gradient"""
    c = X.case(name)
    chain = eng.texture_mips(T(c['tex']), c['max_mip_level'])
    want_chain = X.mips(c['tex'], c['max_mip_level'], np.float32)
    assert len(chain) == len(want_chain) == c['Lmax'] + 1
    for l, (got, want) in enumerate(zip(chain, want_chain)):
        same(f'{name} mip level {l} {tuple(want.shape[1:3])}', got, want)
    bad = ~np.isfinite(c['uv']).all(-1)
    for filt, bnd in MODES:
        r = X.reference(name, filt, bnd)
        tag = f'{name} {filt} {bnd}'
        runs = r['runs']
        print(f'{tag}: {len(runs)} runs, longest {int(runs.max()) if len(runs) else 0}')
        out, g = run(eng, c, filt, bnd)
        same(f'{tag} out', out, r['out32'])
        same(f'{tag} duv', g.duv, r['duv32'])
        same(f'{tag} dtex', g.dtex, r['dtex32'])
        out2, g2 = run(eng, c, filt, bnd)
        same(f'{tag} out, repeat', out2, out, quiet=True)
        same(f'{tag} duv, repeat', g2.duv, g.duv, quiet=True)
        same(f'{tag} dtex, repeat', g2.dtex, g.dtex, quiet=True)
        _, only_u = run(eng, c, filt, bnd, want=('duv',))
        _, only_t = run(eng, c, filt, bnd, want=('dtex',))
        assert set(only_u) == {'duv'} and set(only_t) == {'dtex'}
        same(f'{tag} duv alone', only_u.duv, g.duv, quiet=True)
        same(f'{tag} dtex alone', only_t.dtex, g.dtex, quiet=True)
        if bad.any():
            assert not bool(out.cpu()[torch.as_tensor(bad)].any()) and not bool(g.duv.cpu()[torch.as_tensor(bad)].any())
    if c['kind'] == 'runs':
        assert np.sort(X.reference(name, X.NEAREST, 'wrap')['runs']).tolist() == list(X.RUN_LENGTHS)
    if c['kind'] == 'magnify':
        assert int(X.reference(name, X.LINEAR, 'wrap')['runs'].max()) > 1000


def test_non_finite_uv(eng):
    """an image of non-finite uv alone: the output and both gradients are 0"""
    c = X.case('t16_mm8_c3_37x53')
    uv = T(c['uv'][:, :3, :4]).clone()
    uv[..., 0], uv[0, 0, 0, 0], uv[0, 1, 1, 1] = float('nan'), float('inf'), float('-inf')
    da, dout, tex = T(c['uv_da'][:, :3, :4]), T(c['dout'][:, :3, :4]), T(c['tex'])
    for filt, bnd in MODES:
        out = eng.texture(tex, uv, da, filt, bnd, 8)
        g = eng.texture_backward(tex, uv, dout, da, filt, bnd, 8)
        assert not bool(out.any()) and not bool(g.duv.any()) and not bool(g.dtex.any()), (filt, bnd)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g.dtex).all())


@pytest.mark.parametrize('name', ['t8x2_c4_9x7_shared3', 't5x3_c5_9x7_perview3', 't16_mm8_c3_37x53_perview2'])
def test_view_independence(eng, name):
    """row b of out, of duv and of a per-view dtex equals the one-view call; a shared texture's dtex is the views' results added in
    ascending order"""
    c = X.case(name)
    for filt, bnd in ((X.TRILINEAR, 'wrap'), (X.LINEAR, 'clamp'), (X.NEAREST, 'wrap')):
        out, g = run(eng, c, filt, bnd)
        total = None
        for b in range(c['B']):
            tv = slice(0, 1) if c['Bt'] == 1 else slice(b, b + 1)
            o1, g1 = run(eng, c, filt, bnd, views=slice(b, b + 1), tex_views=tv)
            same(f'{name} {filt} view {b} out', out[b:b + 1], o1, quiet=True)
            same(f'{name} {filt} view {b} duv', g.duv[b:b + 1], g1.duv, quiet=True)
            if c['Bt'] != 1:
                same(f'{name} {filt} view {b} dtex', g.dtex[b:b + 1], g1.dtex, quiet=True)
            total = g1.dtex if total is None else total + g1.dtex
        if c['Bt'] == 1:
            same(f'{name} {filt} shared dtex = the views added in ascending order', g.dtex, total)
        assert bool(g.dtex.any())


def test_stale_scratch(eng):
    """the smallest case before and after the largest in one ctx gives the same bits: nothing is read from what an earlier call left"""
    small, big = X.case('t1x1_c1_1x1'), X.case('t2x2_magnify_64x64')
    out_a, g_a = run(eng, small, X.TRILINEAR, 'wrap')
    out_b, g_b = run(eng, big, X.TRILINEAR, 'wrap')
    same('64 x 64 dtex', g_b.dtex, X.reference('t2x2_magnify_64x64', X.TRILINEAR, 'wrap')['dtex32'])
    wide = X.case('t16_mm2_c64_9x7')
    run(eng, wide, X.TRILINEAR, 'clamp')
    out_c, g_c = run(eng, small, X.TRILINEAR, 'wrap')
    same('small out after large', out_c, out_a)
    same('small duv after large', g_c.duv, g_a.duv)
    same('small dtex after large', g_c.dtex, g_a.dtex)
    same('small dtex against the restatement', g_c.dtex, X.reference('t1x1_c1_1x1', X.TRILINEAR, 'wrap')['dtex32'])


@pytest.mark.parametrize('H,W,views', [(37, 53, 2), (9, 7, 2), (1, 1, 1)])
def test_differentials_bits(eng, H, W, views):
    """rast_db and out_da equal the restatement bit for bit on ra_rasterize's own maps; rasterize_db and interpolate_db return the bits of
    rasterize and interpolate in their first outputs"""
    s = X.sphere_scene(H, W, views)
    pos, faces = T(s['pos']), T(s['faces'])
    face = s['r32']['face']
    rast = raster_utils.rasterize(pos, faces, H, W, engine=eng)
    rast2, db = raster_utils.rasterize_db(pos, faces, H, W, engine=eng)
    same(f'{H} x {W} rasterize_db rast', rast2, rast)
    same(f'{H} x {W} face map', (rast[..., 3] - 1).int(), face)
    want_db = X.rast_db(s['pos'], s['faces'], face, H, W, np.float32)
    print(f'{H} x {W}: {int((face >= 0).sum())} covered pixels of {face.size}')
    same(f'{H} x {W} rast_db', db, want_db)
    same(f'{H} x {W} rast_db, repeat', eng.raster_db(pos, faces, dotdict(face=T(face))), db)
    assert not db.requires_grad and not bool(db.cpu()[torch.as_tensor(face < 0)].any())
    rng = np.random.default_rng(7)
    for kind, attr in (('shared', rng.standard_normal((s['pos'].shape[1], 5)).astype(np.float32)),
                       ('per view', rng.standard_normal((views, s['pos'].shape[1], 5)).astype(np.float32))):
        for channels in ([3, 4], [0], 'all'):
            ch = list(range(5)) if channels == 'all' else channels
            out, da = raster_utils.interpolate_db(T(attr), rast, faces, db, channels, engine=eng)
            same(f'{H} x {W} {kind} interpolate_db out {channels}', out, raster_utils.interpolate(T(attr), rast, faces, engine=eng), quiet=True)
            same(f'{H} x {W} {kind} out_da {channels}', da, X.attr_da(attr, s['faces'], face, want_db, ch, np.float32))
            assert da.shape == (views, H, W, 2 * len(ch)) and not da.requires_grad
    wide = rng.standard_normal((s['pos'].shape[1], 70)).astype(np.float32)
    ch = list(range(69, 5, -1))          # 64 channels, descending
    same(f'{H} x {W} out_da of 64 channels of 70', eng.interpolate_da(T(wide), dotdict(face=T(face)), faces, db, ch),
         X.attr_da(wide, s['faces'], face, want_db, ch, np.float32))


def test_differentials_gradients(eng):
    """rasterize_db's rast and interpolate_db's out carry rasterize's and interpolate's backward"""
    s = X.sphere_scene(9, 7, 2)
    faces = T(s['faces'])
    attr = T(np.random.default_rng(5).standard_normal((s['pos'].shape[1], 3)).astype(np.float32))
    w = T(np.random.default_rng(6).standard_normal((2, 9, 7, 3)).astype(np.float32))
    grads = []
    for db_path in (False, True):
        pos, a = T(s['pos']).requires_grad_(True), attr.clone().requires_grad_(True)
        if db_path:
            rast, db = raster_utils.rasterize_db(pos, faces, 9, 7, engine=eng)
            out, _ = raster_utils.interpolate_db(a, rast, faces, db, 'all', engine=eng)
        else:
            out = raster_utils.interpolate(a, raster_utils.rasterize(pos, faces, 9, 7, engine=eng), faces, engine=eng)
        (out * w).sum().backward()
        grads.append((pos.grad.clone(), a.grad.clone()))
    same('pos.grad through rasterize_db / interpolate_db', grads[1][0], grads[0][0])
    same('attrs.grad through interpolate_db', grads[1][1], grads[0][1])
    assert bool(grads[0][0].any())


@pytest.mark.parametrize('name', X.BY_VALUE)
def test_by_value(eng, name):
    """the 10 x float32 rule against float64: out of the linear modes on every pixel, duv and the nearest output on the decided pixels, dtex
    on the texels no undecided pixel reaches"""
    c = X.case(name)
    for filt, bnd in MODES:
        r = X.reference(name, filt, bnd)
        tag = f'{name} {filt} {bnd}'
        und = r['undecided']
        print(f'{tag}: undecided {int(und.sum())} of {und.size} pixels ({float(und.mean()):.2%}), dtex on {int(r["keep_texels"].sum())} of {r["keep_texels"].size} texels')
        assert float(und.mean()) <= X.UNDECIDED_CAP
        out, g = run(eng, c, filt, bnd)
        keep = ~und
        if filt == X.NEAREST:
            parity(f'{tag} out', out, r['outplain'], r['out64'], keep=np.broadcast_to(keep[..., None], r['out32'].shape).copy())
        else:
            parity(f'{tag} out', out, r['outplain'], r['out64'])
            parity(f'{tag} duv', g.duv, r['duvplain'], r['duv64'], keep=np.broadcast_to(keep[..., None], r['duv32'].shape).copy())
        parity(f'{tag} dtex', g.dtex, r['dtexplain'], r['dtex64'], keep=np.broadcast_to(r['keep_texels'][..., None], r['dtex32'].shape).copy())


def test_autograd_op(eng):
    """raster_utils.texture: the op's gradients are texture_backward's, 'auto' picks the mode by uv_da, and a (TH,TW,C) call of the Engine
    returns a (TH,TW,C) dtex"""
    c = X.case('t16_mm8_c3_37x53')
    r = X.reference('t16_mm8_c3_37x53', X.TRILINEAR, 'wrap')
    tex, uv = T(c['tex']).requires_grad_(True), T(c['uv']).requires_grad_(True)
    da = T(c['uv_da']).requires_grad_(True)
    out = raster_utils.texture(tex, uv, da, max_mip_level=8, engine=eng)
    same('texture(auto, uv_da) = linear-mipmap-linear', out, r['out32'])
    (out * T(c['dout'])).sum().backward()
    same('tex.grad', tex.grad, r['dtex32'])
    same('uv.grad', uv.grad, r['duv32'])
    assert da.grad is None
    lin = raster_utils.texture(T(c['tex']), T(c['uv']), engine=eng)
    same('texture(auto) = linear', lin, X.reference('t16_mm8_c3_37x53', X.LINEAR, 'wrap')['out32'])
    g = eng.texture_backward(T(c['tex'])[0], T(c['uv']), T(c['dout']), T(c['uv_da']), max_mip_level=8)
    same('dtex of a (TH,TW,C) texture', g.dtex, r['dtex32'][0])
    with pytest.raises(Exception, match='bad sizes'):
        eng.texture(torch.zeros(1, 4, 4, X.MAX_CHANNELS + 1, device=DEV), torch.zeros(1, 2, 2, 2, device=DEV), None, 'linear')
    with pytest.raises(ValueError):
        eng.texture(torch.zeros(2, 4, 4, 3, device=DEV), torch.zeros(3, 2, 2, 2, device=DEV), None, 'linear')


@pytest.mark.parametrize('H,W,R_S', [(37, 53, 1), (20, 26, 2)])
def test_render_textured_by_value(eng, H, W, R_S):
    """render_textured on two views of the sphere against the float64 pipeline under the 10 x rule, on the output pixels all of whose
    source pixels are decided; at most 1 % are left out"""
    r = X.render_reference(H, W, R_S)
    RH, RW = H * R_S, W * R_S
    eye = torch.eye(4, device=DEV)[None]
    img, msk = raster_utils.render_textured(T(r['pos']), T(r['faces']), uv=T(r['uv_vert']), img=T(r['img']), H=H, W=W, K=eye, R_S=R_S, engine=eng)
    assert img.shape == (2, H, W, 3) and msk.shape == (2, H, W)
    resize = lambda a: raster_utils.bilinear_interpolation(torch.tensor(np.ascontiguousarray(a)), [H, W]).numpy()
    full64, full32 = resize(r['full64']), resize(r['full32'].astype(np.float32))
    decided = torch.tensor(r['decided'].copy()).view(2, H, R_S, W, R_S).permute(0, 1, 3, 2, 4).reshape(2, H, W, -1).all(-1).numpy()
    left_out = 1.0 - float(decided.mean())
    print(f'{H} x {W} R_S {R_S}: rasterised at {RH} x {RW}, {int(r["decided"].sum())} of {r["decided"].size} source pixels decided, '
          f'{left_out:.2%} of the output pixels left out, mask covers {float(full64[..., -1].mean()):.1%}')
    assert left_out <= 0.01
    got = torch.cat([img, msk[..., None]], -1)
    parity(f'render_textured {H} x {W} R_S {R_S}', got, full32, full64, keep=np.broadcast_to(decided[..., None], full64.shape).copy())
    assert not bool(img.cpu()[torch.as_tensor(full64[..., -1] == 0)].any())
    # with attributes: the attribute maps are render_nvdiffrast's, the image is the texture-only call's
    attrs = T(np.random.default_rng(9).standard_normal((r['pos'].shape[1], 2)).astype(np.float32))
    a3, img3, msk3 = raster_utils.render_textured(T(r['pos']), T(r['faces']), attrs, T(r['uv_vert']), T(r['img']), H=H, W=W, K=eye, R_S=R_S, engine=eng)
    a2, msk2 = raster_utils.render_nvdiffrast(T(r['pos']), T(r['faces']), attrs, H=H, W=W, K=eye, R_S=R_S, engine=eng)
    same('render_textured attributes = render_nvdiffrast', a3, a2)
    same('render_textured mask = render_nvdiffrast', msk3, msk2)
    same('render_textured image with attributes = without', img3, img)


def test_end_to_end_fit(eng):
    """a 16 x 16 texture recovered from two renderings of the sphere by plain gradient descent through raster_utils.texture: the loss falls by
    at least half the factor the same loop reaches in float64 torch on the CPU (tests/texture_ref.py fit_float64; both in DESIGN.md)"""
    fi = X.fit_inputs()
    ref = X.fit_float64()
    uv, da, mask = T(fi['uv']), T(fi['uv_da']), T(fi['mask'])[..., None]
    target = raster_utils.texture(T(fi['tex']), uv, da, max_mip_level=8, engine=eng)
    t = torch.full(fi['tex'].shape, 0.5, device=DEV, requires_grad=True)
    losses = []
    for _ in range(X.FIT_STEPS + 1):
        loss = (((raster_utils.texture(t, uv, da, max_mip_level=8, engine=eng) - target) * mask) ** 2).sum()
        losses.append(float(loss.detach()))
        g, = torch.autograd.grad(loss, t)
        with torch.no_grad():
            t -= X.FIT_LR * g
    factor, factor64 = losses[0] / losses[-1], ref[0] / ref[-1]
    print(f'fit: {X.FIT_STEPS} steps of {X.FIT_LR}: loss {losses[0]:.4f} -> {losses[-1]:.4f} (factor {factor:.2f}); float64 on the CPU {ref[0]:.4f} -> {ref[-1]:.4f} '
          f'(factor {factor64:.2f}); largest |t - true| {float((t.detach() - T(fi["tex"])).abs().max()):.3f}')
    assert abs(losses[0] - ref[0]) <= 1e-3 * ref[0]          # one float32 sum of 4 600 squares against float64: n eps = 3e-4 at the worst
    assert factor >= 0.5 * factor64

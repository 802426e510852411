"""ra_antialias and ra_antialias_backward on the device.  Run with `-m gpu` on an MI355X.

Exactness is bit equality: the forward, dcolor and dpos equal the kernel-order numpy restatement (tests/antialias_ref.py) on the float32
maps of raster_ref (what ra_rasterize returns bit for bit), a repeat gives the same bits, a view of a batch equals the call of that view
alone, the halves of `want` equal the full call, and pos_gradient_boost is one float32 product on dpos.  By value the three outputs are held
to the project's 10 x float32 rule (frame_stage_ref.parity) against torch autograd in float64 with the float64 pair set held fixed, on
the pixels and vertices no undecided pair touches, in the cases with at least 100 active pairs.  Every test prints its figures before it
asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import antialias_ref as A
import raster_ref as R
from frame_stage_ref import parity
from relightableavatar_amd import largesteps, raster_utils
from relightableavatar_amd.base_utils import dotdict
from relightableavatar_amd.config import make_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BY_VALUE = ('two_triangles_32x32', 'open_37x53', 'sphere2_136x200', 'tri012_130x70')


def make_engine():
    from relightableavatar_amd.engine import Engine
    return Engine(make_cfg('relight'), device=DEV)          # any context will do: no weights are read


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return make_engine()


def T(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)          # a copy: the shared references are read-only


def bits(t):
    t = torch.as_tensor(t).cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(tag, got, want):
    x, y = bits(got), bits(torch.as_tensor(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want)
    ok = x.shape == y.shape and bool(torch.equal(x, y))
    print(f'{tag}: bit-equal {ok} ({x.numel()} values, {int((x != y).sum()) if x.shape == y.shape else -1} differ)')
    assert ok, tag


def device_case(eng, name, views=slice(None)):
    c = A.case(name)
    pos = T(c['pos'][views])
    return c, pos, T(c['faces']), dotdict(zw=T(c['zw'][views]), face=T(c['face'][views])), eng.topology(T(c['faces']), c['pos'].shape[1])


def run(eng, topo, color, rast, pos, dout, **kw):
    return eng.antialias(topo, color, rast, pos), eng.antialias_backward(topo, color, rast, pos, dout, **kw)


@pytest.mark.parametrize('name,Cn', A.PARAMS)
def test_bits(eng, name, Cn):
    """forward, dcolor and dpos equal the float32 restatement in kernel order and themselves on a repeat; the halves of `want` equal the
    full call; pos_gradient_boost = 3 is the float32 product on dpos and leaves dcolor alone"""
    c, pos, faces, rast, topo = device_case(eng, name)
    ref = A.reference(name, Cn)
    n = A.counts(c)
    print(f'{name} C={Cn}: {n["active32"]} active pairs of {n["candidates"]}')
    color, dout = T(ref['color']), T(ref['dout'])
    out, g = run(eng, topo, color, rast, pos, dout)
    same(f'{name} C={Cn} out', out, ref['out'])
    same(f'{name} C={Cn} dcolor', g.dcolor, ref['kernel']['dcolor'])
    same(f'{name} C={Cn} dpos', g.dpos, ref['kernel']['dpos'])
    out2, g2 = run(eng, topo, color, rast, pos, dout)
    same(f'{name} C={Cn} out, repeat', out2, out)
    same(f'{name} C={Cn} dcolor, repeat', g2.dcolor, g.dcolor)
    same(f'{name} C={Cn} dpos, repeat', g2.dpos, g.dpos)
    only_c = eng.antialias_backward(topo, color, rast, pos, dout, want=('dcolor',))
    only_p = eng.antialias_backward(topo, color, rast, pos, dout, want=('dpos',))
    assert set(only_c) == {'dcolor'} and set(only_p) == {'dpos'}
    same(f'{name} C={Cn} dcolor alone', only_c.dcolor, g.dcolor)
    same(f'{name} C={Cn} dpos alone', only_p.dpos, g.dpos)
    g3 = eng.antialias_backward(topo, color, rast, pos, dout, pos_gradient_boost=3.0)
    same(f'{name} C={Cn} dpos, boost 3', g3.dpos, ref['kernel3']['dpos'])
    same(f'{name} C={Cn} dpos, boost 3 = 3 dpos', g3.dpos, (g.dpos * 3.0))
    same(f'{name} C={Cn} dcolor, boost 3', g3.dcolor, g.dcolor)
    if name in ('sphere_1x1', 'empty_8x8'):
        same(f'{name} out = color', out, color)
        same(f'{name} dcolor = dout', g.dcolor, dout)
        assert not bool(g.dpos.any())
    topo.close()


def test_device_maps_are_the_restated_ones(eng):
    """the maps the cases feed to ra_antialias are ra_rasterize's own, bit for bit"""
    for name in ('two_triangles_32x32', 'open_37x53', 'degenerate_32x32'):
        c = A.case(name)
        got = eng.rasterize(T(c['pos']), T(c['faces']), c['H'], c['W'])
        same(f'{name} face', got.face, c['face'])
        same(f'{name} zw', got.zw, c['zw'])


def test_view_independence(eng):
    """row b of a three-view call equals the one-view call, bit for bit"""
    c2 = A.case('sphere2_136x200')
    H, W = c2['H'], c2['W']
    ref = R.sphere_reference(H, W, 2)
    idx = [0, 1, 0]
    pos, face, zw = ref['pos'][idx], ref['r32']['face'][idx], ref['r32']['zw'][idx].astype(np.float32)
    rng = np.random.default_rng(11)
    color, dout = rng.standard_normal((3, H, W, 4)).astype(np.float32), rng.standard_normal((3, H, W, 4)).astype(np.float32)
    topo = eng.topology(T(ref['faces']), pos.shape[1])
    rast = dotdict(zw=T(zw), face=T(face))
    out, g = run(eng, topo, T(color), rast, T(pos), T(dout))
    for b in range(3):
        r1 = dotdict(zw=T(zw[b:b + 1]), face=T(face[b:b + 1]))
        o1, g1 = run(eng, topo, T(color[b:b + 1]), r1, T(pos[b:b + 1]), T(dout[b:b + 1]))
        same(f'view {b} out', out[b:b + 1], o1)
        same(f'view {b} dcolor', g.dcolor[b:b + 1], g1.dcolor)
        same(f'view {b} dpos', g.dpos[b:b + 1], g1.dpos)
    assert bool(g.dpos.any())
    topo.close()


def test_stale_scratch(eng):
    """a small case before and after the 130 x 70 case in one ctx gives the same bits: nothing is read from what an earlier call left"""
    def small():
        c, pos, faces, rast, topo = device_case(eng, 'two_triangles_32x32')
        ref = A.reference('two_triangles_32x32', 4)
        out, g = run(eng, topo, T(ref['color']), rast, pos, T(ref['dout']))
        topo.close()
        return out, g, ref
    out_a, g_a, ref = small()
    c, pos, faces, rast, topo = device_case(eng, 'tri012_130x70')
    big = A.reference('tri012_130x70', 4)
    out_b, g_b = run(eng, topo, T(big['color']), rast, pos, T(big['dout']))
    same('130 x 70 dpos', g_b.dpos, big['kernel']['dpos'])
    topo.close()
    out_c, g_c, _ = small()
    same('small out after large', out_c, out_a)
    same('small dcolor after large', g_c.dcolor, g_a.dcolor)
    same('small dpos after large', g_c.dpos, g_a.dpos)
    same('small dpos against the restatement', g_c.dpos, ref['kernel']['dpos'])


def test_foreign_topology_and_sizes(eng):
    other = make_engine()
    c, pos, faces, rast, topo = device_case(eng, 'tri012_32x32')
    foreign = other.topology(faces, c['pos'].shape[1])
    ref = A.reference('tri012_32x32', 4)
    color, dout = T(ref['color']), T(ref['dout'])
    with pytest.raises(Exception, match='not a topology of this ctx'):
        eng.antialias(foreign, color, rast, pos)
    with pytest.raises(Exception, match='not a topology of this ctx'):
        eng.antialias_backward(foreign, color, rast, pos, dout)
    with pytest.raises(Exception, match='bad sizes'):
        eng.antialias(topo, color, rast, torch.cat([pos, pos], 1))          # not the topology's vertex count
    with pytest.raises(ValueError):
        eng.antialias(topo, color[..., 0], rast, pos)
    # a face id outside the topology's range makes its pairs inert
    wild = dotdict(zw=rast.zw, face=torch.where(rast.face >= 0, torch.full_like(rast.face, 7), rast.face))
    out = eng.antialias(topo, color, wild, pos)
    same('face ids outside [0, F): out = color', out, color)
    g = eng.antialias_backward(topo, color, wild, pos, dout)
    same('face ids outside [0, F): dcolor = dout', g.dcolor, dout)
    assert not bool(g.dpos.any())
    foreign.close()
    topo.close()


@pytest.mark.parametrize('name', BY_VALUE)
def test_by_value(eng, name):
    """the 10 x float32 rule against float64 autograd, on the pixels and vertices no undecided pair touches"""
    c, pos, faces, rast, topo = device_case(eng, name)
    ref = A.reference(name, 4)
    n = A.counts(c)
    share = n['undecided'] / max(n['candidates'], 1)
    print(f'{name}: {n["active64"]} active pairs in float64, undecided {n["undecided"]} of {n["candidates"]} ({share:.2%})')
    assert n['active64'] >= A.MIN_ACTIVE and share <= A.UNDECIDED_CAP
    out, g = run(eng, topo, T(ref['color']), rast, pos, T(ref['dout']))
    keep_pix = np.broadcast_to(ref['keep_pix'][..., None], ref['out'].shape).copy()
    keep_vert = np.broadcast_to(ref['keep_vert'][..., None], ref['kernel']['dpos'].shape).copy()
    t32, t64 = ref['t32'], ref['t64']
    parity(f'{name} out', out, t32['out'], t64['out'], keep=keep_pix)
    parity(f'{name} dcolor', g.dcolor, t32['dcolor'], t64['dcolor'], keep=keep_pix)
    assert keep_pix.any()
    if name == 'tri012_130x70':         # all three vertices touch an undecided pair: dpos of the long runs is pinned by bit equality (test_bits) alone
        assert not keep_vert.any()
    else:
        assert keep_vert.any()
        parity(f'{name} dpos', g.dpos, t32['dpos'], t64['dpos'], keep=keep_vert)
    topo.close()


def _triangle_scene(H=32, W=32):
    verts = torch.tensor([[-0.45, -0.4, 0.0], [0.5, -0.3, 0.0], [0.0, 0.5, 0.0], [0.3, 0.3, 0.0], [-0.2, 0.1, 0.5]], device=DEV)       # two vertices no face uses
    faces = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=DEV)
    Rt = torch.eye(3, device=DEV)[None]
    Tt = torch.tensor([[[0.0], [0.0], [2.0]]], device=DEV)
    K = torch.tensor([[1.6 * W / 2, 0, W / 2], [0, 1.6 * W / 2, H / 2], [0, 0, 1]], device=DEV)
    return verts, faces, Rt, Tt, raster_utils.get_ndc_perspective_matrix(K[None], H, W)


def test_end_to_end(eng):
    """render_nvdiffrast(antialias=True, R_S=1): a fractional mask on the outline whose loss reaches the vertices; antialias=False gives
    none — the gap this closes; 20 AdamUniform steps on a translated triangle lower the mask loss"""
    H = W = 32
    verts, faces, Rt, Tt, P = _triangle_scene(H, W)
    topo = eng.topology(faces, verts.shape[0])
    attrs = torch.ones(verts.shape[0], 1, device=DEV)
    render = lambda v, aa: raster_utils.render_nvdiffrast(v, faces, attrs, H=H, W=W, R=Rt, T=Tt, K=P, R_S=1, engine=eng, topology=topo, antialias=aa)[1]
    target = render(verts, True).detach()
    frac = (target > 0) & (target < 1)
    plain = render(verts, False)
    print(f'mask: {int((plain > 0).sum())} covered pixels, {int(frac.sum())} fractional values with antialias=True, '
          f'{int(((plain > 0) & (plain < 1)).sum())} without')
    assert int(frac.sum()) > 10 and not bool(((plain > 0) & (plain < 1)).any())
    assert float(target.min()) >= 0 and float(target.max()) <= 1
    moved = verts.clone()
    moved[:3, :2] += torch.tensor([0.06, -0.04], device=DEV)
    grads = {}
    for aa in (True, False):
        p = moved.clone().requires_grad_(True)
        loss = ((render(p, aa) - target) ** 2).sum()
        loss.backward()
        grads[aa] = p.grad.clone()
        print(f'antialias={aa}: loss {float(loss):.4f}, max |verts.grad| {float(p.grad.abs().max()):.4e}')
    assert bool(grads[True][:3].any()) and not bool(grads[True][3:].any()) and bool(torch.isfinite(grads[True]).all())
    assert not bool(grads[False].any())
    # pos_gradient_boost scales the gradient that reaches the vertices through the positions
    p = moved.clone().requires_grad_(True)
    m = raster_utils.render_nvdiffrast(p, faces, attrs, H=H, W=W, R=Rt, T=Tt, K=P, R_S=1, engine=eng, topology=topo, antialias=True, pos_gradient_boost=2.0)[1]
    ((m - target) ** 2).sum().backward()
    assert torch.allclose(p.grad, 2 * grads[True], rtol=1e-5, atol=1e-12)
    # without a topology the op builds its own
    p = moved.clone().requires_grad_(True)
    m = raster_utils.render_nvdiffrast(p, faces, attrs, H=H, W=W, R=Rt, T=Tt, K=P, R_S=1, engine=eng, antialias=True)[1]
    ((m - target) ** 2).sum().backward()
    same('verts.grad with a topology of the op', p.grad, grads[True])
    param = moved.clone().requires_grad_(True)
    opt = largesteps.AdamUniform([param], lr=5e-3, engine=eng)
    losses = []
    for _ in range(21):
        opt.zero_grad()
        loss = ((render(param, True) - target) ** 2).sum()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print(f'fit: loss {losses[0]:.4f} -> {losses[-1]:.4f}')
    assert losses[-1] < losses[0]
    topo.close()


def test_images_without_pixels(eng):
    """H = 0: nothing is launched, the outputs are empty and dpos is zero (the C entry points take the null pointers of empty tensors)"""
    c, pos, faces, rast, topo = device_case(eng, 'tri012_32x32')
    color = torch.zeros(1, 0, 5, 4, device=DEV)
    empty = dotdict(zw=torch.zeros(1, 0, 5, device=DEV), face=torch.zeros(1, 0, 5, dtype=torch.int32, device=DEV))
    assert eng.antialias(topo, color, empty, pos).shape == (1, 0, 5, 4)
    g = eng.antialias_backward(topo, color, empty, pos, color)
    assert g.dcolor.shape == (1, 0, 5, 4) and g.dpos.shape == pos.shape and not bool(g.dpos.any())
    topo.close()

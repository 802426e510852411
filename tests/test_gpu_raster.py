"""ra_rasterize, ra_interpolate and their backward passes on the device.  Run with `-m gpu` on an MI355X.

Exactness is bit equality: ra_rasterize equals the kernel-order numpy restatement (tests/raster_ref.py), the binned call equals
RA_RASTER_BRUTE, a repeat gives the same bits, a view of a batch equals the call of that view alone.  Arithmetic outputs are held to the
project's 10 x float32 rule (frame_stage_ref.parity) against float64; the float32 reference is raster_ref.plain32 / torch autograd in
float32, the float64 one raster_ref's exhaustive restatement / torch autograd in float64 with the face map held fixed.  Every test
prints its figures before it asserts."""
import functools

import numpy as np
import pytest
import torch

import raster_ref as R
import raycast_ref
from frame_stage_ref import parity
from relightableavatar_amd import _lib, largesteps, mesh_utils, raster_utils
from relightableavatar_amd.config import make_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


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


def same_maps(tag, a, b, view_a=slice(None), view_b=slice(None)):
    for k in ('uv', 'zw', 'face'):
        x, y = bits(torch.as_tensor(a[k])[view_a]), bits(torch.as_tensor(b[k])[view_b])
        same = x.shape == y.shape and bool(torch.equal(x, y))
        print(f'{tag}: {k} bit-equal {same} ({x.numel()} values, {int((x != y).sum()) if x.shape == y.shape else -1} differ)')
        assert same, (tag, k)


@functools.lru_cache(None)
def cases():
    """name -> (pos (B,V,4) float32, faces, H, W)"""
    out = {}
    for H, W in ((64, 64), (37, 53), (1, 1), (8, 8), (9, 7)):
        pos, f = R.sphere_case(H, W)
        out[f'sphere_{H}x{W}'] = (pos[None], f, H, W)
    pos, f = R.lattice_grid()
    out['lattice'] = (pos[None], f, 16, 16)
    for name, (pos, f) in R.triangle_cases().items():
        out[name] = (pos[None], f, 32, 32)
    return out


@functools.lru_cache(None)
def restated(name):
    pos, f, H, W = cases()[name]
    ref = R.sphere_reference(H, W)['r32'] if name in ('sphere_64x64', 'sphere_37x53') else R.raster(pos, f, H, W, np.float32)
    return ref


@pytest.mark.parametrize('name', sorted(cases()))
def test_rasterize_bits(eng, name):
    """the binned call equals the numpy restatement, the brute scan and itself, bit for bit, on every mesh and image size"""
    pos, f, H, W = cases()[name]
    assert eng.lib.ra_raster_tile(0) == 8 and eng.lib.ra_raster_tile(2) == 64
    got = eng.rasterize(T(pos), T(f), H, W)
    ref = restated(name)
    print(f'{name}: {int((got.face >= 0).sum())} covered pixels of {H * W}, restatement {int((ref["face"] >= 0).sum())}')
    same_maps(f'{name} vs restatement', got, {k: torch.tensor(ref[k]) for k in ('uv', 'zw', 'face')})
    same_maps(f'{name} brute', got, eng.rasterize(T(pos), T(f), H, W, brute=True))
    same_maps(f'{name} repeat', got, eng.rasterize(T(pos), T(f), H, W))
    empty = (got.face < 0).cpu()
    assert bool((got.uv.cpu()[empty] == 0).all()) and bool((got.zw.cpu()[empty] == 0).all())


def test_lattice_and_sphere_coverage(eng):
    """the lattice grid covers exactly 64 pixels; the w < 0 triangle and the 300 stacked faces rasterise something"""
    pos, f, H, W = cases()['lattice']
    got = eng.rasterize(T(pos), T(f), H, W)
    n = int((got.face >= 0).sum())
    print(f'lattice: {n} covered pixels')
    assert n == 64
    for name in ('w_negative', 'stacked'):
        pos, f, H, W = cases()[name]
        n = int((eng.rasterize(T(pos), T(f), H, W).face >= 0).sum())
        print(f'{name}: {n} covered pixels')
        assert n > 0


def test_two_views_and_empty(eng):
    """B = 2 with different poses: each view equals its own B = 1 call; F = 0 gives empty maps; a bad index is reported"""
    ref = R.sphere_reference(64, 64, 2)
    pos, f = T(ref['pos']), T(ref['faces'])
    both = eng.rasterize(pos, f, 64, 64)
    same_maps('two views vs restatement', both, {k: torch.tensor(ref['r32'][k]) for k in ('uv', 'zw', 'face')})
    for b in range(2):
        same_maps(f'view {b} alone', both, eng.rasterize(pos[b:b + 1], f, 64, 64), slice(b, b + 1))
    assert not torch.equal(both.face[0], both.face[1])
    none = eng.rasterize(pos, f[:0], 9, 7)
    assert none.face.shape == (2, 9, 7) and bool((none.face == -1).all()) and bool((none.uv == 0).all()) and bool((none.zw == 0).all())
    bad = f.clone()
    bad[5, 1] = pos.shape[1]
    with pytest.raises(_lib.RaError, match='face index'):
        eng.rasterize(pos, bad, 16, 16)
    with pytest.raises(_lib.RaError, match='face index'):
        eng.rasterize(pos, bad, 16, 16, brute=True)


@pytest.mark.parametrize('size', [(64, 64), (37, 53)])
def test_against_float64(eng, size):
    """decided pixels carry the float64 face; u, v, zw under the 10 x rule"""
    H, W = size
    ref = R.sphere_reference(H, W)
    got = eng.rasterize(T(ref['pos']), T(ref['faces']), H, W)
    r64 = ref['r64']
    face = got.face.cpu().numpy()
    undecided = float((~r64['decided']).mean())
    wrong = int(((face != r64['face']) & r64['decided']).sum())
    print(f'sphere {H}x{W}: undecided {undecided:.4%}, wrong faces on decided pixels {wrong}')
    assert undecided <= 0.01 and wrong == 0
    keep = (face == r64['face']) & (face >= 0) & r64['decided']
    plain = R.plain32(ref['pos'], ref['faces'], r64['face'], H, W)
    parity(f'sphere {H}x{W} uv', got.uv.cpu(), plain['uv'], r64['uv'], keep=torch.from_numpy(keep)[..., None].expand(-1, -1, -1, 2))
    parity(f'sphere {H}x{W} zw', got.zw.cpu(), plain['zw'], r64['zw'], keep=keep)


def test_against_raycast(eng):
    """rays through the same pixel centres (camera coordinate i + 0.5) meet the same face on decided pixels, with the same barycentrics"""
    H = W = 64
    ref = R.sphere_reference(H, W)
    verts, faces = R.uv_sphere()
    K, Rm, Tv = R.camera(H, W)
    ix, iy = np.meshgrid(np.arange(W), np.arange(H))
    pix = np.stack([ix + 0.5, iy + 0.5, np.ones_like(ix, dtype=np.float64)], -1).reshape(-1, 3)
    d = (pix @ np.linalg.inv(K).T) @ Rm
    o = np.broadcast_to(-Rm.T @ Tv, d.shape)
    o32, d32 = o.astype(np.float32), d.astype(np.float32)
    got = eng.rasterize(T(ref['pos']), T(ref['faces']), H, W)
    mesh = eng.mesh(T(verts.astype(np.float32)), torch.from_numpy(faces))
    hit = mesh.raycast(T(o32), T(d32), want=('t', 'face', 'uv'), sort=False)
    mesh.close()
    r64 = ref['r64']
    decided = r64['decided'].reshape(-1)
    rf, cf = got.face.cpu().numpy().reshape(-1), hit.face.cpu().numpy()
    differ = int(((rf != cf) & decided).sum())
    print(f'raycast cross-check: {int((rf >= 0).sum())} raster hits, {int((cf >= 0).sum())} ray hits, {differ} decided pixels with another face')
    assert differ == 0
    keep = (rf == cf) & (rf >= 0) & decided
    # the two bounds of the 10 x rule, neither taken from the code under test: the float32 baselines' own errors against float64
    plain = R.plain32(ref['pos'], ref['faces'], r64['face'], H, W)
    m = (r64['face'] >= 0)
    raster_bound = 10 * float(np.abs(plain['uv'][m] - r64['uv'][m]).max())
    tris = verts[faces][r64['face'].reshape(-1)[keep]]
    pair = lambda dt: np.stack([np.stack(raycast_ref.moller_trumbore(o32[keep][k:k + 1], d32[keep][k:k + 1], tris[k:k + 1], dt)[:2], -1)[0, 0]
                                for k in range(int(keep.sum()))])
    ray_bound = 10 * float(np.abs(pair(np.float32).astype(np.float64) - pair(np.float64)).max())
    u, v = got.uv.cpu().numpy().reshape(-1, 2)[keep].T
    ray_uv = hit.uv.cpu().numpy()[keep]         # the barycentrics of corners 1 and 2
    worst = max(float(np.abs(v - ray_uv[:, 0]).max()), float(np.abs(((1 - u) - v) - ray_uv[:, 1]).max()))
    print(f'raycast cross-check: max barycentric difference {worst:.3e}, bound {raster_bound:.3e} + {ray_bound:.3e} on {int(keep.sum())} pixels')
    assert worst <= raster_bound + ray_bound


@functools.lru_cache(None)
def grad_case():
    """two views of the sphere at 64 x 64 with seeded attributes and upstream gradients, and the autograd references"""
    ref = R.sphere_reference(64, 64, 2)
    rng = np.random.default_rng(11)
    V = ref['pos'].shape[1]
    face = ref['r32']['face']
    out = dict(ref=ref, face=face, duv=rng.standard_normal((2, 64, 64, 2)).astype(np.float32))
    for A in (1, 3, 64):
        out[A] = dict(shared=rng.standard_normal((V, A)).astype(np.float32), per_view=rng.standard_normal((2, V, A)).astype(np.float32),
                      dout=rng.standard_normal((2, 64, 64, A)).astype(np.float32))
    return out


@pytest.mark.parametrize('A', [1, 3, 64])
@pytest.mark.parametrize('kind', ['shared', 'per_view'])
def test_interpolate(eng, A, kind):
    """forward and backward of the interpolation under the 10 x rule, repeatable, 0 where nothing is seen"""
    g = grad_case()
    ref, face = g['ref'], g['face']
    attr, dout = g[A][kind], g[A]['dout']
    rast = eng.rasterize(T(ref['pos']), T(ref['faces']), 64, 64)
    assert torch.equal(rast.face.cpu(), torch.tensor(face))
    out = eng.interpolate(T(attr), rast, T(ref['faces']))
    uv32 = ref['r32']['uv']
    i32, i64 = R.interp(attr, ref['faces'], uv32, face, np.float32), R.interp(attr, ref['faces'], uv32, face, np.float64)
    parity(f'interpolate A={A} {kind}', out.cpu(), i32, i64)
    assert bool((out.cpu()[torch.from_numpy(face < 0)] == 0).all())
    topo = eng.topology(T(ref['faces']), ref['pos'].shape[1])
    got = eng.interpolate_backward(topo, T(attr), rast, T(dout))
    a32 = R.grads_autograd(ref['pos'], ref['faces'], face, g['duv'], attr, dout, torch.float32)
    a64 = R.grads_autograd(ref['pos'], ref['faces'], face, g['duv'], attr, dout, torch.float64)
    parity(f'd attr A={A} {kind}', got.dattr.cpu(), a32['dattr'], a64['dattr'])
    parity(f'd uv A={A} {kind}', got.duv.cpu(), a32['duv_interp'], a64['duv_interp'])
    again = eng.interpolate_backward(topo, T(attr), rast, T(dout))
    assert torch.equal(bits(got.dattr), bits(again.dattr)) and torch.equal(bits(got.duv), bits(again.duv))
    seen = np.zeros(ref['pos'].shape[1], bool)
    views = range(2)
    for b in views:
        seen[np.unique(ref['faces'][face[b][face[b] >= 0]])] = True
    print(f'd attr A={A} {kind}: {int((~seen).sum())} vertices no pixel sees')
    assert (~seen).sum() > 0 and bool((got.dattr.cpu()[..., torch.from_numpy(~seen), :] == 0).all())
    assert bool((got.duv.cpu()[torch.from_numpy(face < 0)] == 0).all())
    topo.close()


def test_rasterize_backward(eng):
    """d pos under the 10 x rule against float64 autograd; repeatable; a view's rows do not depend on the other view; the pole (valence
    16) is covered; a vertex no pixel sees gets exactly 0"""
    g = grad_case()
    ref, face, duv = g['ref'], g['face'], g['duv']
    pos, f = T(ref['pos']), T(ref['faces'])
    rast = eng.rasterize(pos, f, 64, 64)
    topo = eng.topology(f, pos.shape[1])
    assert topo.max_outgoing == 16
    got = eng.rasterize_backward(topo, pos, rast, T(duv))
    attr, dout = g[1]['shared'], g[1]['dout']
    a32 = R.grads_autograd(ref['pos'], ref['faces'], face, duv, attr, dout, torch.float32)
    a64 = R.grads_autograd(ref['pos'], ref['faces'], face, duv, attr, dout, torch.float64)
    parity('d pos', got.cpu(), a32['dpos'], a64['dpos'])
    assert bool((got[..., 2] == 0).all())
    again = eng.rasterize_backward(topo, pos, rast, T(duv))
    assert torch.equal(bits(got), bits(again))
    for b in range(2):
        one = eng.rasterize(pos[b:b + 1], f, 64, 64)
        alone = eng.rasterize_backward(topo, pos[b:b + 1], one, T(duv[b:b + 1]))
        same = torch.equal(bits(got[b:b + 1]), bits(alone))
        print(f'd pos: view {b} alone bit-equal {same}')
        assert same
    for b in range(2):
        seen = np.zeros(pos.shape[1], bool)
        seen[np.unique(ref['faces'][face[b][face[b] >= 0]])] = True
        pole = [v for v in (0, pos.shape[1] - 1) if seen[v]]
        print(f'd pos view {b}: {int(seen.sum())} vertices seen, poles seen {pole}')
        assert (~seen).any() and bool((got[b].cpu()[torch.from_numpy(~seen)] == 0).all())
        if b == 0:
            assert pole and all(float(got[b, v].abs().max()) > 0 for v in pole)
    topo.close()


def test_autograd_end_to_end(eng):
    """raster_utils.rasterize -> interpolate -> loss: torch.autograd reaches the positions and the attributes and matches the engine calls"""
    g = grad_case()
    ref = g['ref']
    pos = T(ref['pos']).requires_grad_(True)
    attr = T(g[3]['shared']).requires_grad_(True)
    f = T(ref['faces'])
    topo = eng.topology(f, pos.shape[1])
    rast = raster_utils.rasterize(pos, f, 64, 64, engine=eng, topology=topo)
    assert rast.shape == (2, 64, 64, 4) and torch.equal((rast[..., 3] - 1).int().cpu(), torch.tensor(g['face']))
    out = raster_utils.interpolate(attr, rast, f, engine=eng, topology=topo)
    w = T(g[3]['dout'])
    (out * w).sum().backward()
    raw = eng.rasterize(pos.detach(), f, 64, 64)
    d = eng.interpolate_backward(topo, attr.detach(), raw, w)
    assert torch.equal(bits(attr.grad), bits(d.dattr))
    assert torch.equal(bits(pos.grad), bits(eng.rasterize_backward(topo, pos.detach(), raw, d.duv)))
    assert float(pos.grad.abs().max()) > 0
    # without a topology the backward builds its own
    pos2 = T(ref['pos']).requires_grad_(True)
    raster_utils.interpolate(attr.detach(), raster_utils.rasterize(pos2, f, 64, 64, engine=eng), f, engine=eng).mul(w).sum().backward()
    assert torch.equal(bits(pos2.grad), bits(pos.grad))
    topo.close()


def test_render_and_maps(eng):
    """render_nvdiffrast(R_S=2) and raster_maps: shapes, dtypes, masks; the texture arguments raise"""
    verts, faces = R.uv_sphere()
    K, Rm, Tv = R.camera(32, 32)
    v, f = T(verts.astype(np.float32)), T(faces)
    Rt, Tt = T(np.stack([Rm, Rm]).astype(np.float32)), T(np.stack([Tv, Tv]).astype(np.float32))[..., None]
    P = raster_utils.get_ndc_perspective_matrix(T(np.stack([K, K]).astype(np.float32)), 32, 32)
    attrs = torch.rand(v.shape[0], 5, device=DEV)
    img, msk = raster_utils.render_nvdiffrast(v, f, attrs, H=32, W=32, R=Rt, T=Tt, K=P, R_S=2, engine=eng)
    assert img.shape == (2, 32, 32, 5) and msk.shape == (2, 32, 32) and img.dtype == msk.dtype == torch.float32
    assert 0 < float(msk.mean()) < 1 and float(msk.min()) == 0 and float(msk.max()) == 1
    assert bool(((msk > 0) & (msk < 1)).any())          # the soft edge of the supersampled mask
    assert torch.equal(bits(img[0]), bits(img[1]))
    maps = mesh_utils.raster_maps(v, f, 32, 32, K, Rm, Tv, engine=eng)
    assert maps.acc_map.shape == (32, 32, 1) and maps.depth_map.shape == (32, 32, 1) and maps.norm_map.shape == (32, 32, 3) and maps.face.shape == (32, 32)
    assert maps.face.dtype == torch.int32 and maps.acc_map.dtype == maps.depth_map.dtype == maps.norm_map.dtype == torch.float32
    hit = maps.face >= 0
    depth = maps.depth_map[..., 0]
    print(f'raster_maps: {int(hit.sum())} pixels, depth {float(depth[hit].min()):.3f} .. {float(depth[hit].max()):.3f}')
    assert 0 < int(hit.sum()) < 32 * 32 and torch.equal(maps.acc_map[..., 0] > 0, hit)
    assert float(depth[hit].min()) > 1.4 and float(depth[hit].max()) < 2.1 and bool((depth[~hit] == 0).all())
    assert torch.allclose(maps.norm_map[hit].norm(dim=-1), torch.ones(int(hit.sum()), device=DEV), atol=1e-5)
    with pytest.raises(NotImplementedError):
        raster_utils.render_nvdiffrast(v, f, attrs, uv=torch.rand(v.shape[0], 2), img=torch.rand(1, 8, 8, 3), H=32, W=32, engine=eng)
    with pytest.raises(NotImplementedError):
        raster_utils.interpolate(attrs, torch.zeros(1, 4, 4, 4, device=DEV), f, rast_db=torch.zeros(1), engine=eng)


def test_fit(eng):
    """30 steps of AdamUniform on a subdivided icosahedron's vertices against the depth and normal maps of a smoothed copy lower the loss"""
    t = (1 + 5 ** 0.5) / 2
    ico = torch.tensor([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1],
                        [-t, 0, 1]], dtype=torch.float32, device=DEV) * 0.25
    faces = torch.tensor([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2],
                          [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], dtype=torch.int32, device=DEV)
    topo = eng.topology(faces, 12)
    verts, faces, topo = topo.subdivide(ico)
    verts, faces, topo = topo.subdivide(verts)
    target = topo.smooth(verts, iter=20)
    H = W = 48
    K, Rm, Tv = R.camera(H, W)
    Rt, Tt = T(Rm.astype(np.float32))[None], T(Tv.astype(np.float32))[None, :, None]
    P = raster_utils.get_ndc_perspective_matrix(T(K.astype(np.float32))[None], H, W)

    def maps(v):
        cam = v @ Rt[0].mT + Tt[0].mT
        fn = torch.linalg.cross(v[faces.long()[:, 1]] - v[faces.long()[:, 0]], v[faces.long()[:, 2]] - v[faces.long()[:, 0]])
        vn = torch.zeros_like(v).index_add(0, faces.long().reshape(-1), fn.repeat_interleave(3, 0))
        vn = vn / vn.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        return raster_utils.render_nvdiffrast(v, faces, torch.cat([cam[:, 2:3], vn], -1), H=H, W=W, R=Rt, T=Tt, K=P, R_S=1, engine=eng, topology=topo)[0]

    goal = maps(target).detach()
    param = verts.clone().requires_grad_(True)
    opt = largesteps.AdamUniform([param], lr=2e-3, engine=eng)
    losses = []
    for _ in range(31):
        opt.zero_grad()
        loss = (maps(param) - goal).square().mean()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print(f'fit: loss {losses[0]:.4e} -> {losses[-1]:.4e}')
    assert losses[-1] < losses[0]
    topo.close()


def test_foreign_topology_is_refused(eng):
    """the backward calls take a topology of their own ctx; sizes that do not fit it are named"""
    import ctypes as C
    ref = R.sphere_reference(64, 64)
    pos, f = T(ref['pos']), T(ref['faces'])
    rast = eng.rasterize(pos, f, 64, 64)
    g = torch.zeros_like(rast.uv)
    p = lambda t: C.c_void_p(t.data_ptr())
    L, err = eng.lib, lambda: eng.lib.ra_last_error().decode()
    stranger = C.c_void_p(8)          # compared with the ctx's topologies, never dereferenced
    assert L.ra_rasterize_backward(eng.ctx, stranger, p(pos), 1, pos.shape[1], 64, 64, p(rast.uv), p(rast.face), p(g), p(torch.empty_like(pos)), eng.stream) != 0
    assert 'ra_rasterize_backward: not a topology of this ctx' in err()
    a = torch.zeros(pos.shape[1], 2, device=DEV)
    d = torch.zeros(1, 64, 64, 2, device=DEV)
    assert L.ra_interpolate_backward(eng.ctx, stranger, p(a), 0, pos.shape[1], 2, p(rast.uv), p(rast.face), 1, 64, 64, p(d), p(torch.empty_like(a)), None, eng.stream) != 0
    assert 'ra_interpolate_backward: not a topology of this ctx' in err()
    topo = eng.topology(f[:10], pos.shape[1] + 1)
    with pytest.raises(_lib.RaError, match='bad sizes'):
        eng.rasterize_backward(topo, pos, rast, g)
    with pytest.raises(_lib.RaError, match='bad sizes'):
        eng.interpolate_backward(topo, a, rast, d)
    topo.close()

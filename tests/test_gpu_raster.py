"""ra_rasterize, ra_interpolate and their backward passes on the device.  Run with `-m gpu` on an MI355X.

Exactness is bit equality: ra_rasterize equals the kernel-order numpy restatement (tests/raster_ref.py), the binned call equals
RA_RASTER_BRUTE, a repeat gives the same bits, a view of a batch equals the call of that view alone, and the three gradients equal
raster_ref.grads_kernel_order on faces that own from 1 to 4 363 pixels.  Arithmetic outputs are held to the
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


# ---- the backward passes on faces that own more than one wave of pixels (tests/raster_ref.py: backward_case_list) -------------------------
def same_bits(tag, got, ref):
    """prints the verdict and returns it: the asserts come after every figure of the test is printed"""
    x, y = bits(got), bits(torch.as_tensor(np.ascontiguousarray(ref)))
    same = x.shape == y.shape and bool(torch.equal(x, y))
    print(f'{tag}: bit-equal {same} ({x.numel()} values, {int((x != y).sum()) if x.shape == y.shape else -1} differ)')
    return same


def forward_of(eng, name):
    """the device's forward of a case, asserted equal to the restatement: the backward references start from the restatement's uv and face"""
    c = R.backward_case(name)
    rast = eng.rasterize(T(c['pos']), T(c['faces']), c['H'], c['W'])
    same_maps(f'{name} forward vs restatement', rast, {k: torch.tensor(c['r32'][k]) for k in ('uv', 'zw', 'face')})
    return c, rast


def seen_vertices(c, b):
    face = c['r32']['face'][b]
    seen = np.zeros(c['pos'].shape[1], bool)
    seen[np.unique(c['faces'][face[face >= 0]])] = True
    return seen


@pytest.mark.parametrize('name,A', R.BACKWARD_PARAMS)
@pytest.mark.parametrize('kind', ['shared', 'per_view'])
def test_interpolate_backward_runs(eng, name, A, kind):
    """d attr and d uv equal the kernel-order restatement bit for bit, hold the 10 x rule against float32 and float64 autograd, repeat
    with the same bits, and are exactly 0 where nothing is seen"""
    c, rast = forward_of(eng, name)
    g = R.backward_reference(name, A, kind)
    topo = eng.topology(T(c['faces']), c['pos'].shape[1])
    got = eng.interpolate_backward(topo, T(g['attr']), rast, T(g['dout']))
    again = eng.interpolate_backward(topo, T(g['attr']), rast, T(g['dout']))
    topo.close()
    runs = c['runs']
    print(f'{name} A={A} {kind}: {len(runs)} runs, largest {int(runs.max()) if len(runs) else 0}, {int((runs > 64).sum())} above 64')
    ok = [same_bits(f'{name} A={A} {kind} d attr vs kernel order', got.dattr, g['kernel']['dattr']),
          same_bits(f'{name} A={A} {kind} d uv vs kernel order', got.duv, g['kernel']['duv_interp']),
          same_bits(f'{name} A={A} {kind} d attr repeat', again.dattr, got.dattr.cpu().numpy()),
          same_bits(f'{name} A={A} {kind} d uv repeat', again.duv, got.duv.cpu().numpy())]
    parity(f'{name} A={A} {kind} d attr', got.dattr.cpu(), g['a32']['dattr'], g['a64']['dattr'])
    parity(f'{name} A={A} {kind} d uv', got.duv.cpu(), g['a32']['duv_interp'], g['a64']['duv_interp'])
    assert all(ok), ok
    dattr = got.dattr.cpu().numpy()
    seen = np.stack([seen_vertices(c, b) for b in range(c['pos'].shape[0])])
    unseen = ~seen.any(0) if kind == 'shared' else ~seen
    assert not dattr[unseen].any() and not got.duv.cpu().numpy()[c['r32']['face'] < 0].any()
    if name == 'sphere_1x1':
        assert not dattr.any() and not got.duv.cpu().numpy().any()


@pytest.mark.parametrize('name', R.BACKWARD_CASES)
def test_rasterize_backward_runs(eng, name):
    """d pos equals the kernel-order restatement bit for bit, holds the 10 x rule against float32 and float64 autograd, repeats with the
    same bits, carries nothing in z and is exactly 0 at vertices no pixel sees or no face references"""
    c, rast = forward_of(eng, name)
    g = R.backward_reference(name, 3, 'shared')
    pos = T(c['pos'])
    topo = eng.topology(T(c['faces']), pos.shape[1])
    got = eng.rasterize_backward(topo, pos, rast, T(c['duv']))
    again = eng.rasterize_backward(topo, pos, rast, T(c['duv']))
    topo.close()
    runs = c['runs']
    print(f'{name}: {len(runs)} runs, largest {int(runs.max()) if len(runs) else 0}, {int((runs > 64).sum())} above 64')
    ok = [same_bits(f'{name} d pos vs kernel order', got, g['kernel']['dpos']), same_bits(f'{name} d pos repeat', again, got.cpu().numpy())]
    parity(f'{name} d pos', got.cpu(), g['a32']['dpos'], g['a64']['dpos'])
    assert all(ok), ok
    d = got.cpu().numpy()
    assert not d[..., 2].any()
    for b in range(d.shape[0]):
        seen = seen_vertices(c, b)
        print(f'{name} view {b}: {int(seen.sum())} of {len(seen)} vertices seen')
        assert not d[b, ~seen].any() and (not seen.any() or d[b, seen].any())
    if name == 'sphere_1x1':
        assert not d.any()
    if name == 'open_37x53':
        assert not d[:, -3:].any()


def test_three_views_are_independent(eng):
    """B = 3: row b of d pos and of per-view d attr equals the B = 1 call of that view; d uv likewise"""
    name = 'sphere3_37x53'
    c, rast = forward_of(eng, name)
    g = R.backward_reference(name, 3, 'per_view')
    pos, f = T(c['pos']), T(c['faces'])
    topo = eng.topology(f, pos.shape[1])
    attr, dout, duv = T(g['attr']), T(g['dout']), T(c['duv'])
    dpos, di = eng.rasterize_backward(topo, pos, rast, duv), eng.interpolate_backward(topo, attr, rast, dout)
    ok = []
    for b in range(3):
        v = slice(b, b + 1)
        one = eng.rasterize(pos[v], f, c['H'], c['W'])
        same_maps(f'{name} view {b} alone', rast, one, v)
        alone = eng.interpolate_backward(topo, attr[v], one, dout[v])
        ok += [same_bits(f'{name} d pos view {b} alone', eng.rasterize_backward(topo, pos[v], one, duv[v]), dpos[v].cpu().numpy()),
               same_bits(f'{name} d attr view {b} alone', alone.dattr, di.dattr[v].cpu().numpy()),
               same_bits(f'{name} d uv view {b} alone', alone.duv, di.duv[v].cpu().numpy())]
    topo.close()
    assert all(ok), ok
    assert not torch.equal(dpos[0], dpos[1]) and not torch.equal(dpos[1], dpos[2])


@pytest.mark.parametrize('name', ['run_65', 'sphere2_136x200', 'sphere_1x1'])
def test_want_subsets(eng, name):
    """interpolate_backward(want=('dattr',)) and (want=('duv',)) return the bits of the matching half of the full call"""
    c, rast = forward_of(eng, name)
    ok = []
    topo = eng.topology(T(c['faces']), c['pos'].shape[1])
    for kind in ('shared', 'per_view'):
        g = R.backward_reference(name, 3, kind)
        attr, dout = T(g['attr']), T(g['dout'])
        full = eng.interpolate_backward(topo, attr, rast, dout)
        only_a, only_uv = eng.interpolate_backward(topo, attr, rast, dout, want=('dattr',)), eng.interpolate_backward(topo, attr, rast, dout, want=('duv',))
        assert sorted(only_a) == ['dattr'] and sorted(only_uv) == ['duv']
        ok += [same_bits(f'{name} {kind} want dattr', only_a.dattr, full.dattr.cpu().numpy()), same_bits(f'{name} {kind} want duv', only_uv.duv, full.duv.cpu().numpy()),
               same_bits(f'{name} {kind} full d attr vs kernel order', full.dattr, g['kernel']['dattr']),
               same_bits(f'{name} {kind} full d uv vs kernel order', full.duv, g['kernel']['duv_interp'])]
    topo.close()
    assert all(ok), ok


@pytest.mark.parametrize('name', ['w_negative_130x70', 'sphere2_200x136', 'sphere2_136x200', 'sphere3_37x53', 'open_37x53'])
def test_rasterize_bits_at_the_new_shapes(eng, name):
    """the forward at the shapes of the backward cases: partial tiles on both axes, H != W, three views, boundaries — equal to the
    restatement, to RA_RASTER_BRUTE and to a repeat, bit for bit"""
    c, got = forward_of(eng, name)
    pos, f = T(c['pos']), T(c['faces'])
    print(f'{name}: {int((got.face >= 0).sum())} covered pixels of {got.face.numel()}')
    same_maps(f'{name} brute', got, eng.rasterize(pos, f, c['H'], c['W'], brute=True))
    same_maps(f'{name} repeat', got, eng.rasterize(pos, f, c['H'], c['W']))
    empty = (got.face < 0).cpu()
    assert bool((got.uv.cpu()[empty] == 0).all()) and bool((got.zw.cpu()[empty] == 0).all())
    r64 = c['r64']
    wrong = int(((got.face.cpu().numpy() != r64['face']) & r64['decided']).sum())
    print(f'{name}: undecided {float((~r64["decided"]).mean()):.4%}, wrong faces on decided pixels {wrong}')
    assert wrong == 0


def test_scratch_reuse(eng):
    """the ctx's grow-only scratch (raster_keys, raster_pix_sorted, raster_sort_tmp, raster_g_face): a small call after a large one
    ignores the stale tail.  One ctx, in order: the 9 x 7 sphere, the w < 0 triangle at 130 x 70 (4 363 pixels on one face, 64 channels),
    the 9 x 7 sphere again — forward and both backwards each time —, then ra_interpolate_backward with 64 channels and ra_rasterize_backward
    on the 9 x 7 sphere, which share raster_g_face (B F 3 A floats, then B F 9)"""
    def run(name, A):
        c = R.backward_case(name)
        g = R.backward_reference(name, A, 'shared')
        pos, f = T(c['pos']), T(c['faces'])
        rast = eng.rasterize(pos, f, c['H'], c['W'])
        topo = eng.topology(f, pos.shape[1])
        di = eng.interpolate_backward(topo, T(g['attr']), rast, T(g['dout']))
        dpos = eng.rasterize_backward(topo, pos, rast, T(c['duv']))
        topo.close()
        out = dict(uv=rast.uv.cpu().numpy(), zw=rast.zw.cpu().numpy(), face=rast.face.cpu().numpy(), dattr=di.dattr.cpu().numpy(), duv_interp=di.duv.cpu().numpy(),
                   dpos=dpos.cpu().numpy())
        ref = dict(c['r32'], **g['kernel'])
        return out, [same_bits(f'scratch reuse, {name} A={A}: {k} vs restatement', out[k], ref[k]) for k in out]
    first, ok1 = run('sphere2_9x7', 3)
    _, ok2 = run('w_negative_130x70', 64)
    second, ok3 = run('sphere2_9x7', 3)
    ok4 = [same_bits(f'scratch reuse, second 9 x 7 call vs first: {k}', second[k], first[k]) for k in first]
    wide, ok5 = run('sphere2_9x7', 64)          # interpolate_backward with 64 channels, then rasterize_backward in the same scratch
    ok5 += [same_bits('scratch reuse, d pos after the 64-channel call vs first', wide['dpos'], first['dpos'])]
    assert all(ok1) and all(ok2) and all(ok3) and all(ok4) and all(ok5), (ok1, ok2, ok3, ok4, ok5)


# ---- render_nvdiffrast and raster_maps by value ---------------------------------------------------------------------------------------------
def resize64(x, H, W, dtype=torch.float64):
    """(B,h,w,C) numpy -> (B,H,W,C): bilinear, align_corners=False, in the given precision on the CPU"""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).permute(0, 3, 1, 2)
    return torch.nn.functional.interpolate(t, [H, W], mode='bilinear', align_corners=False).permute(0, 2, 3, 1).numpy()


def render_restated(clip, faces, attrs, H, W, R_S):
    """render_nvdiffrast's attribute path restated from the float32 clip positions: raster in float64 at R_S times the size, interp,
    bilinear resize in float64; the float32 baseline is the same steps on plain32's barycentrics.  keep: output pixels whose source
    pixels are all decided (there the float32 face is the float64 face: asserted)."""
    h, w = H * R_S, W * R_S
    r64, r32 = R.raster(clip, faces, h, w, np.float64), R.raster(clip, faces, h, w, np.float32)
    assert int(((r32['face'] != r64['face']) & r64['decided']).sum()) == 0
    face = r64['face']
    img64 = resize64(R.interp(attrs, faces, r64['uv'], face, np.float64), H, W)
    img32 = resize64(R.interp(attrs, faces, R.plain32(clip, faces, face, h, w)['uv'], face, np.float32), H, W, torch.float32)
    msk64 = resize64((face >= 0)[..., None], H, W)[..., 0]
    keep = resize64(r64['decided'][..., None], H, W)[..., 0] == 1
    return dict(img64=img64, img32=img32, msk64=msk64, keep=keep)


@pytest.mark.parametrize('size', [(32, 32), (37, 53)])
@pytest.mark.parametrize('R_S', [1, 2])
def test_render_nvdiffrast_by_value(eng, size, R_S):
    """render_nvdiffrast's image under the 10 x rule and its mask exactly, on the output pixels whose source pixels are all decided"""
    H, W = size
    verts, faces = R.uv_sphere()
    cams = [R.camera(H, W, angle) for angle in (0.6, 1.5)]
    v, f = T(verts.astype(np.float32)), T(faces)
    Rt, Tt = T(np.stack([c[1] for c in cams]).astype(np.float32)), T(np.stack([c[2] for c in cams]).astype(np.float32))[..., None]
    P = raster_utils.get_ndc_perspective_matrix(T(np.stack([c[0] for c in cams]).astype(np.float32)), H, W)
    attrs = np.random.default_rng(7).standard_normal((len(verts), 5)).astype(np.float32)
    img, msk = raster_utils.render_nvdiffrast(v, f, T(attrs), H=H, W=W, R=Rt, T=Tt, K=P, R_S=R_S, engine=eng)
    # step 1, the same float32 clip positions: render_nvdiffrast's own expressions on the same device tensors
    vv = v[None].expand(2, -1, -1).contiguous() @ Rt.mT + Tt.mT
    clip = (torch.cat([vv, vv.new_ones((*vv.shape[:-1], 1))], dim=-1) @ P.mT).cpu().numpy()
    ref = render_restated(clip, faces, attrs, H, W, R_S)
    covered = ref['msk64'] > 0
    left_out = float((covered & ~ref['keep']).sum() / covered.sum())
    mask_same = bool(np.array_equal(msk.cpu().numpy()[ref['keep']], ref['msk64'][ref['keep']].astype(np.float32)))
    soft = int(((ref['msk64'] > 0) & (ref['msk64'] < 1)).sum())
    print(f'render_nvdiffrast {H}x{W} R_S={R_S}: {int(covered.sum())} covered output pixels, {left_out:.4%} of them left out, {soft} soft mask pixels, mask exact {mask_same}')
    assert img.shape == (2, H, W, 5) and msk.shape == (2, H, W) and img.dtype == msk.dtype == torch.float32
    keep = np.broadcast_to(ref['keep'][..., None], img.shape).copy()
    parity(f'render_nvdiffrast {H}x{W} R_S={R_S} image', img.cpu(), ref['img32'], ref['img64'], keep=keep)
    assert left_out <= 0.01 and mask_same and (soft > 0) == (R_S > 1)
    assert not img.cpu().numpy()[(ref['msk64'] == 0) & ref['keep']].any()


@pytest.mark.parametrize('size', [(32, 32), (37, 53)])
def test_raster_maps_by_value(eng, size):
    """raster_maps: the face is the float64 face on decided pixels; depth and normal under the 10 x rule against the float64 restatement"""
    H, W = size
    verts, faces = R.uv_sphere()
    K, Rm, Tv = R.camera(H, W)
    v32 = verts.astype(np.float32)
    v, f = T(v32), T(faces)
    maps = mesh_utils.raster_maps(v, f, H, W, K, Rm, Tv, engine=eng)
    # the same float32 camera-space and clip positions: raster_maps' own expressions on the same device tensors
    Kt, Rt, Tt = (torch.as_tensor(x).to(device=DEV, dtype=torch.float32) for x in (K, Rm, Tv))
    cam = v @ Rt.mT + Tt.reshape(1, 3)
    clip = (torch.cat([cam, torch.ones_like(cam[:, :1])], dim=-1) @ raster_utils.get_ndc_perspective_matrix(Kt, H, W).mT).cpu().numpy()
    z = cam[:, 2:3].cpu().numpy()
    r64 = R.raster(clip, faces, H, W, np.float64)
    face64, decided = r64['face'][0], r64['decided'][0]
    got_face = maps.face.cpu().numpy()
    wrong = int(((got_face != face64) & decided).sum())
    keep = decided & (face64 >= 0) & (got_face == face64)
    covered = face64 >= 0
    left_out = float((covered & ~keep).sum() / covered.sum())
    print(f'raster_maps {H}x{W}: {int(covered.sum())} covered pixels, {wrong} wrong faces on decided pixels, {left_out:.4%} left out')
    depth64 = R.interp(z, faces, r64['uv'], r64['face'], np.float64)[0]
    depth32 = R.interp(z, faces, R.plain32(clip, faces, r64['face'], H, W)['uv'], r64['face'], np.float32)[0]
    normal = lambda dt: (lambda t: np.cross(t[..., 1, :] - t[..., 0, :], t[..., 2, :] - t[..., 0, :]))(v32.astype(dt)[faces[np.maximum(face64, 0)]])
    unit = lambda n: np.where(covered[..., None], n / np.linalg.norm(n, axis=-1, keepdims=True), 0).astype(n.dtype)
    parity(f'raster_maps {H}x{W} depth', maps.depth_map.cpu(), depth32, depth64, keep=keep[..., None])
    parity(f'raster_maps {H}x{W} normal', maps.norm_map.cpu(), unit(normal(np.float32)), unit(normal(np.float64)), keep=np.broadcast_to(keep[..., None], (H, W, 3)).copy())
    assert wrong == 0 and left_out <= 0.01
    assert np.array_equal(maps.acc_map.cpu().numpy()[..., 0] > 0, got_face >= 0)
    assert not maps.depth_map.cpu().numpy()[got_face < 0].any() and not maps.norm_map.cpu().numpy()[got_face < 0].any()

"""ra_sdf_volume, ra_marching_cubes, ra_mesh_largest_component and renderer.mesh_renderer on the device.  Run
with `-m gpu` on an MI355X.

No tolerance is chosen here: vertices, faces AND their order are compared with the numpy restatement (tests/mesh_extract_ref.py)
bit for bit, and the property list of tests/test_oracle_mesh_extract.py — computed from the input volume and the returned mesh only —
is run on what the device returned.  The restatement and the device share one triangle table, so the equality vouches for how the
table is applied and the property list for the table itself.  The volume is held to the oracle under the project's 10 x float32
rule (frame_stage_ref.parity); the end-to-end margins are the issue's, the albedo's the project's rule for the 16-bit material heads.  Every test prints its figures before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mesh_extract_ref as R
from relightableavatar_amd import _lib
from relightableavatar_amd._lib import RaError
from relightableavatar_amd.config import make_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from relightableavatar_amd.engine import Engine
    return Engine(make_cfg('relight'), device='cuda:0')          # any context will do: no weights are read


def edge_sized_volume(shape, seed):
    """a smooth blob plus noise, with a border of outside: crossings in every part of an oddly sized grid"""
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing='ij'), -1)
    vol = (0.8 - np.linalg.norm(g, axis=-1) + 0.3 * np.random.default_rng(seed).uniform(-1, 1, shape)).astype(np.float32)
    for ax in range(3):
        idx = [slice(None)] * 3
        for side in (0, -1):
            idx[ax] = side
            vol[tuple(idx)] = R.OUTSIDE
    return vol


@functools.lru_cache(None)
def volume(name):
    """(volume, iso, closed): closed = no surface reaches the border"""
    if name == 'patterns':
        return R.all_patterns_volume(), 0.0, True
    if name == 'sphere':
        return R.sphere_volume(), 0.0, True
    if name == 'torus':
        return R.torus_volume(), 0.0, True
    if name == 'random':
        return R.random_volume(), 0.0, True
    if name == 'exact_iso':
        return R.exact_iso_volume(), 0.0, True
    if name == '33x17x65':              # more points than one workgroup's, no axis a multiple of the wave
        return edge_sized_volume((33, 17, 65), 1), 0.05, True
    if name == '2x2x2':                 # the smallest legal volume: one cell, open
        return R.pattern_volume(0b10010110)[1:3, 1:3, 1:3].copy(), 0.0, False
    if name == '2x3x65':
        return np.random.default_rng(2).uniform(-1, 1, (2, 3, 65)).astype(np.float32), 0.1, False
    if name == 'last_cell':
        return R.last_cell_volume(), 0.0, False
    raise KeyError(name)


VOLUMES = ('patterns', 'sphere', 'torus', 'random', 'exact_iso', '33x17x65', '2x2x2', '2x3x65', 'last_cell')


@functools.lru_cache(None)
def reference(name):
    vol, iso, _ = volume(name)
    return R.marching_cubes(vol, iso)


@pytest.mark.parametrize('name', VOLUMES)
def test_marching_cubes_equals_the_restatement_bit_for_bit(eng, name):
    vol, iso, closed = volume(name)
    block = _lib.lib().ra_mcubes_tile(0)
    v, f = eng.marching_cubes(torch.from_numpy(vol), iso)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    v, f = v.cpu().numpy(), f.cpu().numpy()
    rv, rf = reference(name)
    fig = R.check_properties(vol, iso, v, f, closed=closed)
    print(name, vol.shape, f'{vol.size} points = {vol.size / block:.2f} workgroups;', fig, '; reference', rv.shape, rf.shape)
    assert v.shape == rv.shape and f.shape == rf.shape
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32)), 'vertices or their order'
    assert np.array_equal(f, rf), 'faces or their order'
    if closed and len(f):
        assert R.normals_towards_smaller(vol, iso, v, f)[0] == 0
    if name in ('sphere', 'torus'):
        chi, sv, n_comp = R.euler(v, f), R.signed_volume(v, f), len(np.unique(R.face_labels(f)))
        lo, hi = R.sphere_volume_bounds(R.SPHERE['R']) if name == 'sphere' else R.torus_volume_bounds(R.TORUS['R'], R.TORUS['r'])
        print(name, 'components', n_comp, 'euler', chi, f'signed volume {sv:.2f} in [{lo:.2f}, {hi:.2f}]')
        assert n_comp == 1 and chi == (2 if name == 'sphere' else 0) and sv > 0 and lo <= sv <= hi
    if name == 'last_cell':
        assert len(v) == 3 and len(f) == 1


def test_marching_cubes_twice_the_same_bits_and_no_crossing(eng):
    vol, iso, _ = volume('33x17x65')
    t = torch.from_numpy(vol).cuda()
    a, b = eng.marching_cubes(t, iso), eng.marching_cubes(t, iso)
    print('two calls:', tuple(a[0].shape), tuple(a[1].shape))
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    for fill in (-1.0, 2.0):
        v, f = eng.marching_cubes(torch.full((3, 4, 5), fill), 0.0)
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    # a NaN is not below: the faces of the corner it replaces, a NaN vertex
    nan = R.pattern_volume(0)
    nan[1, 1, 1] = np.nan
    v, f = eng.marching_cubes(torch.from_numpy(nan), 0.0)
    rv, rf = R.marching_cubes(nan, 0.0)
    assert np.array_equal(f.cpu().numpy(), rf) and np.array_equal(v.cpu().numpy(), rv, equal_nan=True) and torch.isnan(v).any()


def test_marching_cubes_refuses_what_it_cannot_do(eng):
    L, t = eng.lib, torch.zeros(2, 2, 2, device='cuda')
    n = (C.c_int(), C.c_int())
    ptr = C.c_void_p(t.data_ptr())
    out = torch.zeros(16, device='cuda')
    for args, msg in (((ptr, 1, 2, 2, 0.0, None, None, C.byref(n[0]), C.byref(n[1])), 'bad sizes'),
                      ((ptr, 1 << 10, 1 << 10, 1 << 10, 0.0, None, None, C.byref(n[0]), C.byref(n[1])), 'bad sizes'),
                      ((None, 2, 2, 2, 0.0, None, None, C.byref(n[0]), C.byref(n[1])), 'null argument'),
                      ((ptr, 2, 2, 2, float('nan'), None, None, C.byref(n[0]), C.byref(n[1])), 'bad iso'),
                      ((ptr, 2, 2, 2, 0.0, None, None, None, None), 'null argument'),
                      ((ptr, 2, 2, 2, 0.5, C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr()), None, None), 'no size query')):
        assert L.ra_marching_cubes(eng.ctx, *args, eng.stream) != 0
        assert msg in L.ra_last_error().decode(), (msg, L.ra_last_error())
    with pytest.raises(ValueError):
        eng.marching_cubes(torch.zeros(1, 4, 4), 0.0)


# ------------------------------------------------------------------------------------------------ largest component
@functools.lru_cache(None)
def component_case(name):
    if name == 'two_sizes':             # the small one first
        s, b = R.sphere_mesh((20, 0, 0), 3.0), R.sphere_mesh((0, 0, 0), 5.0)
        return np.concatenate([s[0], b[0]]), np.concatenate([s[1], b[1] + len(s[0])])
    if name == 'two_equal':             # the tie goes to the lower face index, whose vertices come second
        a, b = R.sphere_mesh((0, 0, 0), 4.0), R.sphere_mesh((20, 0, 0), 4.0)
        return np.concatenate([b[0], a[0]]), np.concatenate([a[1] + len(b[0]), b[1]])
    if name == 'nested':                # a sphere inside a sphere, faces interleaved
        o, i = R.sphere_mesh((0, 0, 0), 6.0), R.sphere_mesh((0, 0, 0), 2.0)
        v, f = np.concatenate([i[0], o[0]]), np.concatenate([i[1], o[1] + len(i[0])])
        return v, f[np.random.default_rng(0).permutation(len(f))]
    if name == 'vertex_contact':        # two fans that share one vertex only, and a vertex no face refers to
        return (np.arange(24, dtype=np.float32).reshape(8, 3),
                np.array([[0, 1, 2], [0, 2, 3], [0, 4, 5], [0, 5, 6], [0, 6, 4]], np.int32))
    if name == 'random_volume':         # six components, found through marching cubes' own output
        return reference('random')
    if name == 'strip':                 # a chain of 3000 triangles with the lowest index at one end: labels travel the whole way
        n = 3000
        v = np.zeros((n + 2, 3), np.float32)
        v[:, 0] = np.arange(n + 2) // 2
        v[:, 1] = np.arange(n + 2) % 2
        f = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1).astype(np.int32)
        lone = np.array([[0, 0, 0]], np.float32) + 50
        return np.concatenate([lone, lone, lone, v]), np.concatenate([[[0, 1, 2]], f + 3]).astype(np.int32)
    if name == 'shuffled_strip':        # 20 000 triangles in a chain whose face order is random: no order of execution helps a label along
        n = 20000
        v = np.zeros((n + 2, 3), np.float32)
        v[:, 0] = np.arange(n + 2) // 2
        v[:, 1] = np.arange(n + 2) % 2
        f = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1).astype(np.int32)
        return v, f[np.random.default_rng(3).permutation(n)]
    if name == 'empty':
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    raise KeyError(name)


COMPONENT_CASES = ('two_sizes', 'two_equal', 'nested', 'vertex_contact', 'random_volume', 'strip', 'shuffled_strip', 'empty')


@pytest.mark.parametrize('name', COMPONENT_CASES)
def test_largest_component_equals_the_numpy_rule(eng, name):
    v, f = component_case(name)
    rv, rf = R.largest_component(v, f)
    ov, of = eng.largest_component(torch.from_numpy(v), torch.from_numpy(f))
    assert ov.dtype == torch.float32 and of.dtype == torch.int32 and ov.is_cuda and of.is_cuda
    ov, of = ov.cpu().numpy(), of.cpu().numpy()
    readbacks, passes = (eng.lib.ra_mesh_extract_stats(eng.ctx, k) for k in (2, 3))
    print(name, 'read-backs', readbacks, 'label passes that lowered a label', passes, 'of', eng.lib.ra_mcubes_tile(1), end='; ')
    print('in', v.shape, f.shape, 'components', len(np.unique(R.face_labels(f))) if len(f) else 0, 'kept', ov.shape, of.shape, 'reference', rv.shape, rf.shape)
    assert ov.shape == rv.shape and of.shape == rf.shape
    assert np.array_equal(ov.view(np.uint32), rv.view(np.uint32)) and np.array_equal(of, rf)
    if name == 'empty':
        assert ov.shape == (0, 3) and of.shape == (0, 3) and readbacks == 0
    else:       # the passes decide on the device whether they have work: one look at the result, also for the chains
        assert readbacks == 1 and passes < eng.lib.ra_mcubes_tile(1)
    if name == 'strip':
        assert len(of) == 3000


def test_largest_component_refuses_a_face_index_out_of_range(eng):
    v = torch.zeros(4, 3)
    for bad in (4, -1):
        with pytest.raises(RaError, match='face index'):
            eng.largest_component(v, torch.tensor([[0, 1, 2], [1, 2, bad]], dtype=torch.int32))
    ov, of = eng.largest_component(v, torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32))      # the context is fine afterwards
    assert tuple(ov.shape) == (4, 3) and of.cpu().tolist() == [[0, 1, 2], [1, 2, 3]]


def test_extraction_then_component_on_the_device(eng):
    """the two calls chained as the renderer will: two balls in one volume, the larger one comes out, closed, with the ball's topology"""
    n = 24
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing='ij'), -1)
    vol = np.maximum(5.0 - np.linalg.norm(g - [7.3, 8.6, 9.45], axis=-1), 3.0 - np.linalg.norm(g - [18.2, 17.7, 16.4], axis=-1)).astype(np.float32)
    v, f = eng.marching_cubes(torch.from_numpy(vol), 0.0)
    ov, of = eng.largest_component(v, f)
    rv, rf = R.largest_component(*R.marching_cubes(vol, 0.0))
    ov, of = ov.cpu().numpy(), of.cpu().numpy()
    fig = R.mesh_figures(ov, of)
    print('two balls:', tuple(v.shape), tuple(f.shape), '-> kept', ov.shape, of.shape, fig, 'euler', R.euler(ov, of))
    assert np.array_equal(ov.view(np.uint32), rv.view(np.uint32)) and np.array_equal(of, rf)
    assert fig['repeated_directed'] == 0 and fig['unmatched'] == 0 and R.euler(ov, of) == 2 and len(ov) < len(v)
    lo, hi = R.sphere_volume_bounds(5.0)
    assert lo <= R.signed_volume(ov, of) <= hi


# ------------------------------------------------------------------------------------------------ stage A: the scalar volume
VOLUME_DIST_TH = 0.125      # the configuration's (make_cfg('relight').dist_th)
VOLUME_MODES = ('canonical', 'tpose', 'posed')


@functools.lru_cache(None)
def _net():
    from relightableavatar_amd import synthetic
    from relightableavatar_amd.networks import make_network
    cfg = make_cfg('relight')
    sd = synthetic.make_state_dict(0, relight=True, cfg=cfg)
    net = make_network(cfg)
    net.load_state_dict(sd)
    return cfg, sd, net.to('cuda:0').eval()


@functools.lru_cache(None)
def oracle_volume(mode, precision):
    """computed once per (mode, precision) and left unchanged: float32 as the reference runs, and the float64-accumulating oracle"""
    cfg, sd, _ = _net()
    return R.oracle_volume(mode, sd, cfg, VOLUME_DIST_TH, emulate=None if precision == 32 else 'f64acc')


@pytest.mark.parametrize('mode', VOLUME_MODES)
def test_sdf_volume_against_the_oracle(mode):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from frame_stage_ref import parity
    from relightableavatar_amd import synthetic
    cfg, sd, net = _net()
    o32, o64 = oracle_volume(mode, 32), oracle_volume(mode, 64)
    eng = net.set_frame(synthetic.to_device(o32['body'], torch.device('cuda:0')))
    verts = o32['verts'] if mode == 'posed' else None
    fill, pad = -10.0, 10
    assert cfg.dist_th == VOLUME_DIST_TH
    vol = eng.sdf_volume(*o32['axes'], mode, VOLUME_DIST_TH, fill=fill, pad=pad, verts=verts)
    assert eng.lib.ra_mesh_extract_stats(eng.ctx, 0) == 1       # the kept count, read back once
    nx, ny, nz = o32['shape']
    tiles = [eng.lib.ra_mcubes_tile(k) for k in (0, 2)]
    assert tuple(vol.shape) == (nx + 2 * pad, ny + 2 * pad, nz + 2 * pad) and vol.dtype == torch.float32
    assert all(n % 64 for n in (nx, ny, nz)) and all((nx * ny * nz) % t for t in tiles)
    vol = vol.cpu()
    inner = vol[pad:-pad, pad:-pad, pad:-pad].reshape(-1)
    border = R.borderline(o32['t'], VOLUME_DIST_TH)
    share = float(border.double().mean())
    kept, got_kept = o32['kept'], inner != fill
    wrong = int(((got_kept != kept) & ~border).sum())
    outside = vol.clone()
    outside[pad:-pad, pad:-pad, pad:-pad] = fill
    print(mode, (nx, ny, nz), 'kept', int(kept.sum()), 'of', kept.numel(), 'device kept', eng.last_kept, 'borderline share', share, 'decisions that differ', wrong)
    assert share <= 1e-3, 'the oracle alone must stay within 0.1 % of borderline cells: pick another seed or voxel size'
    assert wrong == 0
    assert bool((outside == fill).all()) and bool((inner[~got_kept] == fill).all())            # pad and dropped cells: the fill value exactly
    keep = (kept & ~border)[kept]
    ratio = parity(f'sdf_volume {mode}', inner[kept], o32['values'], o64['values'], keep=keep & got_kept[kept])
    print(mode, 'worst ratio to the float32 oracle\'s own error', ratio)
    flat = eng.sdf_volume(*o32['axes'], mode, VOLUME_DIST_TH, fill=fill, pad=0, verts=verts).cpu()
    assert tuple(flat.shape) == (nx, ny, nz) and torch.equal(flat.reshape(-1).view(torch.int32), inner.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ end to end: Renderer.render
E2E_VOXEL = R.VOLUME_VOXEL
E2E_TH = 0.0        # -sdf = 0: the synthetic weights' field does not reach the configuration's 0.5


def _restated_blend(src, ref, values, K, dtype):
    """sample_utils.py:605-611, 631-646 on a brute-force K-NN"""
    src, ref, values = src.to(dtype), ref.to(dtype), values.to(dtype)
    top = torch.topk((src[:, None] - ref[None]).pow(2).sum(-1), K, dim=-1, largest=False)
    d = top.values.sqrt()
    w = 1 / (d + 1e-8)
    w = w / w.sum(-1, keepdim=True)
    return torch.einsum('nkd,nk->nd', values[top.indices], w)


@pytest.mark.parametrize('switch,mode', [('vis_can_mesh', 'canonical'), ('vis_posed_mesh', 'posed')])
def test_renderer_extracts_a_mesh_end_to_end(switch, mode):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from frame_stage_ref import parity
    from oracle import ra_oracle as O
    from relightableavatar_amd import config, synthetic
    from relightableavatar_amd.base_utils import dotdict
    from relightableavatar_amd.evaluators import mesh_evaluator
    from relightableavatar_amd.networks import make_network
    from relightableavatar_amd.renderer import make_renderer, mesh_renderer
    old = config.active_cfg()
    try:
        cfg = make_cfg('relight', voxel_size=E2E_VOXEL, mesh_th=E2E_TH, **{switch: True})
        sd = synthetic.make_state_dict(0, relight=True, cfg=cfg)
        net = make_network(cfg)
        net.load_state_dict(sd)
        net = net.to('cuda:0').eval()
        renderer = make_renderer(cfg, net)
        assert isinstance(renderer, mesh_renderer.Renderer)
        body = synthetic.make_body(R.VOLUME_SEED, posed=True)
        batch = dotdict(synthetic.to_device(body, torch.device('cuda:0')))
        batch.meta = dotdict(latent_index=torch.tensor([0]), frame_index=torch.tensor([0]), view_index=torch.tensor([0]))
        out = renderer.render(batch)
        v, f = out.verts, out.faces
        assert v.dtype == np.float32 and f.dtype == np.int32 and out.weights.shape == (len(v), cfg.n_bones)
        fig = R.mesh_figures(v, f)
        n_comp = len(np.unique(R.face_labels(f)))
        print(switch, 'verts', v.shape, 'faces', f.shape, fig, 'components', n_comp)
        assert len(f) > 100 and fig['repeated_directed'] == 0 and fig['unmatched'] == 0                     # 3
        assert fig['out_of_range'] == 0 and fig['repeats_in_face'] == 0 and n_comp == 1                    # 5, one component
        # the numpy mesh of the oracle's own volume, through the same steps
        o = R.oracle_volume(mode, sd, cfg, cfg.dist_th)
        bounds = (body['wbounds'] if mode == 'posed' else body['tbounds'])[0].numpy()
        rv, rf = R.marching_cubes(o['volume'].numpy(), E2E_TH)
        rv, rf = R.largest_component(((rv - 10) * np.float32(E2E_VOXEL[0]) + bounds[0]).astype(np.float32), rf)
        onet, fr = O.OracleNet(sd, cfg), O._frame(body)
        decode = (lambda x: onet.sdf_feat(x)[0]) if mode == 'canonical' else (lambda x: O.hdq_sdf(onet, x, fr, cfg.dist_th, smooth_transition=False))
        resid = lambda x: float((-decode(torch.from_numpy(x)).reshape(-1) - E2E_TH).abs().max())
        dev_resid, ref_resid = resid(v), resid(rv)
        print(switch, 'max |-sdf - th| at the vertices: device mesh', dev_resid, 'numpy mesh of the oracle volume', ref_resid, 'ratio', dev_resid / ref_resid)
        assert dev_resid <= 1.1 * ref_resid
        # blend weights against the restated sample_blend_K_closest_points
        ref_verts = o['verts']
        w32 = _restated_blend(torch.from_numpy(v), ref_verts, body['weights'][0], cfg.sample_vert_cnt, torch.float32)
        w64 = _restated_blend(torch.from_numpy(v), ref_verts, body['weights'][0], cfg.sample_vert_cnt, torch.float64)
        parity(f'{switch} weights', out.weights, w32, w64)
        parity(f'{switch} weight row sums', out.weights.sum(-1), w32.sum(-1), w64.sum(-1))
        assert abs(float(out.weights.sum(-1).mean()) - 1) < 1e-5
        assert tuple(out.albedo.shape) == (len(v), 3) and torch.equal(out.roughness.view(torch.int32), out.albedo.view(torch.int32))      # the quirk
        assert out.roughness.data_ptr() != out.albedo.data_ptr() and bool(torch.isfinite(out.albedo).all())
        # albedo against the reference's material_decoder restated on the oracle (mesh_renderer.py:103-114) at the returned vertices.  The
        # features come from the 16-bit-operand full query, so the rule is the project's for these heads (test_gpu_heads.BOUND): the rms
        # error against the float64 chain at most 1.25 x that of the emulated chain (kernel-like sdf_feat, features rounded to f16,
        # emulated_heads).  Features of the wrong points miss it by orders of magnitude
        from test_gpu_heads import BOUND
        from test_oracle_heads_grad import emulated_heads, oracle_heads, rms
        x = torch.from_numpy(v)
        n64, ne = O.OracleNet(sd, cfg, emulate='f64acc'), O.OracleNet(sd, cfg, emulate='f16', kernel_like=True)
        with torch.no_grad():
            if mode == 'canonical':
                c64 = ce = x
            else:       # inference_world_geometry: world -> big pose, then the residual
                big = O.world_to_bigpose(onet, x, fr, cfg.dist_th)
                assert bool(big.mask.all()), 'a vertex outside dist_th of the body'
                c64, ce = big.bpts + n64.residuals(big.bpts, fr.cond), big.bpts + ne.residuals(big.bpts, fr.cond)
            feat64, feat_e = n64.sdf_feat(c64)[1], ne.sdf_feat(ce)[1].half().float()
        theta = net.engine().heads_params()
        a64 = oracle_heads(theta, feat64, dtype=torch.float64, want_grad=False)[0]
        ae = emulated_heads(theta, feat_e, want_grad=False)[0]
        floor, e = rms(ae, a64), rms(out.albedo, a64)
        print(switch, f'albedo at the vertices vs the float64 chain: rms {e:.3e}, floor (emulated chain) {floor:.3e}, ratio {e / floor:.3f}; spread of albedo {float(a64.std()):.3e}')
        assert e <= BOUND * floor, (e, floor)
        ev = mesh_evaluator.Evaluator(generator=torch.Generator(device='cuda').manual_seed(0))
        ev.evaluate({'mesh': out}, {'obj': [(torch.from_numpy(rv), torch.from_numpy(rf.astype(np.int64)))]}, engine=net.engine())
        res = ev.summarize()
        print(switch, 'against the numpy mesh:', res, 'voxel', E2E_VOXEL[0])
        assert res['chamfer'] < E2E_VOXEL[0]
    finally:
        config.set_active_cfg(old)

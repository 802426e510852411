"""ra_set_light_xyz / ra_light_visibility through the C ABI (Engine.set_light_xyz, .light_positions, .light_visibility), the re-shade
op that carries its light positions (relight_utils.reshade(light_xyz=...)) and fitting.fit_heads under the trainer's light-position
noise.  Run with `-m gpu` on an MI355X.

Parity rules are the existing ones, under moved lights:
  * the visibility stage: the bounds tests/test_gpu_parity.py::test_unused_stage_fixtures holds it to at the loaded positions, against
    the reference's own outputs for the same noise (tests/golden/light_noise.npz);
  * the re-shade and its gradient: DESIGN.md section 10's rule (tests/test_oracle_reshade_grad.py) — within 10 x the fp32 oracle's own
    error against the float64 oracle, per output, on the maximum and on the median;
  * everything structural is bit for bit: the public entry against the test hook, row subsets against the full call, a re-traced frame
    against its cached maps, a summed loss against its parts, zero noise against no noise.

Bit for bit on a re-traced frame means on the pixels with acc == 1: the renderer's maps are premultiplied by acc (alpha_output_), the
stage's input is the surface point itself, and (x * acc) / acc is x only up to an ulp.  The pixels left out are printed; at most 5 % of
the hit pixels may be.

Every test prints its figures before it asserts (pytest -s); DESIGN.md section 13 holds the record.
"""
import os

import numpy as np
import pytest
import torch

from relightableavatar_amd import _lib, fitting, relight_utils, synthetic
from relightableavatar_amd.base_utils import dotdict
from relightableavatar_amd.config import make_cfg
from test_oracle_heads_grad import flat, unflat
from test_oracle_light_noise import NOISY, oracle_grads_moved, reshade_case
from test_oracle_reshade_grad import OUTPUTS, assert_within_fp32_spread, errors

pytestmark = pytest.mark.gpu
from oracle import ra_oracle as O      # noqa: E402

T = torch.from_numpy


def build(mode, **kw):
    from relightableavatar_amd.networks import make_network
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    dev = torch.device('cuda:0')
    cfg = make_cfg(mode, **kw)
    net = make_network(cfg)
    net.load_state_dict(synthetic.make_state_dict(0, relight=mode in ('relight', 'novel_light'), cfg=cfg))
    return cfg, net.to(dev).eval(), dev


_engines = {}


def engine(**kw):
    """a relight engine per configuration on the posed body of ops.npz"""
    key = tuple(sorted(kw.items()))
    if key not in _engines:
        cfg, net, dev = build('relight', **kw)
        eng = net.set_frame(synthetic.to_device(synthetic.make_body(0, posed=True), dev))
        _engines[key] = (cfg, net, eng, dev)
    return _engines[key]


@pytest.fixture(scope='module')
def fix(golden):
    return golden('light_noise.npz')


@pytest.fixture(scope='module')
def pts(golden):
    """the 24 surface points of ops.npz's light-visibility case"""
    z = golden('ops.npz')
    return dotdict(surf=T(z['lv_surf']), norm=T(z['lv_norm']), acc=T(z['lv_acc']), bbox=z['lv_bbox'].reshape(-1).tolist())


def moved(net, z, draw):
    xyz0 = net.light_xyz_.detach().float().reshape(-1, 3)
    return xyz0 + T(z[f'draw{draw}.noise']).to(xyz0.device)


def lvis_on(eng, p, dev, **kw):
    out = eng.light_visibility(p.surf.to(dev), p.norm.to(dev), p.acc.to(dev), p.bbox, **kw)
    torch.cuda.synchronize()
    return out


def test_native_symbols_are_loaded():
    cfg, net, eng, dev = engine()
    assert 'librelightableavatar_hip.so' in open('/proc/self/maps').read()
    assert eng.lib.ra_abi_version() == 9
    for name in ('ra_set_light_xyz', 'ra_light_visibility'):
        assert hasattr(eng.lib, name), name


# ---------------------------------------------------------------------------------------------- 1. stage parity under moved lights
@pytest.mark.parametrize('draw', NOISY)
def test_stage_parity_under_moved_lights(fix, pts, draw):
    ref_lvis, ref_ldot = T(fix[f'draw{draw}.lvis']), T(fix[f'draw{draw}.ldot'])      # (512, 24) like ops.npz
    err = lambda a, b: (a.detach().cpu().float() - b).abs()
    cfg, net, eng, dev = engine()
    with eng.light_positions(moved(net, fix, draw)):
        lvis, ldot = lvis_on(eng, pts, dev)
    e = err(lvis.T, ref_lvis)
    cfg2, net2, eng2, _ = engine(trace_precision=2)
    with eng2.light_positions(moved(net2, fix, draw)):
        lvis2, ldot2 = lvis_on(eng2, pts, dev)
    e2 = err(lvis2.T, ref_lvis)
    still = float(err(lvis.T, T(fix['draw0.lvis'])).mean())
    print(f'moved lights, draw {draw}: ldot max {float(err(ldot.T, ref_ldot).max()):.2e}; plain tier lvis mean {float(e.mean()):.2e} max {float(e.max()):.2e} '
          f'within 3e-2: {float((e < 3e-2).float().mean()) * 100:.2f} %; all compensated mean {float(e2.mean()):.2e} max {float(e2.max()):.2e}; '
          f'mean |lvis - lvis at the loaded positions| {still:.2e}')
    assert float(err(ldot.T, ref_ldot).max()) < 1e-5 and float(err(ldot2.T, ref_ldot).max()) < 1e-5
    assert float(lvis.T.cpu()[ref_ldot < -1e-4].abs().max()) == 0.0                        # back-facing lights: exactly 0
    assert float(e.mean()) < 3e-3 and float((e < 3e-2).float().mean()) >= 0.98
    assert float(e2.mean()) < 1e-4 and float(e2.max()) < 1e-3
    assert still > 0.0


# ---------------------------------------------------------------------------------------------- 2. the public entry is the tested stage
def test_public_entry_is_the_tested_stage_and_positions_restore(fix, pts):
    cfg, net, eng, dev = engine()
    eq = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    hook = eng.debug_lvis(pts.surf.to(dev), pts.norm.to(dev), pts.acc.to(dev), pts.bbox)
    first = lvis_on(eng, pts, dev)
    assert eq(first, hook)
    eng.set_light_xyz(moved(net, fix, 1))
    away = lvis_on(eng, pts, dev)
    assert eq(away, eng.debug_lvis(pts.surf.to(dev), pts.norm.to(dev), pts.acc.to(dev), pts.bbox))       # the hook follows the lights too
    assert not torch.equal(away[0], first[0]) and not torch.equal(away[1], first[1])
    eng.set_light_xyz(None)
    assert eq(lvis_on(eng, pts, dev), first)
    with pytest.raises(RuntimeError, match='stop'):
        with eng.light_positions(moved(net, fix, 2)):
            assert not torch.equal(lvis_on(eng, pts, dev)[0], first[0])
            raise RuntimeError('stop')
    assert eq(lvis_on(eng, pts, dev), first)
    # empty calls succeed and write nothing; a wrong number of positions is refused before any launch
    none = eng.light_visibility(pts.surf[:0].to(dev), pts.norm[:0].to(dev), pts.acc[:0].to(dev), pts.bbox)
    assert none[0].shape == (0, 512)
    norows = lvis_on(eng, pts, dev, rows=torch.zeros(0, dtype=torch.int64))
    assert norows[0].shape == (0, 512) and norows[1].shape == (0, 512)
    with pytest.raises(ValueError, match='512 lights'):
        eng.set_light_xyz(torch.zeros(100, 3))
    # a context without a light set
    cfg2, net2, _ = build('anisdf')
    eng2 = net2.set_frame(synthetic.to_device(synthetic.make_body(0, posed=True), dev))
    rc = eng2.lib.ra_set_light_xyz(eng2.ctx, None, eng2.stream)
    assert rc != 0 and b'relight ctx' in eng2.lib.ra_last_error()


# ---------------------------------------------------------------------------------------------- 3. rows
@pytest.mark.parametrize('rows', [[23, 0, 7], [11], list(range(23, -1, -1))])
def test_rows_are_rows_of_the_full_call(fix, pts, rows):
    cfg, net, eng, dev = engine()
    with eng.light_positions(moved(net, fix, 1)):
        full = lvis_on(eng, pts, dev)
        part = lvis_on(eng, pts, dev, rows=torch.tensor(rows))
        part32 = lvis_on(eng, pts, dev, rows=torch.tensor(rows, dtype=torch.int32, device=dev))
    for k in range(2):
        assert part[k].shape == (len(rows), 512)
        assert torch.equal(part[k], full[k][rows]) and torch.equal(part32[k], part[k])


# ---------------------------------------------------------------------------------------------- the 64 x 64 relit frame
def relit_frame(trace_precision=1, light_xyz=None):
    """the frame of tests/test_gpu_heads.py rendered by the sphere-tracing renderer as one chunk with ret_raw and vis_novel_light:
    (cfg, net, eng, batch, maps, probe it was shaded with)"""
    from relightableavatar_amd.renderer import make_renderer
    ref = dict(np.load(os.path.join(os.path.dirname(__file__), 'golden', 'frame_novel.npz')))
    cfg, net, dev = build('relight', vis_novel_light=True, trace_precision=trace_precision)
    H = int(ref['H'])
    batch = synthetic.to_device(synthetic.make_batch(H, H, seed=0, posed=True, crop=int(ref['crop'])), dev)
    assert batch.ray_o.shape[1] <= cfg.render_chunk_size                           # one render chunk
    eng = net.engine()
    if light_xyz is not None:
        eng.set_light_xyz(light_xyz(net))
    maps = make_renderer(cfg, net).render(batch)
    probe = maps.envmap.probe[0].detach().clone()
    return cfg, net, eng, batch, maps, probe


_frames = {}


def frame():
    if 'f' not in _frames:
        _frames['f'] = relit_frame()
    return _frames['f']


def counted(maps):
    """the hit pixels' cached maps as the visibility stage wants them, and which of them have acc == 1"""
    acc = maps.acc_map.reshape(-1)
    hit = acc > 0
    a = acc[hit]
    surf, norm = maps.surf_map.reshape(-1, 3)[hit] / a[:, None], maps.norm_map.reshape(-1, 3)[hit] / a[:, None]
    full = a == 1
    left_out = int((~full).sum())
    print(f'{int(hit.sum())} hit pixels, {left_out} with acc < 1 left out of the bit-for-bit comparison')
    assert int(hit.sum()) >= 64 and left_out <= 0.05 * int(hit.sum())
    return hit, surf.contiguous(), norm.contiguous(), a.contiguous(), full


# ---------------------------------------------------------------------------------------------- 4. re-tracing reproduces the cached maps
@pytest.mark.parametrize('jitter', [False, True])
@pytest.mark.parametrize('trace_precision', [0, 1])
def test_retracing_a_rendered_frame_reproduces_its_cached_maps(fix, trace_precision, jitter):
    cfg, net, eng, batch, maps, probe = relit_frame(trace_precision, (lambda n: moved(n, fix, 2)) if jitter else None)
    try:
        hit, surf, norm, acc, full = counted(maps)
        box = batch.wbounds.detach().reshape(-1).cpu().tolist()                    # as the render left it
        lvis, ldot = eng.light_visibility(surf, norm, acc, box, probe=probe)
        rows = full.nonzero()[:, 0]
        sel = rows[torch.randperm(rows.shape[0], generator=torch.Generator().manual_seed(1)).to(rows.device)][:40]      # a permuted subset
        part = eng.light_visibility(surf, norm, acc, box, probe=probe, rows=sel)
    finally:
        eng.set_light_xyz(None)
    c_lvis, c_ldot = maps.lvis_map.reshape(-1, 512)[hit], maps.ldot_map.reshape(-1, 512)[hit]
    print(f'trace_precision {trace_precision}, jitter {jitter}: max |re-traced - cached| lvis {float((lvis - c_lvis)[full].abs().max()):.1e}, '
          f'ldot {float((ldot - c_ldot)[full].abs().max()):.1e} on {int(full.sum())} pixels; mean lvis {float(c_lvis.mean()):.3f}')
    assert torch.equal(lvis[full], c_lvis[full]) and torch.equal(ldot[full], c_ldot[full])
    assert 0.0 < float(c_lvis[full].mean()) < 1.0                                  # shadowed and lit rays both
    assert torch.equal(part[0], c_lvis[sel]) and torch.equal(part[1], c_ldot[sel])
    if jitter:      # the renderer honoured the override: these are not the maps of the loaded positions
        still = frame()[4]
        assert not torch.equal(maps.lvis_map, still.lvis_map) and not torch.equal(maps.rgb_map, still.rgb_map)


# ---------------------------------------------------------------------------------------------- 5. re-shade and gradient under moved lights
def test_reshade_and_gradient_under_moved_lights(fix):
    name, x, case_cfg = reshade_case(fix)
    cfg, net, eng, dev = engine(**synthetic.RESHADE_GRAD_CASES[name]['cfg'])
    noise = T(fix['draw1.noise'])
    f32, f64 = oracle_grads_moved(case_cfg, x, torch.float32, noise), oracle_grads_moved(case_cfg, x, torch.float64, noise)
    xd = type(x)({k: v.to(dev) for k, v in x.items()})
    before = eng.reshade(xd.ray_o, xd.surf, xd.norm, xd.albedo, xd.rough, xd.lvis, xd.ldot, xd.probes)[0]
    albedo, rough, probes = (t.clone().requires_grad_(True) for t in (xd.albedo, xd.rough, xd.probes))
    rgb = relight_utils.reshade(eng, xd.ray_o, xd.surf, xd.norm, albedo, rough, xd.lvis, xd.ldot, probes, light_xyz=moved(net, fix, 1))
    eng.set_light_xyz(moved(net, fix, 2))          # somebody moves the lights between the forward and the backward
    (rgb * xd.d_rgb).sum().backward()
    got = dict(d_albedo=albedo.grad, d_roughness=rough.grad, d_probe=probes.grad)
    e_rgb = float((rgb.detach().cpu() - T(fix['reshade.rgb'])).abs().max())
    print(f'rgb under moved lights vs the reference: max {e_rgb:.2e}')
    assert e_rgb <= 1e-5
    report = []
    assert_within_fp32_spread(f'kernel {name}, moved lights', got, f32, f64, report=report)
    for k in OUTPUTS:      # against the reference's own numbers: 1 x + 10 x the spread (tests/test_gpu_reshade_grad.py)
        ref = T(fix[f'reshade.{k}'])
        d = float((got[k].cpu() - ref).abs().max()) / float(ref.abs().max())
        bound = 11.0 * errors(f32[k], f64[k])[0]
        print(f'kernel vs reference {name} {k}, moved lights: max {d:.2e} (bound {bound:.2e})')
        assert d <= bound, (k, d, bound)
    # both the forward and the backward left the engine at the loaded positions
    after = eng.reshade(xd.ray_o, xd.surf, xd.norm, xd.albedo, xd.rough, xd.lvis, xd.ldot, xd.probes)[0]
    assert torch.equal(after, before) and float((rgb.detach() - before).abs().max()) > 1e-3
    # light_xyz=None is today's op bit for bit
    a2, r2, p2 = (t.clone().requires_grad_(True) for t in (xd.albedo, xd.rough, xd.probes))
    plain = relight_utils.reshade(eng, xd.ray_o, xd.surf, xd.norm, a2, r2, xd.lvis, xd.ldot, p2)
    assert torch.equal(plain, before)


# ---------------------------------------------------------------------------------------------- 6. key lights follow the lights
def test_key_lights_follow_the_lights(fix, pts):
    cfg, net, eng, dev = engine()
    L = cfg.env_h * cfg.env_w
    sd = synthetic.make_state_dict(0, relight=True, cfg=cfg)
    on = O.OracleNet(sd, cfg)
    lights = synthetic.make_novel_lights(8, 0)
    probes = [O.OracleNet(synthetic.make_state_dict(0, relight=True, cfg=cfg, env='front'), cfg).global_env_map] + [lights[k].probe[0] for k in list(lights)[-2:]]
    xyz = moved(net, fix, 1)
    loaded = on.light_xyz
    try:
        for pr in probes:
            d0 = loaded.reshape(-1, 3) / (loaded.reshape(-1, 3).norm(dim=-1, keepdim=True) + 1e-8)
            w0 = (O.sample_envmap_image(pr, d0).mean(-1) * on.light_area.reshape(-1)).clamp_min(0)
            on.light_xyz = xyz.cpu().reshape(loaded.shape)
            want = O.key_lights(on, [pr], cfg.key_light_share)
            d = on.light_xyz.reshape(-1, 3)
            d = d / (d.norm(dim=-1, keepdim=True) + 1e-8)
            w = (O.sample_envmap_image(pr, d).mean(-1) * on.light_area.reshape(-1)).clamp_min(0)
            smax = w / w.sum()
            on.light_xyz = loaded
            eng.set_key_probes([pr.to(dev)])                      # named before the move ...
            eng.debug_key_lights(L)
            eng.set_light_xyz(xyz)
            with pytest.raises(_lib.RaError):                     # ... and gone after it
                eng.debug_key_lights(L)
            lvis_on(eng, pts, dev, probe=pr.to(dev))
            key, share = eng.debug_key_lights(L)
            eng.set_light_xyz(None)
            assert float((share.cpu() - smax).abs().max()) < 1e-5 * float(smax.max()) + 1e-9
            thr = max(cfg.key_light_share, 4.0 / L)
            clear = (smax - thr).abs() > 1e-5 * thr
            got = key.cpu()
            if int(want.sum()) < 48:
                assert bool((got == want)[clear].all()), (int(got.sum()), int(want.sum()))
            else:
                assert int(got.sum()) == 48 and float(smax[got].min()) >= float(smax[~got].max()) - 1e-7
            # the shares are those of the MOVED lights: at the loaded positions they are other numbers, far outside the tolerance
            moved_by = float((smax - w0 / w0.sum()).abs().max())
            print(f'{int(got.sum())} key lights under the moved lights; largest share {float(smax.max()):.3f}, moved by up to {moved_by:.2e}')
            assert moved_by > 100 * (1e-5 * float(smax.max()) + 1e-9)
    finally:
        on.light_xyz = loaded
        eng.set_light_xyz(None)


# ---------------------------------------------------------------------------------------------- 7. the autograd ordering hazard
def test_summed_loss_backward_runs_every_frame_under_its_own_lights(fix):
    cfg, net, eng, batch, maps, probe0 = frame()
    target = maps.rgb_map.reshape(-1, 3).clone()
    cache = [fitting._frame_cache(eng, cfg, batch, maps, target * s, None, True, retrace=True) for s in (1.0, 0.5)]
    xyz = [moved(net, fix, 1), moved(net, fix, 2)]
    theta0 = unflat(eng.heads_params().cpu().clone())
    for i in (4, 5, 10, 11):
        theta0[i] *= 0.7
    theta0 = flat(theta0).to(eng.device)

    def grads(which):
        theta, probe = theta0.clone().requires_grad_(True), probe0.clone().requires_grad_(True)
        views, shades = zip(*(fitting.step_frame(eng, cache[i], probe, None, xyz[i]) for i in which))
        loss = fitting.heads_loss(eng, list(views), theta, probe, shades=list(shades))
        loss.backward()
        torch.cuda.synchronize()
        return theta.grad.clone(), probe.grad.clone(), float(loss)
    g_a, g_b, g_ab, g_ba = grads([0]), grads([1]), grads([0, 1]), grads([1, 0])
    print(f'losses {g_a[2]:.3e} + {g_b[2]:.3e}; max |d_theta| {float(g_ab[0].abs().max()):.2e}, max |d_probe| {float(g_ab[1].abs().max()):.2e}; '
          f'd_probe of frame A under B\'s lights would differ by {float((g_a[1] - g_b[1]).abs().max()):.2e}')
    assert float(g_a[1].abs().max()) > 0 and float(g_a[0].abs().max()) > 0 and not torch.equal(g_a[1], g_b[1])
    for k in range(2):
        assert torch.equal(g_ab[k], g_a[k] + g_b[k]) and torch.equal(g_ba[k], g_a[k] + g_b[k])


# ---------------------------------------------------------------------------------------------- 8. fit_heads
def perturbed(eng):
    start = unflat(eng.heads_params().cpu().clone())
    for i in (4, 5, 10, 11):          # DESIGN.md section 11's start: the last layers x 0.7
        start[i] *= 0.7
    return flat(start)


def test_fit_heads_zero_noise_is_no_noise(fix):
    cfg, net, eng, batch, maps, probe = frame()
    target = maps.rgb_map.reshape(-1, 3).clone()
    acc = maps.acc_map.reshape(-1)
    mask = acc == 1          # see the module docstring; counted() asserts that at most 5 % of the hit pixels are left out
    counted(maps)
    kw = dict(steps=3, lr=1e-3, fit_probe=False, probe_init=probe, theta_init=perturbed(eng))
    plain = fitting.fit_heads(net, [(batch, maps, target, mask)], **kw)
    zero = fitting.fit_heads(net, [(batch, maps, target, mask)], light_noise_fn=lambda step, frame: torch.zeros(512, 3, device=eng.device), **kw)
    print(f'loss history without noise {plain.loss}, with zero noise {zero.loss}')
    assert zero.loss == plain.loss and torch.equal(zero.theta, plain.theta)
    reg = fitting.fit_heads(net, [(batch, maps, target, mask)], regularisers=True, generator=torch.Generator().manual_seed(5), **kw)
    reg0 = fitting.fit_heads(net, [(batch, maps, target, mask)], regularisers=True, generator=torch.Generator().manual_seed(5), light_noise=0.0, **kw)
    assert reg0.loss == reg.loss and torch.equal(reg0.theta, reg.theta) and reg0.terms == reg.terms


def test_fit_heads_first_loss_is_the_loss_assembled_by_hand(fix):
    cfg, net, eng, batch, maps, probe = frame()
    dev = eng.device
    target = maps.rgb_map.reshape(-1, 3).clone()
    theta = perturbed(eng).to(dev)
    noise = T(fix['draw2.noise']).to(dev)
    n_hit = int((maps.acc_map.reshape(-1) > 0).sum())
    rows = torch.randperm(n_hit, generator=torch.Generator().manual_seed(3))[:32].to(dev)
    fit = fitting.fit_heads(net, [(batch, maps, target, None)], steps=1, lr=1e-3, fit_probe=False, probe_init=probe, theta_init=theta,
                            light_noise_fn=lambda step, frame: noise * (step + 1), pixels_per_step=32, pixel_fn=lambda step, frame, n: rows)
    with torch.no_grad():
        c = fitting._frame_cache(eng, cfg, batch, maps, target, None, True, retrace=True)
        assert c.w.shape[0] == n_hit
        pr = torch.nn.functional.softplus(fitting._inv_softplus(probe.clamp_min(1e-6)))
        xyz = moved(net, fix, 2)
        with eng.light_positions(xyz):
            lvis, ldot = eng.light_visibility(c.surf_pts, c.norm_pts, c.acc, c.bbox, probe=pr, rows=rows)
        scale = c.scale[rows]
        view = dotdict(w=c.w[rows], bg=c.bg[rows], scale=scale, S=c.S)
        feat = c.feat.reshape(n_hit, c.S, 256)[rows].reshape(-1, 256)
        albedo, rough = fitting.composite_heads(cfg, view, *relight_utils.material_heads(eng, theta, feat))
        rgb = relight_utils.reshade(eng, c.ray_o[rows], c.surf[rows], c.norm[rows], albedo, rough, lvis * scale[:, None], ldot * scale[:, None], pr[None],
                                    light_xyz=xyz)[0]
        by_hand = float(torch.nn.functional.mse_loss(rgb, c.target[rows]))
    print(f'fit_heads loss[0] {fit.loss[0]!r}, by hand {by_hand!r}')
    assert len(fit.loss) == 2 and fit.loss[0] == by_hand
    assert not torch.equal(fit.theta, theta)


def test_fit_heads_under_noise_lowers_the_noise_free_loss_and_restores_the_lights(fix, pts):
    cfg, net, eng, batch, maps, probe = frame()
    dev = eng.device
    target = maps.rgb_map.reshape(-1, 3).clone()
    hook = lambda: eng.debug_lvis(pts.surf.to(dev), pts.norm.to(dev), pts.acc.to(dev), pts.bbox)
    eng.set_frame(batch)
    before = hook()
    frames = [(batch, maps, target, None)]
    start = perturbed(eng)
    noise_free = lambda theta: fitting.fit_heads(net, frames, steps=0, lr=1e-3, fit_probe=False, probe_init=probe, theta_init=theta).loss[0]
    loss0 = noise_free(start)
    fit = fitting.fit_heads(net, frames, steps=20, lr=1e-3, fit_probe=False, probe_init=probe, theta_init=start, light_noise=True,
                            generator=torch.Generator().manual_seed(0))
    loss1 = noise_free(fit.theta)
    print(f'20 Adam steps under light noise std {cfg.light_xyz_noise_std}: noise-free image loss {loss0:.3e} -> {loss1:.3e}; noisy history {fit.loss[0]:.3e} -> {fit.loss[-1]:.3e}')
    assert len(fit.loss) == 21 and np.isfinite(fit.loss).all()
    assert loss1 < loss0
    after = hook()
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])

    def failing(step, frame):
        if step == 1:
            raise RuntimeError('no noise today')
        return T(fix['draw1.noise']).to(dev)
    with pytest.raises(RuntimeError, match='no noise today'):
        fitting.fit_heads(net, frames, steps=3, lr=1e-3, fit_probe=False, probe_init=probe, theta_init=start, light_noise_fn=failing)
    after = hook()
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])

"""ra_reshade_backward (csrc/ra_shade_bwd.hip) through the C ABI, the autograd op on top of it (relight_utils.reshade) and the
fitting entry point (fitting.fit_relight).  Run with `-m gpu` on an MI355X.

Parity rule (tests/test_oracle_reshade_grad.py states and implements it): no tolerance is chosen in advance.  The oracle is evaluated
in float64 and in float32 on the same inputs; per output, the kernel's max |diff| / max |ref| and median |diff| / max |ref| against the
float64 oracle may be at most 10 x the float32 oracle's own error against float64.  Every element is inside the bound.  The margin
covers libm-versus-device acosf / atan2f / powf and the order of the sums.  Both roughness ranges are tested: over the full range
[0.09, 0.99] a few grazing, low-roughness pixels dominate a gradient's maximum, in fp32 as in the kernel.

Every test prints its figures before it asserts (pytest -s); DESIGN.md section 10 holds the record.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from relightableavatar_amd import _lib, fitting, relight_utils, synthetic
from relightableavatar_amd.config import make_cfg
from test_oracle_reshade_grad import CASES, OUTPUTS, assert_within_fp32_spread, case_inputs, errors, lights, oracle_grads

pytestmark = pytest.mark.gpu
from oracle import ra_oracle as O      # noqa: E402


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
    """a relight engine per configuration (lambert_only / glossy_only live in the ctx config)"""
    key = tuple(sorted(kw.items()))
    if key not in _engines:
        cfg, net, dev = build('relight', **kw)
        eng = net.set_frame(synthetic.to_device(synthetic.make_body(0, posed=True), dev))
        _engines[key] = (cfg, net, eng, dev)
    return _engines[key]


def backward(eng, x, **kw):
    da, dr, dp = eng.reshade_backward(x.ray_o, x.surf, x.norm, x.albedo, x.rough, x.lvis, x.ldot, x.probes, x.d_rgb, **kw)
    torch.cuda.synchronize()
    return dict(d_albedo=da, d_roughness=dr, d_probe=dp)


def raw_call(eng, x, d_alb, d_rgh, d_prb, **override):
    """the C call itself on device tensors; override: argument name -> tensor or None"""
    a = dict(ray_o=x.ray_o, surf=x.surf, norm=x.norm, albedo=x.albedo, rough=x.rough, lvis=x.lvis, ldot=x.ldot, probes=x.probes, d_rgb=x.d_rgb)
    a.update(override)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    n, ph, pw = x.probes.shape[:3]
    rc = eng.lib.ra_reshade_backward(eng.ctx, p(a['ray_o']), p(a['surf']), p(a['norm']), p(a['albedo']), p(a['rough']), p(a['lvis']), p(a['ldot']),
                                     x.ray_o.shape[0], p(a['probes']), n, ph, pw, p(a['d_rgb']), p(d_alb), p(d_rgh), p(d_prb), eng.stream)
    _lib.check(rc, 'ra_reshade_backward')
    torch.cuda.synchronize()


def test_native_symbol_is_loaded():
    cfg, net, eng, dev = engine()
    assert 'librelightableavatar_hip.so' in open('/proc/self/maps').read()
    assert eng.lib.ra_abi_version() == 9 and hasattr(eng.lib, 'ra_reshade_backward')


# ---------------------------------------------------------------------------------------------- 1. the reference's fixture
@pytest.mark.parametrize('name', CASES)
def test_parity_with_the_reference_fixture(golden, name):
    z = golden('reshade_grad.npz')
    x = case_inputs(z, name)
    kw = synthetic.RESHADE_GRAD_CASES[name]['cfg']
    cfg, net, eng, dev = engine(**kw)
    f32, f64 = oracle_grads(cfg, x, torch.float32), oracle_grads(cfg, x, torch.float64)
    xd = type(x)({k: v.to(dev) for k, v in x.items()})
    got = backward(eng, xd)
    rgb = eng.reshade(xd.ray_o, xd.surf, xd.norm, xd.albedo, xd.rough, xd.lvis, xd.ldot, xd.probes)[0]
    assert float((rgb.cpu() - torch.from_numpy(z[f'{name}.rgb'])).abs().max()) <= 1e-5
    assert_within_fp32_spread(f'kernel {name}', got, f32, f64)
    # ... and against the reference's own numbers: it is one fp32 evaluation (within 1 x the spread of float64, as the CPU test
    # shows to 10 x), the kernel another (10 x): 11 x by the triangle inequality
    for k in OUTPUTS:
        ref = torch.from_numpy(z[f'{name}.{k}'])
        if float(ref.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, (name, k)
            continue
        d = float((got[k].cpu() - ref).abs().max()) / float(ref.abs().max())
        bound = 11.0 * errors(f32[k], f64[k])[0]
        print(f'kernel vs reference {name} {k}: max {d:.2e} (bound {bound:.2e})')
        assert d <= bound, (name, k, d, bound)


# ---------------------------------------------------------------------------------------------- 2. a large random case
def linear_test_inputs(P=5000):
    """the inputs of test_gpu_parity.test_reshade_is_linear_in_the_probe (same generator, same order of draws), roughness mapped to the
    conditioned range, two of its probes, and a d_rgb"""
    g = torch.Generator().manual_seed(3)
    ro = torch.randn(P, 3, generator=g) + torch.tensor([0.0, 0.0, -2.0])
    surf = torch.rand(P, 3, generator=g) - 0.5
    nrm = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    alb, rgh = torch.rand(P, 3, generator=g), torch.rand(P, generator=g) * 0.69 + 0.3
    lvis, ldot = torch.rand(P, 512, generator=g), torch.rand(P, 512, generator=g) * 2 - 1
    p1, p2 = torch.rand(16, 32, 3, generator=g), torch.rand(16, 32, 3, generator=g) * 3
    d_rgb = torch.randn(2, P, 3, generator=g)
    return synthetic.dotdict(ray_o=ro, surf=surf, norm=nrm, albedo=alb, rough=rgh, lvis=lvis, ldot=ldot,
                                                                probes=torch.stack([p1, p2]), d_rgb=d_rgb)


def oracle_grads_chunked(cfg, x, dtype, chunk=1250):
    """oracle_grads over pixel chunks (the oracle holds (L, P, 3) tensors): d_probe sums over the chunks in float64"""
    P = x.ray_o.shape[0]
    da, dr, dp = [], [], torch.zeros(x.probes.shape, dtype=torch.float64)
    for a in range(0, P, chunk):
        sub = type(x)({k: (v[:, a:a + chunk] if k == 'd_rgb' else (v if k == 'probes' else v[a:a + chunk])) for k, v in x.items()})
        g = oracle_grads(cfg, sub, dtype)
        da.append(g['d_albedo']), dr.append(g['d_roughness'])
        dp += g['d_probe'].double()
    return dict(d_albedo=torch.cat(da), d_roughness=torch.cat(dr), d_probe=dp.to(dtype))


def test_large_random_case_against_the_oracle():
    cfg, net, eng, dev = engine()
    x = linear_test_inputs()
    f32, f64 = oracle_grads_chunked(cfg, x, torch.float32), oracle_grads_chunked(cfg, x, torch.float64)
    got = backward(eng, type(x)({k: v.to(dev) for k, v in x.items()}))
    assert_within_fp32_spread('kernel P=5000', got, f32, f64)


# ---------------------------------------------------------------------------------------------- 3. structure
def test_ten_probes_are_two_launches():
    """each probe's d_probes does not depend on its neighbours in the call (bit for bit); d_albedo / d_roughness sum over the probes"""
    cfg, net, eng, dev = engine()
    x = synthetic.make_reshade_inputs(50, 512, n_probes=10, rough=(0.3, 0.99))
    x.probes = x.probes * torch.linspace(0.3, 2.0, 10)[:, None, None, None]
    f32, f64 = oracle_grads(cfg, x, torch.float32), oracle_grads(cfg, x, torch.float64)
    xd = type(x)({k: v.to(dev) for k, v in x.items()})
    got = backward(eng, xd)
    one = []
    for q in range(10):
        xq = type(x)(dict(xd, probes=xd.probes[q:q + 1].contiguous(), d_rgb=xd.d_rgb[q:q + 1].contiguous()))
        one.append(backward(eng, xq))
        assert torch.equal(one[-1]['d_probe'][0], got['d_probe'][q]), q
    summed = dict(d_albedo=sum(o['d_albedo'] for o in one), d_roughness=sum(o['d_roughness'] for o in one), d_probe=got['d_probe'])
    assert_within_fp32_spread('10 probes', got, f32, f64)
    assert_within_fp32_spread('10 one-probe calls, summed', summed, f32, f64)
    for k in ('d_albedo', 'd_roughness'):
        d = float((got[k] - summed[k]).abs().max()) / float(f64[k].abs().max())
        assert d <= 10.0 * errors(f32[k], f64[k])[0], (k, d)


def test_ablation_switches_give_exact_zeros():
    x = synthetic.reshade_case_inputs('default_full')
    for kw, zero, live in (({'glossy_only': True}, 'd_albedo', 'd_roughness'), ({'lambert_only': True}, 'd_roughness', 'd_albedo')):
        cfg, net, eng, dev = engine(**kw)
        got = backward(eng, type(x)({k: v.to(dev) for k, v in x.items()}))
        assert float(got[zero].abs().max()) == 0.0 and float(got[live].abs().max()) > 0.0 and float(got['d_probe'].abs().max()) > 0.0


def test_clipped_pixels_get_no_gradient():
    """lin > 1: the tone map's clip passes nothing — per channel for d_albedo and the probe, per pixel for d_roughness"""
    cfg, net, eng, dev = engine()
    x = synthetic.reshade_case_inputs('bright')
    lin_cfg = make_cfg('relight', tonemapping_rendering=False)
    lin = O.shade_pixels(lights(lin_cfg, torch.float64), x.probes[0].double(), x.ray_o.double(), x.surf.double(), x.norm.double(), x.albedo.double(),
                         x.rough.double()[:, None], x.lvis.double().T, x.ldot.double().T, main_pass=False)[0]
    over = lin > 1.001                    # clearly over, in any fp32 arithmetic
    assert int(over.sum()) > 50 and int(over.all(-1).sum()) >= 8 and int((lin < 0.999).sum()) > 20
    xd = type(x)({k: v.to(dev) for k, v in x.items()})
    got = backward(eng, xd)
    assert float(got['d_albedo'].cpu()[over].abs().max()) == 0.0
    assert float(got['d_roughness'].cpu()[over.all(-1)].abs().max()) == 0.0
    assert float(got['d_albedo'].cpu()[lin < 0.999].abs().min()) > 0.0
    # only the unclipped (pixel, channel) pairs reach the probe: the same call with d_rgb zeroed there gives a zero probe gradient
    xz = type(x)(dict(xd, d_rgb=(xd.d_rgb * over.to(dev)[None]).contiguous()))
    assert float(backward(eng, xz)['d_probe'].abs().max()) == 0.0


def test_null_outputs_and_empty_calls():
    cfg, net, eng, dev = engine()
    x = synthetic.reshade_case_inputs('two_probes')
    xd = type(x)({k: v.to(dev) for k, v in x.items()})
    full = backward(eng, xd)
    for i, k in enumerate(OUTPUTS):          # one output at a time, the others NULL: the same bits
        only = backward(eng, xd, want=tuple(j == i for j in range(3)))
        assert torch.equal(only[k], full[k]) and all(only[o] is None for o in OUTPUTS if o != k)
    raw_call(eng, xd, None, None, None)      # nothing wanted: accepted
    # P = 0 and n_probes = 0 write nothing
    sent = [torch.full((96, 3), 7.0, device=dev), torch.full((96,), 7.0, device=dev), torch.full((2, 16, 32, 3), 7.0, device=dev)]
    e0 = type(x)({k: (v[:, :0] if k == 'd_rgb' else (v if k == 'probes' else v[:0])).contiguous() for k, v in xd.items()})
    raw_call(eng, e0, *sent)
    n0 = type(x)(dict(xd, probes=xd.probes[:0].contiguous(), d_rgb=xd.d_rgb[:0].contiguous()))
    raw_call(eng, n0, *sent)
    assert all(float((s - 7.0).abs().max()) == 0.0 for s in sent)


def test_bad_arguments_raise():
    cfg, net, eng, dev = engine()
    x = synthetic.reshade_case_inputs('default')
    xd = type(x)({k: v.to(dev) for k, v in x.items()})
    outs = [torch.zeros(96, 3, device=dev), torch.zeros(96, device=dev), torch.zeros(1, 16, 32, 3, device=dev)]
    for k in ('ray_o', 'surf', 'norm', 'albedo', 'rough', 'lvis', 'ldot', 'probes', 'd_rgb'):
        with pytest.raises(_lib.RaError, match='null input'):
            raw_call(eng, xd, *outs, **{k: None})
    big = type(x)(dict(xd, probes=torch.zeros(1, 64, 128, 3, device=dev)))      # 96 KB: no LDS tile for it
    with pytest.raises(_lib.RaError, match='LDS'):
        raw_call(eng, big, outs[0], outs[1], torch.zeros(1, 64, 128, 3, device=dev))
    cfg2, net2, dev2 = build('anisdf')
    eng2 = net2.set_frame(synthetic.to_device(synthetic.make_body(0, posed=True), dev2))
    with pytest.raises(_lib.RaError, match='relight ctx'):
        eng2.reshade_backward(xd.ray_o, xd.surf, xd.norm, xd.albedo, xd.rough, xd.lvis, xd.ldot, xd.probes, xd.d_rgb)


def test_two_identical_calls_are_bit_identical():
    """all three outputs: every sum of the kernel has a fixed order (the header comment of ra_shade_bwd.hip says how)"""
    cfg, net, eng, dev = engine()
    x = synthetic.make_reshade_inputs(51, 3000, n_probes=3, rough=(0.09, 0.99))
    xd = type(x)({k: v.to(dev) for k, v in x.items()})
    a = backward(eng, xd)
    other = backward(eng, type(x)(dict(xd, d_rgb=(xd.d_rgb * 2).contiguous())))      # something else in between, in the same scratch
    b = backward(eng, xd)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), k
        assert not torch.equal(a[k], other[k])


# ---------------------------------------------------------------------------------------------- 4. the autograd op
def test_autograd_op():
    cfg, net, eng, dev = engine()
    x = synthetic.reshade_case_inputs('two_probes')
    xd = type(x)({k: v.to(dev) for k, v in x.items()})
    albedo, rough, probes = (t.clone().requires_grad_(True) for t in (xd.albedo, xd.rough, xd.probes))
    others = [t.clone().requires_grad_(True) for t in (xd.ray_o, xd.surf, xd.norm, xd.lvis, xd.ldot)]
    rgb = relight_utils.reshade(eng, others[0], others[1], others[2], albedo, rough, others[3], others[4], probes)
    assert torch.equal(rgb.detach(), eng.reshade(xd.ray_o, xd.surf, xd.norm, xd.albedo, xd.rough, xd.lvis, xd.ldot, xd.probes)[0])
    rgb.backward(xd.d_rgb)
    want = backward(eng, xd)
    assert torch.equal(albedo.grad, want['d_albedo']) and torch.equal(rough.grad, want['d_roughness']) and torch.equal(probes.grad, want['d_probe'])
    assert all(t.grad is None for t in others)
    # a (P, 1) roughness as the renderer's roughness_map has it, and only the probe wanting a gradient
    probes2 = xd.probes.clone().requires_grad_(True)
    relight_utils.reshade(eng, xd.ray_o, xd.surf, xd.norm, xd.albedo, xd.rough[:, None], xd.lvis, xd.ldot, probes2).backward(xd.d_rgb)
    assert torch.equal(probes2.grad, want['d_probe'])


# ---------------------------------------------------------------------------------------------- 5. fitting
def known_probe():
    probe = torch.full((16, 32, 3), 0.15)          # dim ambient + one bright patch
    probe[5:8, 10:14] = 6.0
    return probe


def test_fit_relight_recovers_the_light_like_the_oracle_loop():
    """100 Adam steps from the reference's initialisation on P = 256 random maps, on the GPU through fit_relight and on the CPU through
    the oracle's autograd, same parametrisation, same initial parameter.  Measured on the CPU (lr 5e-2): loss 4.6e-3 -> 1.7e-4."""
    cfg, net, eng, dev = engine()
    x = synthetic.make_reshade_inputs(52, 256, rough=(0.3, 0.99))
    steps, lr = 100, 5e-2
    o_net = lights(cfg, torch.float32)
    shade = lambda probe: O.shade_pixels(o_net, probe, x.ray_o, x.surf, x.norm, x.albedo, x.rough[:, None], x.lvis.T, x.ldot.T, main_pass=False)[0]
    with torch.no_grad():
        target = shade(known_probe())
    init = fitting.init_probe_param(cfg, generator=torch.Generator().manual_seed(0))
    # the oracle loop
    param = init.clone().requires_grad_(True)
    opt = torch.optim.Adam([param], lr=lr)
    o_loss = []
    for _ in range(steps):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(shade(torch.nn.functional.softplus(param.expand(*param.shape[:2], 3))), target)
        loss.backward()
        opt.step()
        o_loss.append(float(loss))
    with torch.no_grad():
        o_loss.append(float(torch.nn.functional.mse_loss(shade(torch.nn.functional.softplus(param.expand(*param.shape[:2], 3))), target)))
    # the product
    maps = synthetic.dotdict(ray_o=x.ray_o, surf_map=x.surf, norm_map=x.norm, albedo_map=x.albedo, roughness_map=x.rough,
                                                                lvis_map=x.lvis, ldot_map=x.ldot)
    fit = fitting.fit_relight(eng, maps, target, steps=steps, lr=lr, generator=torch.Generator().manual_seed(0))
    print(f'fit_relight: loss {fit.loss[0]:.3e} -> {fit.loss[-1]:.3e}; oracle loop {o_loss[0]:.3e} -> {o_loss[-1]:.3e}')
    assert len(fit.loss) == steps + 1 and fit.probe.shape == (cfg.env_h * cfg.envmap_upscale, cfg.env_w * cfg.envmap_upscale, 3)
    assert abs(fit.loss[0] - o_loss[0]) <= 1e-3 * o_loss[0]
    assert fit.loss[-1] <= 1.1 * o_loss[-1], (fit.loss[-1], o_loss[-1])
    assert fit.loss[-1] < 0.1 * fit.loss[0], (fit.loss[0], fit.loss[-1])


def test_fit_relight_materials():
    """albedo and roughness under their sigmoid parametrisation: the fit starts at the maps' values and moves towards the target's.
    The same loop through the oracle's autograd on the CPU: loss 1.1e-3 -> 7.9e-7 in 60 steps, mean |albedo error| 0.079 -> 0.007."""
    cfg, net, eng, dev = engine()
    x = synthetic.make_reshade_inputs(53, 256, rough=(0.3, 0.9))
    xd = type(x)({k: v.to(dev) for k, v in x.items()})
    probe = known_probe().to(dev) + 0.3
    target = eng.reshade(xd.ray_o, xd.surf, xd.norm, xd.albedo, xd.rough, xd.lvis, xd.ldot, probe[None])[0][0]
    off = synthetic.dotdict(ray_o=x.ray_o, surf_map=x.surf, norm_map=x.norm, albedo_map=(x.albedo * 0.7 + 0.1),
                                                               roughness_map=(x.rough * 0.8 + 0.1)[:, None], lvis_map=x.lvis, ldot_map=x.ldot)
    fit = fitting.fit_relight(eng, off, target, steps=60, lr=5e-2, fit_probe=False, fit_albedo=True, fit_roughness=True, probe_init=probe)
    assert torch.allclose(fit.probe, probe, rtol=1e-5, atol=1e-6)
    assert fit.loss[-1] < 0.1 * fit.loss[0], (fit.loss[0], fit.loss[-1])
    assert float((fit.albedo_map - xd.albedo).abs().mean()) < float((off.albedo_map.to(dev) - xd.albedo).abs().mean())


# ---------------------------------------------------------------------------------------------- 6. a whole frame
def test_whole_frame_maps(golden):
    """the op on the maps the novel-light renderer really returns (their shapes, their (P, L) layout)"""
    from relightableavatar_amd.renderer import make_renderer
    ref = golden('frame_novel.npz')
    cfg, net, dev = build('novel_light')
    H = int(ref['H'])
    batch = synthetic.to_device(synthetic.make_batch(H, H, seed=0, posed=True, crop=int(ref['crop']), n_novel_lights=3), dev)
    out = make_renderer(cfg, net).render(batch)
    eng = net.engine()
    maps = out['probe00']
    probe = batch.novel_lights['probe00'].probe
    probe = (probe[0] if probe.ndim == 4 else probe).to(dev).float()
    target = maps.rgb_map.reshape(-1, 3)
    hit = maps.acc_map.reshape(-1) > 0
    assert int(hit.sum()) >= 64
    # from the true probe the loss is zero up to the softplus round trip of the parametrisation
    fit = fitting.fit_relight(eng, maps, target, steps=3, lr=1e-6, probe_init=probe)
    assert fit.loss[0] <= 1e-10 and all(np.isfinite(fit.loss)), fit.loss
    # ... and the gradient there is fp32 noise.  The loss gradient is linear in the residual rgb - target: a target that is off by
    # 1e-3 everywhere has a residual 1e4 x the 1e-7 of fp32's rgb, so the gradient at the optimum is below 1e-3 of that one (10 x margin)
    def grad_norm(tgt):
        p = probe.clone().requires_grad_(True)
        rgb = relight_utils.reshade(eng, maps.ray_o, maps.surf_map, maps.norm_map, maps.albedo_map, maps.roughness_map, maps.lvis_map, maps.ldot_map, p[None])[0]
        torch.nn.functional.mse_loss(rgb, tgt).backward()
        return float(p.grad.norm())
    g0, g1 = grad_norm(target), grad_norm(target + 1e-3)
    print(f'whole frame: |grad| at the optimum {g0:.3e}, with the target off by 1e-3 {g1:.3e}')
    assert g1 > 0 and g0 <= 1e-3 * g1, (g0, g1)
    # the gradients themselves on a 64-pixel subset of the hit pixels against the oracle on the same maps
    idx = torch.nonzero(hit)[:64, 0]
    sub = lambda t, *s: t.reshape(*s)[idx].contiguous()
    g = torch.Generator().manual_seed(7)
    x = synthetic.dotdict(
        ray_o=sub(maps.ray_o, -1, 3), surf=sub(maps.surf_map, -1, 3), norm=sub(maps.norm_map, -1, 3), albedo=sub(maps.albedo_map, -1, 3),
        rough=sub(maps.roughness_map, -1), lvis=sub(maps.lvis_map, target.shape[0], -1), ldot=sub(maps.ldot_map, target.shape[0], -1),
        probes=probe[None].contiguous(), d_rgb=torch.randn(1, 64, 3, generator=g).to(dev))
    assert x.lvis.shape == (64, cfg.env_h * cfg.env_w)
    got = backward(eng, x)
    f32, f64 = oracle_grads(cfg, x, torch.float32), oracle_grads(cfg, x, torch.float64)
    assert_within_fp32_spread('whole frame, 64 hit pixels', got, f32, f64)

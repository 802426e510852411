"""ra_heads_forward / ra_heads_backward (csrc/ra_heads.hip) through the C ABI, the autograd op on top of them
(relight_utils.material_heads), ra_bigpose_features and the fitting entry point (fitting.fit_heads).  Run with `-m gpu` on an MI355X.

Parity rule.  The kernels round their MFMA operands to f16; what that costs is measured, not chosen: floor = rms(emulation - float64) on
the same inputs, the emulation being the per-layer operand rounding of tests/test_oracle_heads_grad.py.  The kernel may be at most
1.25 x the floor from float64 — the project's bound for these heads inside K4 (PARITY['albedo+rough'] of test_gpu_parity.py).  Gradients
are measured per head on the pooled, per-tensor-normalised errors (test_oracle_heads_grad.pooled_errors); per-tensor ratios are printed.
Measured on the CPU: forward floor rms 9.3e-6 (fp32: 2.5e-8), gradient floor 3e-5 .. 5e-4 of max |g| per tensor (fp32: 1e-7).

Every test prints its figures before it asserts (pytest -s); DESIGN.md section 11 holds the record.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from relightableavatar_amd import _lib, fitting, relight_utils, synthetic
from relightableavatar_amd.config import make_cfg
from test_oracle_heads_grad import (HEAD_KEYS, HEADS, KINDS, N_FIXTURE, N_PARAMS, case, emulated_heads, flat, heads_cfg, oracle_heads, pooled_rms, rms,
                                    tensor_ratios, unflat)

pytestmark = pytest.mark.gpu
from oracle import ra_oracle as O      # noqa: E402

BOUND = 1.25
A_SIZE = 49795          # floats of the albedo head in theta; the roughness head is the rest


def build(mode, **kw):
    from relightableavatar_amd.networks import make_network
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    dev = torch.device('cuda:0')
    cfg = make_cfg(mode, **kw)
    net = make_network(cfg)
    net.load_state_dict(synthetic.make_state_dict(0, relight=mode in ('relight', 'novel_light'), cfg=cfg))
    return cfg, net.to(dev).eval(), dev


_engine = []


def engine():
    if not _engine:
        cfg, net, dev = build('relight')
        eng = net.set_frame(synthetic.to_device(synthetic.make_body(0, posed=True), dev))
        _engine.append((cfg, net, eng, dev))
    return _engine[0]


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def raw_backward(eng, theta, feat, d_albedo, d_rough, d_theta, n=None):
    rc = eng.lib.ra_heads_backward(eng.ctx, p(theta), p(feat), feat.shape[0] if n is None else n, p(d_albedo), p(d_rough), p(d_theta), eng.stream)
    _lib.check(rc, 'ra_heads_backward')
    torch.cuda.synchronize()


def raw_forward(eng, theta, feat, albedo, rough, n=None):
    rc = eng.lib.ra_heads_forward(eng.ctx, p(theta), p(feat), feat.shape[0] if n is None else n, p(albedo), p(rough), eng.stream)
    _lib.check(rc, 'ra_heads_forward')
    torch.cuda.synchronize()


def cat4(albedo, rough):
    return torch.cat([albedo.detach().cpu().double().reshape(-1, 3), rough.detach().cpu().double().reshape(-1, 1)], 1)


# ---------------------------------------------------------------------------------------------- 1. symbols
def test_native_symbols_are_loaded():
    cfg, net, eng, dev = engine()
    assert 'librelightableavatar_hip.so' in open('/proc/self/maps').read()
    assert eng.lib.ra_abi_version() == 9
    for name in ('ra_heads_param_count', 'ra_heads_get_params', 'ra_heads_forward', 'ra_heads_backward', 'ra_bigpose_features'):
        assert hasattr(eng.lib, name), name
    assert eng.heads_param_count() == N_PARAMS
    sd = synthetic.make_state_dict(0, relight=True, cfg=cfg)
    assert torch.equal(eng.heads_params().cpu(), flat([sd[k].float() for k in HEAD_KEYS]))


# ---------------------------------------------------------------------------------------------- 2. forward parity
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', [1, 191, 192, 1536])
def test_forward_parity(golden, kind, n):
    cfg, net, eng, dev = engine()
    c = case(kind, n)
    albedo, rough = eng.heads_forward(c['theta'].to(dev), c['feat'].to(dev))
    ref, emu, got = cat4(c['albedo64'], c['rough64']), cat4(c['albedo_emu'], c['rough_emu']), cat4(albedo, rough)
    floor, e = rms(emu, ref), rms(got, ref)
    print(f'forward {kind} n = {n}: kernel vs float64 rms {e:.3e}, floor {floor:.3e}, ratio {e / floor:.3f}')
    assert torch.isfinite(got).all() and e <= BOUND * floor, (e, floor)
    if n == N_FIXTURE:      # the reference's own outputs (an fp32 evaluation: 2.5e-8 from float64, far below the floor)
        z = golden('heads_grad.npz')
        e = rms(got, cat4(torch.from_numpy(z[f'{kind}.albedo']), torch.from_numpy(z[f'{kind}.rough'])))
        print(f'forward {kind}: kernel vs the reference fixture rms {e:.3e}')
        assert e <= BOUND * floor, (e, floor)


# ---------------------------------------------------------------------------------------------- 3. consistency with K4
def shell_points(n, seed=11):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    return d * (0.38 + 0.12 * torch.rand(n, 1, generator=g))


def k4_bound(theta, feat):
    """2.5 x the forward floor on these features: K4's heads and ra_heads_forward are each within 1.25 x floor of float64"""
    a64, r64, _ = oracle_heads(theta, feat, dtype=torch.float64, want_grad=False)
    ae, re_, _ = emulated_heads(theta, feat, want_grad=False)
    return 2 * BOUND * rms(cat4(ae, re_), cat4(a64, r64))


def test_consistent_with_k4_and_features_are_debug_mlps():
    cfg, net, eng, dev = engine()
    bpts = shell_points(3000).to(dev)
    _, _, feat, raw = eng.debug_full(bpts)
    theta = eng.heads_params()
    albedo, rough = eng.heads_forward(theta, feat)
    e, bound = rms(cat4(albedo, rough), raw[:, 9:13].cpu().double()), k4_bound(theta, feat)
    print(f'heads_forward vs K4 raw[:, 9:13]: rms {e:.3e}, bound {bound:.3e}')
    assert e <= bound, (e, bound)
    assert torch.equal(feat, feat.half().float())                    # the features are f16 values
    assert torch.equal(eng.bigpose_features(bpts), eng.debug_mlp(bpts)[2])
    assert torch.equal(eng.bigpose_features(bpts[:77]), eng.debug_mlp(bpts[:77])[2])


# ---------------------------------------------------------------------------------------------- 4. / 5. gradient parity, no underflow
def check_gradient(what, got, c, scale=1.0):
    got = got.detach().cpu().double() / scale
    assert torch.isfinite(got).all(), what
    floor, e = pooled_rms(c['grad_emu'], c['grad64']), pooled_rms(got, c['grad64'])
    ratios = tensor_ratios(got, c['grad_emu'], c['grad64'])
    print(f'{what}: pooled rms vs float64 {e[0]:.3e} / {e[1]:.3e} (albedo / roughness), floor {floor[0]:.3e} / {floor[1]:.3e}, '
          f'ratio {e[0] / floor[0]:.3f} / {e[1] / floor[1]:.3f}')
    print('    per tensor: ' + ', '.join(f'{k.replace("_network.linears", "")} {v:.2f}' for k, v in ratios.items()))
    for h in range(2):
        assert e[h] <= BOUND * floor[h], (what, HEADS[h], e[h], floor[h])


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', [1, 191, 1536, 20000])
def test_gradient_parity(kind, n):
    cfg, net, eng, dev = engine()
    c = case(kind, n)
    got = eng.heads_backward(c['theta'].to(dev), c['feat'].to(dev), c['d_albedo'].to(dev), c['d_rough'].to(dev))
    check_gradient(f'gradient {kind} n = {n}', got, c)


def test_gradient_parity_across_tape_chunks():
    """calls longer than the tape (32 768 points) run in chunks that carry on in the same slabs; the last chunk has fewer tiles than workgroups"""
    cfg, net, eng, dev = engine()
    n = 32768 + 100
    c = case('init', n)
    got = eng.heads_backward(c['theta'].to(dev), c['feat'].to(dev), c['d_albedo'].to(dev), c['d_rough'].to(dev))
    check_gradient(f'gradient init n = {n}', got, c)
    albedo, rough = eng.heads_forward(c['theta'].to(dev), c['feat'].to(dev))
    floor, e = rms(cat4(c['albedo_emu'], c['rough_emu']), cat4(c['albedo64'], c['rough64'])), rms(cat4(albedo, rough), cat4(c['albedo64'], c['rough64']))
    print(f'forward init n = {n}: kernel vs float64 rms {e:.3e}, floor {floor:.3e}')
    assert e <= BOUND * floor


@pytest.mark.parametrize('kind', KINDS)
def test_gradient_parity_with_the_reference_fixture(golden, kind):
    cfg, net, eng, dev = engine()
    z = golden('heads_grad.npz')
    c = case(kind, N_FIXTURE)
    got = eng.heads_backward(c['theta'].to(dev), c['feat'].to(dev), c['d_albedo'].to(dev), c['d_rough'].to(dev))
    check_gradient(f'gradient {kind} n = {N_FIXTURE}', got, c)
    ref = flat([torch.from_numpy(z[f'{kind}.grad.{k}']) for k in HEAD_KEYS])
    floor, e = pooled_rms(c['grad_emu'], c['grad64']), pooled_rms(got, ref)
    print(f'gradient {kind} vs the reference fixture: pooled rms {e[0]:.3e} / {e[1]:.3e}, floor {floor[0]:.3e} / {floor[1]:.3e}')
    assert e[0] <= BOUND * floor[0] and e[1] <= BOUND * floor[1]


@pytest.mark.parametrize('kind', KINDS)
def test_no_underflow_at_small_gradients(kind):
    """the gradients of an MSE over a frame are 1e-6: the same call with d_* times 2^-20 is the same gradient times 2^-20"""
    cfg, net, eng, dev = engine()
    c = case(kind, 1536)
    k = 2.0 ** -20
    got = eng.heads_backward(c['theta'].to(dev), c['feat'].to(dev), (c['d_albedo'] * k).to(dev), (c['d_rough'] * k).to(dev))
    check_gradient(f'gradient {kind} n = 1536 at 2^-20', got, c, scale=k)
    # a power of two moves nothing but the exponent: bit-identical to the unit-scale call
    unit = eng.heads_backward(c['theta'].to(dev), c['feat'].to(dev), c['d_albedo'].to(dev), c['d_rough'].to(dev))
    assert torch.equal(got / k, unit)


# ---------------------------------------------------------------------------------------------- 6. structure
def test_calls_are_reproducible_and_heads_are_independent():
    cfg, net, eng, dev = engine()
    c, other = case('init', 1536), case('sharp', 191)
    theta, feat, d_a, d_r = (c[k].to(dev) for k in ('theta', 'feat', 'd_albedo', 'd_rough'))
    first = eng.heads_backward(theta, feat, d_a, d_r)
    eng.heads_backward(other['theta'].to(dev), other['feat'].to(dev), other['d_albedo'].to(dev), other['d_rough'].to(dev))      # another size in between
    eng.heads_forward(theta, feat)
    again = eng.heads_backward(theta, feat, d_a, d_r)
    assert torch.equal(first, again)
    f1, f2 = eng.heads_forward(theta, feat), eng.heads_forward(theta, feat)
    assert torch.equal(f1[0], f2[0]) and torch.equal(f1[1], f2[1])
    only_r = torch.full((N_PARAMS,), 7.0, device=dev)
    raw_backward(eng, theta, feat, None, d_r, only_r)
    assert float(only_r[:A_SIZE].abs().max()) == 0.0 and torch.equal(only_r[A_SIZE:], first[A_SIZE:])
    only_a = torch.full((N_PARAMS,), 7.0, device=dev)
    raw_backward(eng, theta, feat, d_a, None, only_a)
    assert float(only_a[A_SIZE:].abs().max()) == 0.0 and torch.equal(only_a[:A_SIZE], first[:A_SIZE])
    # the forward's outputs are independent too
    a_only, r_only = torch.full((1536, 3), 7.0, device=dev), torch.full((1536,), 7.0, device=dev)
    raw_forward(eng, theta, feat, a_only, None)
    raw_forward(eng, theta, feat, None, r_only)
    assert torch.equal(a_only, f1[0]) and torch.equal(r_only, f1[1])


def test_empty_null_and_wrong_context():
    cfg, net, eng, dev = engine()
    c = case('init', 191)
    theta, feat, d_a, d_r = (c[k].to(dev) for k in ('theta', 'feat', 'd_albedo', 'd_rough'))
    out = [torch.full(s, 7.0, device=dev) for s in ((191, 3), (191,), (N_PARAMS,))]
    raw_forward(eng, theta, feat, out[0], out[1], n=0)
    raw_backward(eng, theta, feat, d_a, d_r, out[2], n=0)
    assert all(bool((t == 7.0).all()) for t in out)
    assert float(eng.heads_backward(theta, feat[:0], d_a[:0], d_r[:0]).abs().max()) == 0.0
    for bad in (lambda: raw_forward(eng, None, feat, out[0], out[1]), lambda: raw_forward(eng, theta, None, out[0], out[1], n=191),
                lambda: raw_backward(eng, None, feat, d_a, d_r, out[2]), lambda: raw_backward(eng, theta, feat, d_a, d_r, None)):
        with pytest.raises(_lib.RaError, match='null input'):
            bad()
    rc = eng.lib.ra_bigpose_features(eng.ctx, None, 5, p(out[0]), eng.stream)
    assert rc != 0 and b'null input' in eng.lib.ra_last_error()
    # a context without the material heads
    cfg2, net2, _ = build('anisdf')
    eng2 = net2.set_frame(synthetic.to_device(synthetic.make_body(0, posed=True), dev))
    for bad in (lambda: raw_forward(eng2, theta, feat, out[0], out[1]), lambda: raw_backward(eng2, theta, feat, d_a, d_r, out[2]),
                lambda: eng2.heads_params(), lambda: eng2.bigpose_features(feat[:, :3])):
        with pytest.raises(_lib.RaError, match='relight ctx'):
            bad()
    assert all(bool((t == 7.0).all()) for t in out)
    # another width or depth is refused before any launch
    eng.cfg.relight_network_width = 64
    try:
        with pytest.raises(_lib.RaError, match='relight_network_width 128'):
            eng.heads_forward(theta, feat)
    finally:
        eng.cfg.relight_network_width = 128


# ---------------------------------------------------------------------------------------------- 7. the autograd op
def test_autograd_op_is_the_raw_calls():
    cfg, net, eng, dev = engine()
    c = case('sharp', 191)
    theta, feat, d_a, d_r = (c[k].to(dev) for k in ('theta', 'feat', 'd_albedo', 'd_rough'))
    theta_p, feat_p = theta.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    albedo, rough = relight_utils.material_heads(eng, theta_p, feat_p)
    raw = eng.heads_forward(theta, feat)
    assert torch.equal(albedo, raw[0]) and torch.equal(rough, raw[1])
    ((albedo * d_a).sum() + (rough * d_r).sum()).backward()
    assert torch.equal(theta_p.grad, eng.heads_backward(theta, feat, d_a, d_r)) and feat_p.grad is None
    # one output unused: its head's slice is zero
    theta_p.grad = None
    (relight_utils.material_heads(eng, theta_p, feat)[1] * d_r).sum().backward()
    assert torch.equal(theta_p.grad, eng.heads_backward(theta, feat, torch.zeros_like(d_a), d_r))
    # n == 0: a zero gradient
    theta_p.grad = None
    a0, r0 = relight_utils.material_heads(eng, theta_p, feat[:0])
    assert a0.shape == (0, 3) and r0.shape == (0,)
    (a0.sum() + r0.sum()).backward()
    assert theta_p.grad.shape == theta.shape and float(theta_p.grad.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- 8. fit and round trip
def cpu_heads(theta, feat):
    """the heads in fp32 under torch autograd on the CPU, on the flat parameters (the oracle's arithmetic: OracleNet.material)"""
    cfg = heads_cfg()
    t = unflat(theta)

    def run(q, slope, bias):
        x = feat
        for i in range(3):
            x = torch.nn.functional.linear(x, q[2 * i], q[2 * i + 1])
            if i < 2:
                x = O.softplus100(x)
        return slope * torch.sigmoid(x) + bias
    return run(t[:6], cfg.albedo_slope, cfg.albedo_bias), run(t[6:], cfg.roughness_slope, cfg.roughness_bias)[:, 0]


def test_fit_heads_and_round_trip(golden):
    from relightableavatar_amd.renderer import make_renderer
    ref = golden('frame_novel.npz')
    cfg, net, dev = build('novel_light')
    H = int(ref['H'])
    batch = synthetic.to_device(synthetic.make_batch(H, H, seed=0, posed=True, crop=int(ref['crop']), n_novel_lights=3), dev)
    maps = make_renderer(cfg, net).render(batch)['probe00']
    eng = net.engine()
    probe = batch.novel_lights['probe00'].probe
    probe = (probe[0] if probe.ndim == 4 else probe).to(dev).float()
    target = maps.rgb_map.reshape(-1, 3).clone()
    hit = maps.acc_map.reshape(-1) > 0
    assert int(hit.sum()) >= 64
    theta0 = eng.heads_params()
    # (a) from the loaded weights, the composite of the heads on the cached features is the renderer's albedo / roughness map
    c = fitting._frame_cache(eng, cfg, batch, maps, target, None, True)
    assert c.feat.shape == (int(hit.sum()) * cfg.n_samples, 256)
    albedo, rough = fitting.composite_heads(cfg, c, *eng.heads_forward(theta0, c.feat))
    e = rms(cat4(albedo, rough), cat4(maps.albedo_map.reshape(-1, 3)[hit], maps.roughness_map.reshape(-1)[hit]))
    bound = k4_bound(theta0, c.feat)
    print(f'frame of {int(hit.sum())} hit pixels: composite of heads_forward vs the renderer\'s maps rms {e:.3e}, bound {bound:.3e}')
    assert e <= bound, (e, bound)
    at_optimum = fitting.fit_heads(net, [(batch, maps, target, None)], steps=0, lr=1e-3, fit_probe=False, probe_init=probe)
    # the loss there is what separates two f16-operand evaluations of the heads (K4's inside the renderer, ra_heads_forward here) behind
    # the tone map: an rgb rms below a tenth of an 8-bit step
    print(f'loss from the loaded weights and the true probe: {at_optimum.loss[0]:.3e} (rgb rms {at_optimum.loss[0] ** 0.5:.3e})')
    assert at_optimum.loss[0] <= (0.1 / 255) ** 2 and torch.equal(at_optimum.theta, theta0)
    # (b) perturbed heads are fitted back to the frame like the oracle's fp32 autograd loop fits them on the CPU
    steps, lr = 60, 1e-3
    start = unflat(theta0.cpu().clone())
    for i in (4, 5, 10, 11):
        start[i] *= 0.7
    start = flat(start)
    fit = fitting.fit_heads(net, [(batch, maps, target, None)], steps=steps, lr=lr, fit_probe=False, probe_init=probe, theta_init=start)
    cc = synthetic.dotdict({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in c.items()})
    xyz, area = synthetic.gen_light_xyz(cfg.env_h, cfg.env_w, cfg.env_r)
    o_net = types.SimpleNamespace(cfg=cfg, light_xyz=xyz, light_area=area)      # all shade_pixels reads of a net
    probe_c = torch.nn.functional.softplus(fitting._inv_softplus(probe.cpu().clamp_min(1e-6)))

    def o_loss_fn(theta):
        a, r = fitting.composite_heads(cfg, cc, *cpu_heads(theta, cc.feat))
        rgb = O.shade_pixels(o_net, probe_c, cc.ray_o, cc.surf, cc.norm, a, r[:, None], cc.lvis.T, cc.ldot.T, main_pass=False)[0]
        return torch.nn.functional.mse_loss(rgb, cc.target)
    param = start.clone().requires_grad_(True)
    opt = torch.optim.Adam([param], lr=lr)
    o_loss = []
    for _ in range(steps):
        opt.zero_grad()
        loss = o_loss_fn(param)
        loss.backward()
        opt.step()
        o_loss.append(float(loss.detach()))
    with torch.no_grad():
        o_loss.append(float(o_loss_fn(param)))
    print(f'fit_heads: loss {fit.loss[0]:.3e} -> {fit.loss[-1]:.3e}; oracle loop {o_loss[0]:.3e} -> {o_loss[-1]:.3e}')
    assert len(fit.loss) == steps + 1 and sorted(fit.state_dict) == sorted(HEAD_KEYS)
    assert fit.loss[-1] < 0.1 * fit.loss[0], (fit.loss[0], fit.loss[-1])
    assert fit.loss[-1] <= 1.1 * o_loss[-1], (fit.loss[-1], o_loss[-1])
    # (c) the fitted weights load back: K4's heads inside the renderer are ra_heads_forward on the fitted theta
    net.load_state_dict(fit.state_dict, strict=False)
    eng = net.set_frame(batch)
    assert torch.equal(eng.heads_params(), fit.theta)
    bpts = shell_points(2000).to(dev)
    _, _, feat, raw = eng.debug_full(bpts)
    albedo, rough = eng.heads_forward(fit.theta, feat)
    e, bound = rms(cat4(albedo, rough), raw[:, 9:13].cpu().double()), k4_bound(fit.theta, feat)
    print(f'fitted heads loaded back: heads_forward vs K4 raw[:, 9:13] rms {e:.3e}, bound {bound:.3e}')
    assert e <= bound, (e, bound)

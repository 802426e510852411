"""ra_canonical_features (csrc/ra_k4_canon.hpp) and ra_gaussian_entropy (csrc/ra_entropy.hip) through the C ABI, the autograd op on top
(relight_utils.gaussian_entropy) and the regularised fitting entry point (fitting.fit_heads(regularisers=...)).  Run with `-m gpu` on an
MI355X.

Parity rules — none of them new:
    canonical features   bit identity with ra_bigpose_features on the full query's own canonical points; on arbitrary points the
                         rounding-parity rule and bounds of test_gpu_parity.py (PARITY['feat']).
    entropy              test_oracle_relight_reg.entropy_bound: per output, max and rms error over max |ref| against float64 at most
                         10 x the fp32 oracle's own on the same inputs, or 10 x 8 fp32 unit roundoffs where that is larger.
    jitter outputs       1.25 x the floor of the emulated chain (kernel-like sdf_feat, features rounded to f16, emulated_heads): the
                         project's bound for these heads (test_gpu_heads.BOUND).

Every test prints its figures before it asserts (pytest -s); DESIGN.md section 12 holds the record.
"""
import ctypes as C

import pytest
import torch

from relightableavatar_amd import _lib, fitting, relight_utils, synthetic
from test_gpu_heads import BOUND, build, cat4, engine, k4_bound, shell_points
from test_gpu_parity import _parity_net, _q, rounding_parity
from test_oracle_heads_grad import HEAD_KEYS, emulated_heads, flat, oracle_heads, rms, unflat
from test_oracle_relight_reg import (ENTROPY_SETS, CpuEngine, cpu_heads, entropy_autograd, entropy_bound, entropy_closed_form, entropy_inputs,
                                     gaussian_entropy)

pytestmark = pytest.mark.gpu
from oracle import ra_oracle as O      # noqa: E402


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def raw_entropy(eng, x, n, d_value, value, d_x):
    return eng.lib.ra_gaussian_entropy(eng.ctx, p(x), n, p(d_value), p(value), p(d_x), eng.stream)


# ---------------------------------------------------------------------------------------------- 1. symbols
def test_native_symbols_are_loaded():
    cfg, net, eng, dev = engine()
    assert 'librelightableavatar_hip.so' in open('/proc/self/maps').read()
    assert eng.lib.ra_abi_version() == 9
    for name in ('ra_canonical_features', 'ra_gaussian_entropy'):
        assert hasattr(eng.lib, name), name


# ---------------------------------------------------------------------------------------------- 2. canonical features: bit identity
@pytest.mark.parametrize('dtype', ['f16', 'bf16'])
def test_canonical_features_are_the_full_querys_bit_for_bit(dtype):
    cfg, eng, body, dev = _parity_net('relight', dtype, 'init')
    bpts = shell_points(4000).to(dev)
    _, _, feat, raw = eng.debug_full(bpts)
    cp = raw[:, 0:3].contiguous()                     # the kernel's own fp32 bpts + resd
    big = eng.bigpose_features(bpts)
    got = eng.canonical_features(cp)
    print(f'{dtype}: canonical_features(raw[:, 0:3]) vs bigpose_features(bpts): max |diff| {float((got - big).abs().max()):.3e}, '
          f'max |feat| {float(big.abs().max()):.3e}, moved by the residual net: {float((cp - bpts).abs().max()):.3e} m')
    assert torch.equal(feat, big) and float((cp - bpts).abs().max()) > 0
    assert torch.equal(got, big)
    assert torch.equal(got, _q(got, dtype))           # values of the operand type
    for n in (1, 31, 32, 33, 127, 129):               # tile edges: prefixes of the same points
        assert torch.equal(eng.canonical_features(cp[:n].contiguous()), big[:n]), n
    # into the second half of a larger buffer, the first half untouched
    both = torch.full((2 * 129, 256), 7.0, device=dev)
    eng.canonical_features(cp[:129].contiguous(), out=both[129:])
    assert bool((both[:129] == 7.0).all()) and torch.equal(both[129:], big[:129])


# ---------------------------------------------------------------------------------------------- 3. canonical features: rounding parity
@pytest.mark.parametrize('kind', ['init', 'sharp'])
@pytest.mark.parametrize('dtype', ['f16', 'bf16'])
def test_canonical_features_match_the_operand_rounding_emulation(dtype, kind):
    cfg, eng, body, dev = _parity_net('relight', dtype, kind)
    sd = synthetic.make_state_dict(0, relight=True, cfg=cfg, kind=kind)
    g = torch.Generator().manual_seed(5)
    cpts = shell_points(4000) + 0.02 * torch.randn(4000, 3, generator=g)
    with torch.no_grad():
        emu = O.OracleNet(sd, cfg, emulate=dtype, kernel_like=True).sdf_feat(cpts)[1]
        f64 = O.OracleNet(sd, cfg, emulate='f64acc').sdf_feat(cpts)[1]
    hip = eng.canonical_features(cpts.to(dev)).cpu()
    fails = rounding_parity(f'canonical feat {dtype} {kind}', 'feat', hip, _q(emu, dtype), f64)[1]
    assert not fails, fails


# ---------------------------------------------------------------------------------------------- 4. entropy parity
ENTROPY_CASES = [(name, None) for name in ENTROPY_SETS] + [('skin', n) for n in (63, 64, 65, 20000)]


@pytest.mark.parametrize('name,n', ENTROPY_CASES)
def test_entropy_parity(golden, name, n):
    cfg, net, eng, dev = engine()
    x = entropy_inputs(name) if n is None else entropy_inputs(name, n)
    v64, g64 = entropy_autograd(x, torch.float64)
    v32, g32 = entropy_autograd(x, torch.float32)
    value, d_x = eng.gaussian_entropy(x.to(dev))
    lab = f'entropy {name} n = {x.shape[0]}'
    assert bool(torch.isfinite(value)) and bool(torch.isfinite(d_x).all())
    fails = entropy_bound(f'{lab} value', value, v32, v64) + entropy_bound(f'{lab} dE/dx', d_x, g32, g64)
    if n is None:      # the reference's own fp32 outputs
        z = golden('relight_reg.npz')
        ref_v, ref_g = torch.from_numpy(z[f'entropy.{name}.value']).double(), torch.from_numpy(z[f'entropy.{name}.grad']).double()
        fails += entropy_bound(f'{lab} value vs the reference fixture', value, v32, v64, against=ref_v)
        fails += entropy_bound(f'{lab} dE/dx vs the reference fixture', d_x, g32, g64, against=ref_g)
    assert not fails, fails


# ---------------------------------------------------------------------------------------------- 5. entropy properties
def test_entropy_calls_are_reproducible_and_linear_in_the_upstream_scalar():
    cfg, net, eng, dev = engine()
    x = entropy_inputs('skin', 20000).to(dev)
    v1, g1 = eng.gaussian_entropy(x)
    eng.gaussian_entropy(entropy_inputs('wide').to(dev))      # another size in between
    v2, g2 = eng.gaussian_entropy(x)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    k = 2.0 ** -10
    v3, g3 = eng.gaussian_entropy(x, d_value=torch.tensor([k], device=dev))
    assert torch.equal(v3, v1) and torch.equal(g3, g1 * k)
    v4, none = eng.gaussian_entropy(x, want_grad=False)
    assert none is None and torch.equal(v4, v1)


def test_entropy_degenerate_channels_and_errors():
    cfg, net, eng, dev = engine()
    full = entropy_inputs('skin')
    const = full.clone()
    const[:, 2] = 0.4
    v, g = eng.gaussian_entropy(const.to(dev))
    v_full, g_full = eng.gaussian_entropy(full.to(dev))
    v_o, g_o = entropy_closed_form(const)
    print(f'constant third channel: value {float(v):.6f} (oracle {float(v_o):.6f}, all three channels live {float(v_full):.6f}), '
          f'max |g| of the constant channel {float(g[:, 2].abs().max())}')
    assert bool(torch.isfinite(v)) and float(g[:, 2].abs().max()) == 0.0
    assert torch.equal(g[:, :2], g_full[:, :2])
    assert abs(float(v) - float(v_o)) <= 1e-6 * abs(float(v_o))
    # the gradient of a degenerate channel is zero whatever the upstream factor
    _, g_inf = eng.gaussian_entropy(const.to(dev), d_value=torch.tensor([float('inf')], device=dev))
    assert float(g_inf[:, 2].abs().max()) == 0.0
    # all mass in one bin
    gen = torch.Generator().manual_seed(77)
    one = (0.5 + 0.005 * torch.randn(600, 3, generator=gen)).to(dev)
    v1, g1 = eng.gaussian_entropy(one)
    print(f'0.5 + 0.005 randn: value {float(v1):.6e}, max |g| {float(g1.abs().max()):.3e}')
    assert bool(torch.isfinite(v1)) and bool(torch.isfinite(g1).all())
    # errors
    x = full.to(dev)
    value, d_x = torch.full((), 7.0, device=dev), torch.full((600, 3), 7.0, device=dev)
    assert raw_entropy(eng, x, 1, None, value, d_x) != 0 and b'bad sizes' in eng.lib.ra_last_error()
    assert raw_entropy(eng, None, 600, None, value, d_x) != 0 and b'null input' in eng.lib.ra_last_error()
    assert raw_entropy(eng, x, 600, None, None, d_x) != 0 and b'null input' in eng.lib.ra_last_error()
    rc = eng.lib.ra_canonical_features(eng.ctx, None, 5, p(d_x), eng.stream)
    assert rc != 0 and b'null input' in eng.lib.ra_last_error()
    assert eng.lib.ra_canonical_features(eng.ctx, None, 0, None, eng.stream) == 0
    torch.cuda.synchronize()
    assert float(value) == 7.0 and bool((d_x == 7.0).all())
    # a context without the material heads: fine for the entropy (no weights are read), refused by the feature query
    cfg2, net2, _ = build('anisdf')
    eng2 = net2.set_frame(synthetic.to_device(synthetic.make_body(0, posed=True), dev))
    v2, g2 = eng2.gaussian_entropy(x)
    assert torch.equal(v2, v_full) and torch.equal(g2, g_full)
    with pytest.raises(_lib.RaError, match='relight ctx'):
        eng2.canonical_features(x)


# ---------------------------------------------------------------------------------------------- 6. the autograd op
def test_autograd_op_is_the_raw_call_times_the_upstream_scalar():
    cfg, net, eng, dev = engine()
    x = entropy_inputs('two').to(dev)
    value, d_x = eng.gaussian_entropy(x)
    xp = x.clone().requires_grad_(True)
    e = relight_utils.gaussian_entropy(eng, xp)
    assert e.shape == () and torch.equal(e, value)
    (e * 3.5).backward()
    assert torch.equal(xp.grad, d_x * 3.5)
    xp.grad = None
    relight_utils.gaussian_entropy(eng, xp.reshape(200, 3, 3)).backward()      # (..., 3): the reference's view(-1, 3)
    assert xp.grad.shape == x.shape and torch.equal(xp.grad, d_x)


# ---------------------------------------------------------------------------------------------- 7. / 8. a traced frame
_frame = []


def traced_frame(golden):
    """the 64 x 64 relit frame of test_gpu_heads.test_fit_heads_and_round_trip, built the same way, once"""
    if not _frame:
        from relightableavatar_amd.renderer import make_renderer
        ref = golden('frame_novel.npz')
        cfg, net, dev = build('novel_light')
        H = int(ref['H'])
        batch = synthetic.to_device(synthetic.make_batch(H, H, seed=0, posed=True, crop=int(ref['crop']), n_novel_lights=3), dev)
        maps = make_renderer(cfg, net).render(batch)['probe00']
        probe = batch.novel_lights['probe00'].probe
        probe = (probe[0] if probe.ndim == 4 else probe).to(dev).float()
        target = maps.rgb_map.reshape(-1, 3).clone()
        _frame.append((cfg, net, dev, batch, maps, probe, target))
    return _frame[0]


def test_regulariser_terms_on_a_traced_frame(golden):
    cfg, net, dev, batch, maps, probe, target = traced_frame(golden)
    eng = net.engine()
    theta0 = eng.heads_params()
    c = fitting._frame_cache(eng, cfg, batch, maps, target, None, True)
    n = c.cpts.shape[0]
    assert c.feat2.shape == (2 * n, 256) and c.feat.data_ptr() == c.feat2.data_ptr() and c.feat.shape == (n, 256)
    assert torch.equal(eng.canonical_features(c.cpts), c.feat)        # raw[:, 0:3] are the kernel's own canonical points
    noise = cfg.xyz_noise_std * torch.randn(n, 3, generator=torch.Generator().manual_seed(3))
    terms = fitting.regulariser_terms(eng, c, theta0, noise.to(dev))
    print(f'{n} samples of {n // c.S} hit pixels: ' + ', '.join(f'{k} {float(v):.6e}' for k, v in terms.items()))
    assert sorted(terms) == sorted(fitting.TERMS) and all(bool(torch.isfinite(v)) for v in terms.values())
    # the two entropies against float64 on the DOWNLOADED device values: the same inputs, the rule of test_entropy_parity
    albedo_s, rough_s = eng.heads_forward(theta0, c.feat)
    volume = fitting.composite_heads(cfg, c, albedo_s, rough_s, want_volume=True)[2]
    fails = []
    for name, x in (('albedo_entropy', albedo_s), ('volume_entropy', volume)):
        v64, v32 = entropy_autograd(x.cpu(), torch.float64)[0], entropy_autograd(x.cpu(), torch.float32)[0]
        print(f'{name}: variance per channel {[float(v) for v in x.var(0)]}, float64 {float(v64):.6e}')
        fails += entropy_bound(name, terms[name], v32, v64)
    assert not fails, fails
    # the jitter outputs per sample against the float64 chain; floor: the emulated chain
    albedo_j, rough_j = eng.heads_forward(theta0, eng.canonical_features(c.cpts + noise.to(dev)))
    assert abs(float(terms.albedo_smooth) - float((albedo_s - albedo_j).abs().sum(-1).mean())) <= 1e-6 * float(terms.albedo_smooth)
    assert abs(float(terms.roughness_smooth) - float((rough_s - rough_j).abs().mean())) <= 1e-6 * float(terms.roughness_smooth)
    sd = synthetic.make_state_dict(0, relight=True, cfg=cfg)
    jit = c.cpts.cpu() + noise
    with torch.no_grad():
        feat64 = O.OracleNet(sd, cfg, emulate='f64acc').sdf_feat(jit)[1]
        feat_e = O.OracleNet(sd, cfg, emulate='f16', kernel_like=True).sdf_feat(jit)[1].half().float()
    a64, r64, _ = oracle_heads(theta0, feat64, dtype=torch.float64, want_grad=False)
    ae, re_, _ = emulated_heads(theta0, feat_e, want_grad=False)
    floor, e = rms(cat4(ae, re_), cat4(a64, r64)), rms(cat4(albedo_j, rough_j), cat4(a64, r64))
    print(f'jitter outputs: kernel chain vs float64 rms {e:.3e}, floor (emulated chain) {floor:.3e}, ratio {e / floor:.3f}')
    assert e <= BOUND * floor, (e, floor)
    # zero weights: the history of the image loss alone, bit for bit
    start = unflat(theta0.cpu().clone())
    for i in (4, 5, 10, 11):
        start[i] *= 0.7
    start = flat(start)
    kw = dict(steps=3, lr=1e-3, fit_probe=False, probe_init=probe, theta_init=start)
    plain = fitting.fit_heads(net, [(batch, maps, target, None)], **kw)
    zero = fitting.fit_heads(net, [(batch, maps, target, None)], regularisers={'img_loss_weight': 1.0, 'albedo_sparsity': 0.0, 'albedo_smooth_weight': 0.0,
                                                                              'roughness_smooth_weight': 0.0}, generator=torch.Generator().manual_seed(1), **kw)
    print(f'zero weights: loss {zero.loss} against {plain.loss}')
    assert zero.loss == plain.loss and torch.equal(zero.theta, plain.theta) and 'terms' not in plain
    assert zero.terms.img_loss == plain.loss and all(len(zero.terms[k]) == 4 for k in fitting.TERMS)


def test_regularised_fit_follows_the_oracle_loop(golden):
    cfg, net, dev, batch, maps, probe, target = traced_frame(golden)
    eng = net.engine()
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items() if k in HEAD_KEYS}
    theta0 = eng.heads_params()
    c = fitting._frame_cache(eng, cfg, batch, maps, target, None, True)
    n = c.cpts.shape[0]
    steps, lr = 60, 1e-3
    start = unflat(theta0.cpu().clone())
    for i in (4, 5, 10, 11):
        start[i] *= 0.7
    start = flat(start)
    g = torch.Generator().manual_seed(12)
    noises = [cfg.xyz_noise_std * torch.randn(n, 3, generator=g) for _ in range(steps + 1)]      # drawn once, fed to both sides
    fit = fitting.fit_heads(net, [(batch, maps, target, None)], steps=steps, lr=lr, fit_probe=False, probe_init=probe, theta_init=start, regularisers=True,
                            noise_fn=lambda step, frame, m: noises[step].to(dev))
    # the oracle's fp32 autograd loop on the CPU from the same start
    o_eng = CpuEngine(cfg=cfg, sd=synthetic.make_state_dict(0, relight=True, cfg=cfg))
    cc = synthetic.dotdict({k: (v.cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in c.items()})
    probe_c = torch.nn.functional.softplus(fitting._inv_softplus(probe.cpu().clamp_min(1e-6)))
    weights = fitting.regulariser_weights(cfg, True)
    ops = dict(heads=cpu_heads, entropy=lambda e, x: gaussian_entropy(x), shade=o_eng.shade)
    param = start.clone().requires_grad_(True)
    opt = torch.optim.Adam([param], lr=lr)
    o_loss = []
    for step in range(steps):
        opt.zero_grad()
        loss, _ = fitting.regularised_loss(o_eng, [cc], param, probe_c, weights, [noises[step]], **ops)
        loss.backward()
        opt.step()
        o_loss.append(float(loss.detach()))
    with torch.no_grad():
        o_loss.append(float(fitting.regularised_loss(o_eng, [cc], param, probe_c, weights, [noises[steps]], **ops)[0]))
    print(f'regularised fit_heads: total {fit.loss[0]:.4e} -> {fit.loss[-1]:.4e}; oracle loop {o_loss[0]:.4e} -> {o_loss[-1]:.4e}')
    for k in ('img_loss',) + fitting.TERMS:
        print(f'    {k}: {fit.terms[k][0]:.4e} -> {fit.terms[k][-1]:.4e} (weight {weights[dict(img_loss="img_loss_weight", albedo_entropy="albedo_sparsity", volume_entropy="albedo_sparsity", albedo_smooth="albedo_smooth_weight", roughness_smooth="roughness_smooth_weight")[k]]:g})')
        assert len(fit.terms[k]) == steps + 1 and all(v == v and abs(v) != float('inf') for v in fit.terms[k]), k
    assert len(fit.loss) == steps + 1 and all(v == v and abs(v) != float('inf') for v in fit.loss)
    try:
        assert fit.loss[-1] < fit.loss[0], (fit.loss[0], fit.loss[-1])
        assert fit.loss[-1] <= 1.1 * o_loss[-1], (fit.loss[-1], o_loss[-1])
        # the fitted weights load back and render
        net.load_state_dict(fit.state_dict, strict=False)
        eng = net.set_frame(batch)
        assert torch.equal(eng.heads_params(), fit.theta)
        from relightableavatar_amd.renderer import make_renderer
        again = make_renderer(cfg, net).render(batch)['probe00']
        assert bool(torch.isfinite(again.rgb_map).all()) and again.rgb_map.shape == maps.rgb_map.shape
        bpts = shell_points(2000).to(dev)
        _, _, feat, raw = eng.debug_full(bpts)
        albedo, rough = eng.heads_forward(fit.theta, feat)
        e, bound = rms(cat4(albedo, rough), raw[:, 9:13].cpu().double()), k4_bound(fit.theta, feat)
        print(f'fitted heads loaded back: heads_forward vs K4 raw[:, 9:13] rms {e:.3e}, bound {bound:.3e}')
        assert e <= bound, (e, bound)
    finally:
        net.load_state_dict(sd0, strict=False)      # the frame is shared with the test above
        net.set_frame(batch)

"""The oracle's operand-rounding emulation (16-bit MFMA operands, fp32 accumulate) and the committed precision floors.  CPU only."""
import json
import os

import numpy as np
import torch

from oracle import ra_oracle as O
from relightableavatar_amd import synthetic
from relightableavatar_amd.config import make_cfg

HERE = os.path.dirname(os.path.abspath(__file__))
T = torch.from_numpy


def _nets(**kw):
    cfg = make_cfg('relight')
    sd = synthetic.make_state_dict(0, relight=True, cfg=cfg)
    return cfg, sd


def test_emulation_off_is_the_fp32_oracle_and_on_rounds_operands(golden):
    cfg, sd = _nets()
    ops = golden('ops.npz')
    fr = O._frame(synthetic.make_body(0, posed=True))
    x = T(ops['mlp_bpts'])
    plain = O.observed_sdf(O.OracleNet(sd, cfg), x, fr)
    assert torch.equal(plain, O.observed_sdf(O.OracleNet(sd, cfg, emulate='f32'), x, fr))
    assert float((plain - T(ops['mlp_sdf'])).abs().max()) < 2e-6
    e16 = float((O.observed_sdf(O.OracleNet(sd, cfg, emulate='f16'), x, fr) - plain).abs().mean())
    eb16 = float((O.observed_sdf(O.OracleNet(sd, cfg, emulate='bf16'), x, fr) - plain).abs().mean())
    assert 1e-5 < e16 < 2e-4 and 4 * e16 < eb16 < 2e-3            # 3 mantissa bits apart
    # the kernel-like variant (fp32 pose bias, hi + lo coordinates) is no worse than plain rounding
    ek = float((O.observed_sdf(O.OracleNet(sd, cfg, emulate='f16', kernel_like=True), x, fr) - plain).abs().mean())
    assert ek < 1.1 * e16


def test_committed_floor_is_reproducible(golden):
    """re-derives one entry of tests/golden/precision_floor.json (tools/precision_floor.py) — the frame the SURVEY.md:409
    contract is asserted on — and checks what the file says about the SURVEY 8d body"""
    floors = json.load(open(os.path.join(HERE, 'golden', 'precision_floor.json')))
    ref = golden('frame_relight_smooth.npz')
    cfg = make_cfg('relight', vis_specular_map=True)
    net = O.OracleNet(synthetic.make_state_dict(0, relight=True, cfg=cfg), cfg, emulate='f16', kernel_like=True)
    batch = synthetic.make_batch(int(ref['H']), int(ref['H']), seed=0, posed=True, crop=int(ref['crop']), skin_noise=float(ref['skin_noise']))
    out = O.render_sphere_tracing(net, batch)
    p = O.psnr(out.rgb_map, T(ref['rgb_map']))
    f = floors['frame_relight_smooth.npz:f16']['rgb_map']
    assert abs(p - f['psnr']) < 1.0, (p, f)                       # thread-count dependent summation order moves it a little
    assert f['psnr'] >= 60 and f['max_abs'] <= 1e-2               # f16 operands meet the contract where the trace converges
    g = floors['frame_relight.npz:f16']['rgb_map']
    assert g['max_abs'] > 1e-2 and g['psnr_trim2pct'] > g['psnr'] + 10     # ... and cannot on the SURVEY 8d body: 2 % of the pixels decide
    assert floors['frame_relight.npz:bf16']['rgb_map']['psnr'] < g['psnr'] - 4


def test_reference_trace_limit_cycle_on_the_survey_body():
    """why: on the SURVEY 8d body the fp32 ORACLE's own surface trace does not converge on ~9 % of the hit rays (|d| of each of the
    last three iterations stays above a millimetre: a limit cycle across a jump of the warp), several times more often than
    with a smooth skinning field"""
    cfg, sd = _nets()
    net = O.OracleNet(sd, cfg)
    res = {}
    for sn in (2.0, 0.0):
        b = synthetic.make_batch(128, 128, seed=0, posed=True, crop=16, skin_noise=sn)
        fr = O._frame(b)
        log = []

        def f(x):
            s = O.hdq_sdf(net, x, fr, cfg.dist_th, True)
            log.append(s[:, 0].abs().clone())
            return s
        O.sphere_tracing(b.ray_o[0], b.ray_d[0], b.near[0][:, None], b.far[0][:, None], f, iter=16, offset=0.02)
        res[sn] = float((torch.stack(log[-3:]).amin(0) > 1e-3).float().mean())       # rays still > 1 mm off the surface
    assert res[2.0] > 0.05 and res[0.0] < 0.5 * res[2.0], res


def test_compensated_and_float64_variants_of_the_oracle():
    """round 4's deciding experiment (tools/precision_tiers.py): `f64acc` (every nn.Linear in float64, rounded once) is a differently
    associated fp32 and must agree with the fp32 oracle at rounding level; `f16x2` (f16 hi + lo operand pairs, three products: the
    arithmetic of the HIP kernel K3C) must be as accurate as fp32 itself, two orders of magnitude better than plain f16 operands"""
    cfg, sd = _nets()
    fr = O._frame(synthetic.make_body(0, posed=True))
    g = torch.Generator().manual_seed(11)
    d = torch.nn.functional.normalize(torch.randn(4000, 3, generator=g), dim=-1)
    x = d * (0.38 + 0.12 * torch.rand(4000, 1, generator=g))
    rms = lambda a, b: float((a - b).pow(2).mean().sqrt())
    f64 = O.observed_sdf(O.OracleNet(sd, cfg, emulate='f64acc'), x, fr)
    f32 = O.observed_sdf(O.OracleNet(sd, cfg), x, fr)
    x2 = O.observed_sdf(O.OracleNet(sd, cfg, emulate='f16x2', kernel_like=True), x, fr)
    f16 = O.observed_sdf(O.OracleNet(sd, cfg, emulate='f16', kernel_like=True), x, fr)
    assert rms(f32, f64) < 3e-7 and rms(x2, f64) < 3e-7 and rms(f16, f64) > 2e-5
    tiers = json.load(open(os.path.join(HERE, 'golden', 'precision_tiers.json')))
    for case in ('frame_relight', 'bench_sample', 'full_size_sample'):
        assert tiers[f'{case}:f64acc']['rgb_map']['psnr'] > 85 and tiers[f'{case}:f64acc']['rgb_map']['rays_over_1e2'] == 0       # fp32 pins these frames
        t, k4, plain = (tiers[f'{case}:{v}']['rgb_map'] for v in ('tier', 'tier_k4', 'f16'))
        assert t['psnr'] >= 60 and t['max_abs'] <= 1e-2 and abs(t['psnr'] - k4['psnr']) < 0.5      # only the surface trace needs the tier
        assert plain['max_abs'] > 1e-2                                                              # plain f16 operands do not meet the contract


def test_fp32_unstable_rays_fixture_is_reproducible():
    """tests/golden/fp32_unstable_rays.json (tools/fp32_stability.py): re-derive the smallest ray set and check the shape of all"""
    fx = json.load(open(os.path.join(HERE, 'golden', 'fp32_unstable_rays.json')))
    cfg, sd = _nets()
    net = O.OracleNet(sd, cfg)
    bad = O.fp32_unstable_rays(net, synthetic.make_batch(128, 128, seed=0, posed=True, crop=8))
    assert [int(i) for i in bad.nonzero()[:, 0]] == fx['smoke']['unstable'] == fx['multi_chunk']['unstable']
    for k, v in fx.items():
        if k.startswith('_'):
            continue
        # a handful of rays, not a tolerance in disguise: <= 2 % — and 5 % on the one hard case that stacks everything the reference's trace
        # dislikes (trained-like weights on the noisy skinning field of a body pulled apart: 6 of 144 rays)
        assert len(v['unstable']) <= max(2, (0.05 if k == 'switches.npz:sharp_split' else 0.02) * v['n_rays']), k
    # the mechanism: noise far below any rendering tolerance moves such a ray's surface point by millimetres
    st0, _ = O.surface_trace(net, synthetic.make_batch(128, 128, seed=0, posed=True, crop=8))
    moved = 0
    for s in range(8):
        st, _ = O.surface_trace(net, synthetic.make_batch(128, 128, seed=0, posed=True, crop=8), 1e-7, torch.Generator().manual_seed(s))
        moved += int((st - st0).abs()[bad].max() > 1e-3)
    assert moved >= 1


def _shell(n, seed=11):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    return d * (0.38 + 0.12 * torch.rand(n, 1, generator=g))


def test_backward_emulation_is_opt_in_and_changes_only_the_gradient():
    """emulate_backward off: no custom autograd function is involved (the existing paths, bit for bit); on: the forward values are the
    same bits, only d sdf / d bpts changes — by less than the rounding floor itself"""
    cfg, sd = _nets()
    fr = O._frame(synthetic.make_body(0, posed=True))
    x = _shell(2000)
    rms = lambda a: float(a.pow(2).mean().sqrt())
    g64 = O.bigpose_query(O.OracleNet(sd, cfg, emulate='f64acc'), x, fr.cond)[5]
    for dt in ('f16', 'bf16'):
        off = O.OracleNet(sd, cfg, emulate=dt, kernel_like=True)
        on = O.OracleNet(sd, cfg, emulate=dt, kernel_like=True, emulate_backward=True)
        a, b = O.bigpose_query(off, x, fr.cond), O.bigpose_query(on, x, fr.cond)
        assert off.relu_margin is None and off.delta_stats == {} and on.relu_margin.shape == (2000,) and on.delta_stats['n_nonzero'] > 0
        for k in range(5):                                  # bpts, resd, cpts, sdf, feat
            assert torch.equal(a[k], b[k]), (dt, k)
        assert 0 < rms(b[5] - a[5]) < rms(a[5] - g64), dt
    # the fp32 reference path takes plain autograd: d sdf / d bpts of observed_sdf
    net = O.OracleNet(sd, cfg)
    xr = x.clone().requires_grad_(True)
    ref = torch.autograd.grad(O.observed_sdf(net, xr, fr).sum(), xr)[0]
    assert torch.equal(O.bigpose_query(net, x, fr.cond)[5], ref)
    for bad in (dict(emulate='f16'), dict(emulate=None, kernel_like=True), dict(emulate='f16x2', kernel_like=True), dict(emulate='f64acc')):
        try:
            O.OracleNet(sd, cfg, emulate_backward=True, **bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_backward_emulation_building_blocks():
    """the three autograd pieces against their definitions: the transposed product rounds delta * GRAD_SCALE and nothing else; sigma'
    comes from the ROUNDED scaled activation (1 - 2^-q(y')); the ReLU mask from the sign bit"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(64, 40, generator=g).requires_grad_(True)
    w = torch.randn(24, 40, generator=g)
    up = torch.randn(64, 24, generator=g) * 1e-3
    stats = {}
    y = O._KernelTransposedProduct.apply(x, (x @ w.T).detach(), w, torch.float16, stats)
    gx = torch.autograd.grad(y, x, up)[0]
    q = (up * O.GRAD_SCALE).half().float() / O.GRAD_SCALE
    assert torch.equal(gx, q @ w) and not torch.equal(q, up) and stats['max_abs'] == float((up * O.GRAD_SCALE).abs().max())
    y = O._KernelTransposedProduct.apply(x, (x @ w.T).detach(), w, None, None)          # the SDF head's seed: fp32
    assert torch.equal(torch.autograd.grad(y, x, up)[0], up @ w)
    z = (torch.randn(5000, generator=g) * 0.03).requires_grad_(True)
    for dt in (torch.float16, torch.bfloat16):
        gz = torch.autograd.grad(O._TapedSoftplus.apply(z, dt).sum(), z)[0]
        yq = (O.softplus100(z.detach()) * O.OracleNet.SP_SCALE).to(dt).float()
        assert torch.equal(gz, 1 - torch.exp2(-yq))
        exact = torch.sigmoid(100 * z.detach())
        ulp = torch.finfo(dt).eps
        assert 0 < float((gz - exact).abs().max()) < 2 * ulp * float(yq.abs().max()), dt        # the rounding of y' is all that differs
    z = torch.tensor([-1.0, -0.0, 0.0, 1e-30, -1e-30, 2.0], requires_grad=True)
    assert torch.autograd.grad(O._SignMaskRelu.apply(z).sum(), z)[0].tolist() == [0, 0, 1, 1, 0, 1]


# d sdf / d bpts with the reverse pass emulated, rms against the float64-accumulated oracle on 4 000 near-surface points (measured:
# f16 6.6e-4 / 2.3e-3, bf16 2.9e-3 / 7.7e-3 at init / sharp weights)
GRAD_BANDS = {('f16', 'init'): (5e-4, 8.5e-4), ('bf16', 'init'): (2.3e-3, 3.7e-3),
              ('f16', 'sharp'): (1.8e-3, 2.9e-3), ('bf16', 'sharp'): (6e-3, 9.5e-3)}


def test_backward_emulation_error_bands():
    """the floor the reverse-mode kernel K4 is held to (tests/test_gpu_parity.py rounding_parity): the emulated gradient's error against
    f64acc in a measured band per operand type and weights, bf16 several times f16; at trained-like weights no scaled delta overflows f16
    (K4 carries gradients times GRAD_SCALE = 16 for headroom against underflow)"""
    fr = O._frame(synthetic.make_body(0, posed=True))
    cfg = make_cfg('relight')
    x = _shell(4000)
    rms = lambda a: float(a.pow(2).mean().sqrt())
    got = {}
    for kind in ('init', 'sharp'):
        sd = synthetic.make_state_dict(0, relight=True, cfg=cfg, kind=kind)
        g64 = O.bigpose_query(O.OracleNet(sd, cfg, emulate='f64acc'), x, fr.cond)[5]
        for dt in ('f16', 'bf16'):
            net = O.OracleNet(sd, cfg, emulate=dt, kernel_like=True, emulate_backward=True)
            e = rms(O.bigpose_query(net, x, fr.cond)[5] - g64)
            st = net.delta_stats
            print(f'{dt} {kind}: grad rms vs f64acc {e:.2e}; largest |delta * 16| {st["max_abs"]:.3g}, '
                  f'{100 * st["n_subnormal"] / st["n_nonzero"]:.2f} % of the nonzero scaled deltas below the smallest normal {dt}')
            lo, hi = GRAD_BANDS[(dt, kind)]
            assert lo < e < hi, (dt, kind, e)
            assert st['max_abs'] < 65504 / 16, (dt, kind, st)          # four more octaves of headroom than the scale needs
            got[(dt, kind)] = e
    for kind in ('init', 'sharp'):
        assert got[('bf16', kind)] > 3 * got[('f16', kind)], got

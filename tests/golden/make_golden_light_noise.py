#!/usr/bin/env python3
"""Golden values under MOVED LIGHTS, made by running the REFERENCE itself on the CPU in fp32 (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_light_noise.py            # writes light_noise.npz
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_light_noise.py --check    # recomputes and compares with the committed file

The reference's relight network returns light_xyz_ + randn * cfg.light_xyz_noise_std in training mode (relight_network.py:79-84), once
per render call (sphere_tracing_renderer.py:1029).  Here the noise is explicit and stored, not only its seed.

(a) visibility: the reference's light_visibility (sphere_tracing_renderer.py:265-344) on the 24 surface points of ops.npz's
    light-visibility case (lv_surf / lv_norm / lv_acc / lv_bbox) with xyz = light_xyz_ + noise, for one draw at std 0 and two draws at
    std 1.0 (cfg.light_xyz_noise_std's default).  The std-0 outputs must equal ops.npz's lv_lvis / lv_ldot bit for bit (asserted).
(b) re-shade: render_human of novel_light_sphere_tracing.py (:21-66) under autograd on case RESHADE_CASE of
    synthetic.RESHADE_GRAD_CASES with inputs.xyz = the first noisy draw's positions: rgb, d_albedo, d_roughness, d_probe.

Seed condition.  Its purpose: no ray of the set sits on one of the DFSS state machine's fp32 coin tosses (an accept condition decided by
the last bits of a distance), so that every ray can be held to a bound.  A noisy draw is kept only if
  1. the fp32 oracle (oracle/ra_oracle.py light_visibility with net.light_xyz moved) agrees with the reference on EVERY ray of (a) within
     half of tests/test_oracle_golden.py::test_light_visibility's tolerances (ldot 1e-6 / 2, lvis 2e-4 / 2), and
  2. the reference agrees with the FLOAT64 oracle on every ray within half of the all-compensated tier's bound (lvis 1e-3 / 2).
Condition 1 alone does not serve the purpose: the oracle restates the reference operation by operation, so the two take the same side of
a coin toss.  Seed 5 passes it with one ray (light 252, point 10) where both give 1.0 and the float64 evaluation 0.97007: 3.0e-2 of fp32
arithmetic, not of any kernel.  Condition 2 is the reference's own error against exact arithmetic; nothing in it comes from the device.
Seeds 1, 2, ... are tried, eight at the most, the first two that pass both are kept; every seed tried is recorded in `_about` with its
maxima under both conditions.  The reference never travels: only this fixture is committed.
"""
import argparse
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from make_golden import install_reference, set_cfg, to_ref_batch

OUT = 'light_noise.npz'
STD = 1.0
RESHADE_CASE = 'default'
MAX_SEEDS = 8
LDOT_TOL, LVIS_TOL = 1e-6, 2e-4          # test_oracle_golden.py::test_light_visibility
COMP_TOL = 1e-3                          # test_gpu_parity.py::test_unused_stage_fixtures, trace_precision 2: max |lvis - reference|


def draw(seed, std, n):
    """the reference's randn_like * std with an explicit generator"""
    return torch.randn(n, 3, generator=torch.Generator().manual_seed(seed)) * std


def to_dtype(o, dt):
    """every floating tensor that o holds (attributes, dict values), in place"""
    if isinstance(o, torch.Tensor):
        return o.to(dt) if o.is_floating_point() else o
    if isinstance(o, dict):
        for k in list(o):
            o[k] = to_dtype(o[k], dt)
    elif isinstance(o, (list, tuple)):
        return type(o)(to_dtype(v, dt) for v in o)
    elif hasattr(o, '__dict__'):
        for k, v in list(vars(o).items()):
            setattr(o, k, to_dtype(v, dt))
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--check', action='store_true', help='compare with the committed file instead of writing it')
    args = ap.parse_args()
    from oracle import ra_oracle as O
    from relightableavatar_amd import synthetic
    from relightableavatar_amd.config import make_cfg
    with np.load(os.path.join(HERE, 'ops.npz')) as z:
        ops = {k: torch.from_numpy(z[k]) for k in ('lv_surf', 'lv_norm', 'lv_acc', 'lv_bbox', 'lv_lvis', 'lv_ldot')}
    cfg = install_reference()
    set_cfg(cfg, 'ops')
    torch.manual_seed(0)
    torch.set_grad_enabled(True)
    from lib.utils import relight_utils
    from lib.utils.base_utils import dotdict
    from lib.networks.relight.relight_network import Network
    from lib.networks.renderer import sphere_tracing_renderer as st
    from lib.networks.renderer import novel_light_sphere_tracing as nl
    my = make_cfg('relight')
    sd = synthetic.make_state_dict(0, relight=True, cfg=my)
    net = Network()
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and not [m for m in missing if 'embedder' not in m], (missing, unexpected)
    net.eval()
    batch = to_ref_batch(synthetic.make_body(0, posed=True))
    xyz0 = net.light_xyz_.detach().clone()
    L = xyz0.reshape(-1, 3).shape[0]
    dec = lambda x, **k: net.inference_world_distance_field(x, batch, smooth_transition=True, **k)
    shadow_dec = lambda o, d, n, f, *a, **k: st.sphere_tracing(o, d, n, f, dec, None, None, *a, **k)

    def reference_lvis(noise):
        with torch.no_grad():
            lvis, ldot = st.light_visibility(ops['lv_surf'][None], ops['lv_norm'][None], ops['lv_acc'][None], xyz0 + noise.reshape(xyz0.shape), net.light_sharp,
                                             shadow_dec, ops['lv_bbox'][None].clone(), **cfg.obj_lvis)
        return lvis[0].reshape(L, -1), ldot[0].reshape(L, -1)

    o_net = O.OracleNet(sd, my)
    o_xyz0 = o_net.light_xyz.clone()
    frame = O._frame(synthetic.make_body(0, posed=True))

    def oracle_lvis(noise):
        o_net.light_xyz = o_xyz0 + noise.reshape(o_xyz0.shape)
        try:
            return O.light_visibility(o_net, ops['lv_surf'], ops['lv_norm'], ops['lv_acc'], frame, ops['lv_bbox'], my.obj_lvis,
                                      lambda th: (lambda x: O.hdq_sdf(o_net, x, frame, th, True)))
        finally:
            o_net.light_xyz = o_xyz0

    d_net, d_frame = to_dtype(O.OracleNet(sd, my), torch.float64), to_dtype(O._frame(synthetic.make_body(0, posed=True)), torch.float64)

    def oracle_lvis64(noise):
        """the same fp32 inputs, every operation in float64"""
        d_net.light_xyz = (o_xyz0 + noise.reshape(o_xyz0.shape)).double()
        d = lambda t: t.double()
        return O.light_visibility(d_net, d(ops['lv_surf']), d(ops['lv_norm']), d(ops['lv_acc']), d_frame, d(ops['lv_bbox']), my.obj_lvis,
                                  lambda th: (lambda x: O.hdq_sdf(d_net, x, d_frame, th, True)))[0]

    arrs = {'std': np.asarray(STD, np.float32), 'reshade_case': np.asarray(RESHADE_CASE)}
    zero = torch.zeros(L, 3)
    lvis, ldot = reference_lvis(zero)
    assert torch.equal(lvis, ops['lv_lvis']) and torch.equal(ldot, ops['lv_ldot']), 'std 0 must reproduce ops.npz bit for bit'
    arrs.update({'draw0.noise': zero.numpy(), 'draw0.lvis': lvis.numpy(), 'draw0.ldot': ldot.numpy()})
    tried, kept = [], []
    for seed in range(1, MAX_SEEDS + 1):
        noise = draw(seed, STD, L)
        lvis, ldot = reference_lvis(noise)
        o_lvis, o_ldot = oracle_lvis(noise)
        e_lvis, e_ldot = (o_lvis - lvis).abs(), (o_ldot - ldot).abs()
        bad = int(((e_lvis > LVIS_TOL / 2) | (e_ldot > LDOT_TOL / 2)).sum())
        e64 = (oracle_lvis64(noise) - lvis.double()).abs()
        bad64 = int((e64 > COMP_TOL / 2).sum())
        tried.append(dict(seed=seed, oracle_vs_reference_max_lvis=float(e_lvis.max()), oracle_vs_reference_max_ldot=float(e_ldot.max()),
                          rays_over_half_tolerance=bad, reference_vs_float64_max_lvis=float(e64.max()), rays_off_float64=bad64,
                          kept=bad == 0 and bad64 == 0))
        print(tried[-1])
        if bad == 0 and bad64 == 0:
            kept.append(seed)
            k = len(kept)
            arrs.update({f'draw{k}.noise': noise.numpy(), f'draw{k}.lvis': lvis.numpy(), f'draw{k}.ldot': ldot.numpy(), f'draw{k}.seed': np.asarray(seed)})
            assert float((lvis - ops['lv_lvis']).abs().mean()) > 0.0
        if len(kept) == 2:
            break
    assert len(kept) == 2, ('fewer than two of the eight seeds qualify', tried)
    # (b) the re-shade under the first noisy draw's positions
    x = synthetic.reshade_case_inputs(RESHADE_CASE)
    c = make_cfg('relight', **synthetic.RESHADE_GRAD_CASES[RESHADE_CASE]['cfg'])
    xyz, area = relight_utils.gen_light_xyz(my.env_h, my.env_w, my.env_r, device='cpu')
    assert torch.equal(xyz.reshape(-1, 3), xyz0.reshape(-1, 3))
    mf = relight_utils.Microfacet(f0=c.fresnel_f0, lambert_only=c.lambert_only, glossy_only=c.glossy_only)
    albedo, rough, probes = (t.clone().requires_grad_(True) for t in (x.albedo, x.rough, x.probes))
    moved = xyz + torch.from_numpy(arrs['draw1.noise']).reshape(xyz.shape)
    rgbs = []
    for q in range(probes.shape[0]):
        inputs = dotdict(xyz=moved, area=area, microfacet=mf, envmap=dotdict(probe=probes[q][None]))
        rgb, _, _ = nl.render_human(x.ray_o[None], x.surf[None], x.norm[None], albedo[None], rough[None, :, None], x.lvis[None], x.ldot[None], inputs)
        rgbs.append(rgb[0])
    rgb = torch.stack(rgbs)
    (rgb * x.d_rgb).sum().backward()
    out = dict(rgb=rgb.detach(), d_albedo=albedo.grad, d_roughness=rough.grad, d_probe=probes.grad)
    for k, v in out.items():
        assert torch.isfinite(v).all(), k
        arrs[f'reshade.{k}'] = v.detach().numpy()
    arrs['_about'] = np.asarray(json.dumps(dict(std=STD, max_seeds=MAX_SEEDS, half_tolerances=dict(lvis=LVIS_TOL / 2, ldot=LDOT_TOL / 2, lvis_vs_float64=COMP_TOL / 2),
                                                seeds_tried=tried, seeds_kept=kept, reshade_case=RESHADE_CASE, reshade_noise='draw1')))
    path = os.path.join(HERE, OUT)
    if args.check:
        with np.load(path) as z:
            assert sorted(z.files) == sorted(arrs), (sorted(z.files), sorted(arrs))
            for k in z.files:
                assert z[k].dtype == arrs[k].dtype and np.array_equal(z[k], arrs[k]), k
        print('identical to', OUT, len(arrs), 'arrays')
        return
    np.savez_compressed(path, **arrs)
    print('wrote', OUT, len(arrs), 'arrays', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

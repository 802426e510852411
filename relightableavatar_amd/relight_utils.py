"""Device-side mirror of the reference's environment-map utilities.

    rotate_envmap(novel_light, index, repeat, probe_width, image_width)   lib/utils/relight_utils.py:57-103
    add_light_probe(rgb, probe, batch, cfg)                               lib/utils/relight_utils.py:38-54 (+ gen_light_dir :9-35)
    gen_light_xyz(env_h, env_w, env_r)                                    lib/utils/relight_utils.py:423-465 (host, once per network)

Same names, argument meaning and return values as the reference plus the engine that owns the HIP context; there is no
CPU fallback.
"""
import math

import torch

from .base_utils import dotdict


def rotate_envmap(novel_light, index, repeat, probe_width, image_width, engine):
    keys = list(novel_light.keys())
    if repeat <= 0:
        return keys[index], novel_light[keys[index]]
    n_rotation = probe_width * repeat
    i, j = index // n_rotation, index % n_rotation
    name = f'{keys[i]}-{j:04d}'
    envmap = novel_light[keys[i]]
    eW = envmap.probe.shape[-2]
    uW = eW * repeat
    out = dotdict(probe=engine.shift_envmap(envmap.probe, eW / uW * j))
    if 'image' in envmap:
        out.image = engine.shift_envmap(envmap.image, envmap.image.shape[-2] / uW * j)
    return name, out


def add_light_probe(rgb, probe, batch, cfg, engine):
    H, W = int(batch.meta.H.item()), int(batch.meta.W.item())
    uW = int(W * cfg.probe_size_ratio)
    uH = int(uW * cfg.env_h / cfg.env_w)
    return engine.add_light_probe(rgb, probe, H, W, batch.cam_R[0], uH, uW).reshape(rgb.shape)


def gen_light_xyz(env_h: int, env_w: int, env_r: float):
    """Light-probe geometry; restates lib/utils/relight_utils.py:423-465 (lat/long cell centres)."""
    lat_half = math.pi / env_h / 2
    lng_half = 2 * math.pi / env_w / 2
    lats = torch.linspace(math.pi / 2 - lat_half, -math.pi / 2 + lat_half, env_h)
    lngs = torch.linspace(math.pi - lng_half, -math.pi + lng_half, env_w)
    lngs, lats = torch.meshgrid(lngs, lats, indexing='xy')  # (eH, eW)
    z = env_r * torch.sin(lats)
    x = env_r * torch.cos(lats) * torch.cos(lngs)
    y = env_r * torch.cos(lats) * torch.sin(lngs)
    xyz = torch.stack((x, y, z), dim=-1)
    sin_colat = torch.sin(math.pi / 2 - lats)
    area = 4 * math.pi * sin_colat / torch.sum(sin_colat)
    return xyz, area


class _Reshade(torch.autograd.Function):
    """rgb of Engine.reshade with its gradient: forward = ra_reshade, backward = ra_reshade_backward.  light_xyz (L,3) or None: the light
    positions the op is evaluated under.  The op carries them: a loss summed over several frames calls backward() once, so every frame's
    ra_reshade_backward runs after the LAST frame's forward — the backward sets the positions of its own forward again."""

    @staticmethod
    def forward(ctx, eng, ray_o, surf, norm, albedo, rough, lvis, ldot, probes, light_xyz):
        ctx.eng = eng
        ctx.moved = light_xyz is not None
        if not ctx.moved:
            rgb, _, _ = eng.reshade(ray_o, surf, norm, albedo, rough, lvis, ldot, probes, want_spec=False)
            ctx.save_for_backward(ray_o, surf, norm, albedo, rough, lvis, ldot, probes)
            return rgb
        light_xyz = light_xyz.detach()
        with eng.light_positions(light_xyz):
            rgb, _, _ = eng.reshade(ray_o, surf, norm, albedo, rough, lvis, ldot, probes, want_spec=False)
        ctx.save_for_backward(ray_o, surf, norm, albedo, rough, lvis, ldot, probes, light_xyz)
        return rgb

    @staticmethod
    def backward(ctx, d_rgb):
        ray_o, surf, norm, albedo, rough, lvis, ldot, probes = ctx.saved_tensors[:8]
        want = tuple(ctx.needs_input_grad[i] for i in (4, 5, 8))
        run = lambda: ctx.eng.reshade_backward(ray_o, surf, norm, albedo, rough, lvis, ldot, probes, d_rgb, want=want)
        if ctx.moved:
            with ctx.eng.light_positions(ctx.saved_tensors[8]):
                d_alb, d_rgh, d_prb = run()
        else:
            d_alb, d_rgh, d_prb = run()
        shaped = lambda g, like: None if g is None else g.reshape(like.shape).to(like.dtype)
        return (None, None, None, None, shaped(d_alb, albedo), shaped(d_rgh, rough), None, None, shaped(d_prb, probes), None)


def reshade(eng, ray_o, surf, norm, albedo, rough, lvis, ldot, probes, light_xyz=None):
    """Differentiable novel-light re-shade (novel_light_sphere_tracing.render_human :21-66): probes (n,h,w,3) -> rgb (n,P,3).
    Gradients reach albedo, rough and probes only — the relighting stage's (relight_trainer.py:113-118): geometry is frozen and the
    light visibility was computed without gradients.  Engine.reshade is the plain (no-autograd) call.
    light_xyz (L,3): shade under these light positions (inputs.xyz of render_human: light_xyz_ plus the trainer's noise,
    relight_network.py:79-84) — lvis / ldot are the caller's, traced under the same positions (Engine.light_visibility).  The forward sets
    them and the backward sets them again, whatever ran in between; both leave the engine at the LOADED positions.  None: the engine's
    current positions, and no call beyond ra_reshade / ra_reshade_backward is made."""
    return _Reshade.apply(eng, ray_o, surf, norm, albedo, rough, lvis, ldot, probes, light_xyz)


class _MaterialHeads(torch.autograd.Function):
    """the two material heads on cached features: forward = ra_heads_forward, backward = ra_heads_backward (feat is a constant)"""

    @staticmethod
    def forward(ctx, eng, theta, feat):
        albedo, rough = eng.heads_forward(theta, feat)
        ctx.eng = eng
        ctx.save_for_backward(theta, feat)
        return albedo, rough

    @staticmethod
    def backward(ctx, d_albedo, d_rough):
        theta, feat = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None
        d_theta = ctx.eng.heads_backward(theta, feat, d_albedo, d_rough)
        return None, d_theta.reshape(theta.shape).to(theta.dtype), None


def material_heads(eng, theta, feat):
    """Differentiable material heads (relight_network.py:45-47,91-104) on cached surface features: theta (99332,) in the flat layout of
    Engine.heads_params, feat (n,256) -> albedo (n,3), roughness (n,).  The gradient reaches theta only; n == 0 gives a zero gradient.
    Engine.heads_forward is the plain (no-autograd) call."""
    return _MaterialHeads.apply(eng, theta, feat)


class _GaussianEntropy(torch.autograd.Function):
    """forward = ra_gaussian_entropy with the gradient kept; backward scales it by the incoming scalar"""

    @staticmethod
    def forward(ctx, eng, x):
        value, d_x = eng.gaussian_entropy(x, want_grad=True)
        ctx.save_for_backward(d_x)
        ctx.x_shape, ctx.x_dtype = x.shape, x.dtype
        return value

    @staticmethod
    def backward(ctx, d_value):
        d_x, = ctx.saved_tensors
        return None, (d_x * d_value).reshape(ctx.x_shape).to(ctx.x_dtype)


def gaussian_entropy(eng, x):
    """Differentiable Gaussian-histogram entropy of x (..., 3) (loss_utils.py:51-76, the albedo sparsity term of relight_trainer.py:70-81):
    a 0-dim tensor.  A constant channel contributes 0 and a zero gradient (the reference's autograd returns NaN there).
    Engine.gaussian_entropy is the plain (no-autograd) call."""
    return _GaussianEntropy.apply(eng, x)

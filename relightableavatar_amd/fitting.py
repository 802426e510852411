"""Light and material fitting from a traced frame: the relighting stage's optimisation (lib/train/trainers/relight_trainer.py:113-118)
on the cached maps of one frame.  Geometry and light visibility are frozen; the image loss reaches the probe, the albedo and the
roughness through the shading sum alone.  PyTorch is plumbing here (parameters, Adam, the loss); the hot path is the two C calls
behind relight_utils.reshade: ra_reshade and ra_reshade_backward.
"""
import torch
import torch.nn.functional as F

from .base_utils import dotdict
from .relight_utils import reshade


def _inv_softplus(y):
    return y + torch.log(-torch.expm1(-y))


def _logit(x):
    x = x.clamp(1e-4, 1 - 1e-4)
    return torch.log(x) - torch.log1p(-x)


def init_probe_param(cfg, probe_hw=None, achro_light=None, generator=None):
    """global_env_map_ as relight_network.py:63-66 initialises it: rand * envmap_init_intensity, one channel under achro_light"""
    achro = cfg.achro_light if achro_light is None else achro_light
    h, w = probe_hw if probe_hw is not None else (cfg.env_h * cfg.envmap_upscale, cfg.env_w * cfg.envmap_upscale)
    return torch.rand(h, w, 1 if achro else 3, generator=generator) * cfg.envmap_init_intensity


def fit_relight(eng, maps, target_rgb, *, mask=None, steps, lr, fit_probe=True, fit_albedo=False, fit_roughness=False, probe_hw=None,
                achro_light=None, probe_init=None, generator=None):
    """Fit the environment probe and / or the per-pixel albedo and roughness of one traced frame to a photograph of it.

    maps: what the sphere-tracing / novel-light renderer returns for the frame (ray_o, surf_map, norm_map, albedo_map, roughness_map,
    lvis_map, ldot_map); target_rgb (P,3), tone-mapped like the renderer's rgb_map; mask (P,) bool: the pixels that count.
    Parametrisation as the reference: probe = softplus(param) (relight_network.py:86-89; one channel expanded to three under
    achro_light), initialised as :63-66 — or, with probe_init (h,w,3) > 0, at that probe (a probe that is not fitted must be given);
    albedo = albedo_slope * sigmoid + albedo_bias, roughness = roughness_slope * sigmoid + roughness_bias per pixel (:46-47),
    initialised at the maps' values.  Loss: the image MSE (relight_trainer.py:114); optimiser: Adam.
    Returns dotdict(probe (h,w,3), albedo_map (P,3), roughness_map (P,), loss: list of `steps + 1` floats — before every step and
    after the last)."""
    cfg, dev = eng.cfg, eng.device
    f = lambda t, *s: t.detach().to(dev, torch.float32).reshape(*s).contiguous()
    ray_o, surf, norm = f(maps.ray_o, -1, 3), f(maps.surf_map, -1, 3), f(maps.norm_map, -1, 3)
    P = ray_o.shape[0]
    albedo0, rough0 = f(maps.albedo_map, P, 3), f(maps.roughness_map, P)
    lvis, ldot = f(maps.lvis_map, P, -1), f(maps.ldot_map, P, -1)
    target = f(target_rgb, P, 3)
    keep, albedo_full, rough_full = None, albedo0, rough0
    if mask is not None:
        keep = mask.to(dev).reshape(P).bool()
        ray_o, surf, norm, albedo0, rough0, lvis, ldot, target = (t[keep].contiguous() for t in (ray_o, surf, norm, albedo0, rough0, lvis, ldot, target))

    if probe_init is not None:
        p_param = _inv_softplus(f(probe_init, *probe_init.shape[-3:]).clamp_min(1e-6))
    else:
        if not fit_probe:
            raise ValueError('fit_relight: a probe that is not fitted must be given (probe_init)')
        p_param = init_probe_param(cfg, probe_hw, achro_light, generator).to(dev)
    a_param = _logit((albedo0 - cfg.albedo_bias) / cfg.albedo_slope)
    r_param = _logit((rough0 - cfg.roughness_bias) / cfg.roughness_slope)
    params = []
    for p, fit in ((p_param, fit_probe), (a_param, fit_albedo), (r_param, fit_roughness)):
        p.requires_grad_(bool(fit))
        if fit:
            params.append(p)
    if not params:
        raise ValueError('fit_relight: nothing to fit')
    opt = torch.optim.Adam(params, lr=lr)

    def current():
        probe = F.softplus(p_param.expand(*p_param.shape[:2], 3))
        albedo = cfg.albedo_slope * torch.sigmoid(a_param) + cfg.albedo_bias if fit_albedo else albedo0
        rough = cfg.roughness_slope * torch.sigmoid(r_param) + cfg.roughness_bias if fit_roughness else rough0
        return probe, albedo, rough

    def loss_fn():
        probe, albedo, rough = current()
        rgb = reshade(eng, ray_o, surf, norm, albedo, rough, lvis, ldot, probe[None])[0]
        return F.mse_loss(rgb, target)

    history = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = loss_fn()
        loss.backward()
        opt.step()
        history.append(loss.detach())
    with torch.no_grad():
        history.append(loss_fn())
        probe, albedo, rough = current()
        if keep is not None:      # the fitted values of the pixels that counted, the maps' own elsewhere
            albedo_full, rough_full = albedo_full.clone(), rough_full.clone()
            albedo_full[keep], rough_full[keep] = albedo, rough
            albedo, rough = albedo_full, rough_full
    return dotdict(probe=probe.detach().contiguous(), albedo_map=albedo.detach(), roughness_map=rough.detach(),
                   loss=[float(x) for x in torch.stack(history).cpu()])

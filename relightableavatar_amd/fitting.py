"""Light and material fitting from a traced frame: the relighting stage's optimisation (lib/train/trainers/relight_trainer.py:113-118)
on the cached maps of one frame.  Geometry and light visibility are frozen; the image loss reaches the probe, the albedo and the
roughness through the shading sum alone.  PyTorch is plumbing here (parameters, Adam, the loss); the hot path is the two C calls
behind relight_utils.reshade: ra_reshade and ra_reshade_backward.

fit_heads trains what the reference's relighting stage trains — the weights of the two material networks (relight_network.py:45-47) and
the probe — on cached surface features of one or more traced frames: relight_utils.material_heads (ra_heads_forward / ra_heads_backward)
in front of the same re-shade.  With regularisers it minimises the trainer's loss (relight_trainer.py:70-91,113-118): the image MSE plus
the Gaussian-histogram entropy of the per-sample and of the composited albedo (relight_utils.gaussian_entropy: ra_gaussian_entropy) and
the L1 distance of both heads' outputs from their outputs at jittered canonical points (Engine.canonical_features:
ra_canonical_features on cpts + noise, fresh every step).  With light_noise it also moves the lights every step as the reference's network does
in training mode (relight_network.py:79-84) and traces the frames' light visibility again under the moved lights
(Engine.light_visibility: ra_set_light_xyz, ra_light_visibility), on all counted pixels or on pixels_per_step of them.
"""
import functools

import torch
import torch.nn.functional as F

from .base_utils import dotdict
from .relight_utils import gaussian_entropy, gen_light_xyz, material_heads, reshade


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


def _frame_cache(eng, cfg, batch, maps, target_rgb, mask, premultiplied, retrace=False):
    """what a frame contributes to every step of fit_heads: features of the surface samples of the pixels that count, their constant
    compositing weights, the cached shading maps and the target.  retrace (fit_heads' light noise): instead of the cached lvis / ldot —
    two n x 512 tables that moved lights make useless — the inputs of Engine.light_visibility: the frame's batch, the counted pixels'
    surface points, normals and acc, and the shadow rays' box"""
    dev = eng.device
    f = lambda t, *s: t.detach().to(dev, torch.float32).reshape(*s).contiguous()
    eng.set_frame(batch)
    acc = f(maps.acc_map, -1)
    P, S = acc.shape[0], int(cfg.n_samples)
    hit = acc > 0
    raw = f(maps['raw'], -1, S, 17)                       # per hit pixel in ascending ray order: cpts, bpts, resd, albedo, rough, norm, occ
    if raw.shape[0] != int(hit.sum()):
        raise ValueError('fit_heads: maps.raw does not match maps.acc_map (render the frame with cfg.ret_raw)')
    keep = hit if mask is None else hit & mask.to(dev).reshape(P).bool()
    raw = raw[keep[hit]]
    occ = raw[..., 16]
    # volume_rendering (net_utils.py:970-999) on the samples' occupancies, divided by the accumulated weight (sphere_tracing_renderer.py:
    # render_human): constants of the fit, geometry is frozen
    trans = torch.cumprod(torch.cat([torch.ones_like(occ[:, :1]), 1.0 - occ + 1e-8], dim=-1), dim=-1)[:, :-1]
    w = occ * trans
    o = w.sum(-1)
    c = dotdict()
    c.w = (w / (o[:, None] + 1e-8)).contiguous()
    c.bg = ((1.0 - o) * cfg.bg_brightness / (o + 1e-8)).contiguous()
    # the features twice over: rows [0, n) the samples' own (cached), rows [n, 2n) rewritten every step with the features at the jittered
    # canonical points (regulariser_terms) — one heads call then covers both, with no concatenation per step
    n = raw.shape[0] * S
    c.cpts = raw[..., 0:3].reshape(-1, 3).contiguous()     # the kernel's own fp32 bpts + resd
    c.feat2 = torch.empty(2 * n, 256, device=dev)
    c.feat2[:n] = eng.bigpose_features(raw[..., 3:6].reshape(-1, 3))
    c.feat = c.feat2[:n]
    c.scale = acc[keep].contiguous() if premultiplied else torch.ones_like(acc[keep])      # alpha_output_: the maps are premultiplied by acc
    c.ray_o, c.surf, c.norm = (f(t, P, 3)[keep].contiguous() for t in (maps.ray_o, maps.surf_map, maps.norm_map))
    if retrace:
        c.lvis = c.ldot = None
        c.batch, c.acc = batch, acc[keep].contiguous()
        # the stage traces from the surface point itself: the maps are premultiplied by acc (x / 1 is x: pixels with acc == 1, nearly all, are
        # handed over bit for bit)
        c.surf_pts, c.norm_pts = ((t / c.acc[:, None]).contiguous() for t in (c.surf, c.norm)) if premultiplied else (c.surf, c.norm)
        c.bbox = [float(v) for v in batch.wbounds.detach().reshape(-1).cpu()]      # as the frame's render left it (grown in place, quirk 1)
    else:
        c.lvis, c.ldot = (f(t, P, -1)[keep].contiguous() for t in (maps.lvis_map, maps.ldot_map))
    c.target = f(target_rgb, P, 3)[keep].contiguous()
    c.S, c.premultiplied = S, bool(premultiplied)
    return c


def composite_heads(cfg, c, albedo_s, rough_s, want_volume=False):
    """per-sample head outputs (n_pixels * S, 3), (n_pixels * S,) -> albedo_map (n_pixels, 3), roughness_map (n_pixels,) as render_human
    composites them: volume-rendering weights over the accumulated weight, clipped to [bias, bias + slope], albedo times
    albedo_multiplier — and times acc where the renderer premultiplies its maps.  want_volume: a third output, the clipped albedo
    composite before albedo_multiplier and before the premultiplication: ret.volume_albedo (sphere_tracing_renderer.py:645-647)"""
    n = c.w.shape[0]
    a = (c.w[..., None] * albedo_s.reshape(n, c.S, 3)).sum(1) + c.bg[:, None]
    r = (c.w * rough_s.reshape(n, c.S)).sum(1) + c.bg
    a = a.clamp(cfg.albedo_bias, cfg.albedo_bias + cfg.albedo_slope)
    r = r.clamp(cfg.roughness_bias, cfg.roughness_bias + cfg.roughness_slope)
    volume = a
    if cfg.albedo_multiplier > 0:
        a = a * cfg.albedo_multiplier
    if want_volume:
        return a * c.scale[:, None], r * c.scale, volume
    return a * c.scale[:, None], r * c.scale


def heads_loss(eng, cache, theta, probe, heads=material_heads, shades=None):
    """the loss of fit_heads: the image MSE of every cached frame (_frame_cache) under `probe`, summed; heads(eng, theta, feat) ->
    albedo, roughness per sample (tools/bench_heads.py swaps in a torch evaluation to time against); shades: one re-shade op per frame
    (step_frame's, which carries the frame's light positions) instead of relight_utils.reshade"""
    total = 0.0
    for i, c in enumerate(cache):
        albedo, rough = composite_heads(eng.cfg, c, *heads(eng, theta, c.feat))
        rgb = (reshade if shades is None else shades[i])(eng, c.ray_o, c.surf, c.norm, albedo, rough, c.lvis, c.ldot, probe[None])[0]
        total = total + F.mse_loss(rgb, c.target)
    return total


TERMS = ('albedo_entropy', 'volume_entropy', 'albedo_smooth', 'roughness_smooth')
WEIGHTS = ('img_loss_weight', 'albedo_sparsity', 'albedo_smooth_weight', 'roughness_smooth_weight')


def l1(x, y):
    """lib/utils/loss_utils.py l1: abs().sum(-1).mean()"""
    return (x - y).abs().sum(-1).mean()


def regulariser_weights(cfg, regularisers):
    """fit_heads' `regularisers` argument as a dict of the four WEIGHTS: True -> the cfg's, a dict -> its entries over the cfg's"""
    w = {k: float(cfg[k]) for k in WEIGHTS}
    if isinstance(regularisers, dict):
        unknown = set(regularisers) - set(WEIGHTS)
        if unknown:
            raise ValueError(f'fit_heads: unknown regulariser weights {sorted(unknown)} (known: {WEIGHTS})')
        w.update({k: float(v) for k, v in regularisers.items()})
    elif regularisers is not True:
        raise ValueError('fit_heads: regularisers is None, True or a dict of weights')
    return w


def frame_terms(eng, c, theta, noise, probe=None, grad=(True, True, True), heads=material_heads, entropy=gaussian_entropy, shade=reshade):
    """one cached frame's terms of the trainer's loss, unweighted (relight_trainer.py:70-91,113-118): albedo_entropy (per-sample albedo),
    volume_entropy (the composited albedo, ret.volume_albedo), albedo_smooth and roughness_smooth (l1 of the samples' outputs against
    their outputs at cpts + noise) and — with a probe (h,w,3) — img_loss.  noise: (n_samples,3) on the device.
    grad = (entropies, albedo_smooth, roughness_smooth): a term whose weight is zero is only reported — it is evaluated without a graph,
    and with both smoothness terms off the differentiable heads call covers the cached features alone, exactly as without regularisers.
    heads / entropy / shade: the three device ops (tests and tools swap in torch evaluations)."""
    cfg, n = eng.cfg, c.cpts.shape[0]
    with torch.no_grad():
        eng.canonical_features(c.cpts + noise.reshape(n, 3), out=c.feat2[n:])
    jitter_grad = grad[1] or grad[2]
    if jitter_grad:
        albedo2, rough2 = heads(eng, theta, c.feat2)
        albedo_s, rough_s, albedo_j, rough_j = albedo2[:n], rough2[:n], albedo2[n:], rough2[n:]
    else:
        albedo_s, rough_s = heads(eng, theta, c.feat)
        with torch.no_grad():
            albedo_j, rough_j = heads(eng, theta.detach(), c.feat2[n:])
    albedo, rough, volume = composite_heads(cfg, c, albedo_s, rough_s, want_volume=True)
    out = dotdict()
    with torch.set_grad_enabled(torch.is_grad_enabled() and grad[0]):
        out.albedo_entropy = entropy(eng, albedo_s)
        out.volume_entropy = entropy(eng, volume)
    with torch.set_grad_enabled(torch.is_grad_enabled() and grad[1]):
        out.albedo_smooth = l1(albedo_s, albedo_j)
    with torch.set_grad_enabled(torch.is_grad_enabled() and grad[2]):
        out.roughness_smooth = l1(rough_s[:, None], rough_j[:, None])
    if probe is not None:
        rgb = shade(eng, c.ray_o, c.surf, c.norm, albedo, rough, c.lvis, c.ldot, probe[None])[0]
        out.img_loss = F.mse_loss(rgb, c.target)
    return out


def regulariser_terms(eng, c, theta, noise):
    """the four unweighted regulariser terms (TERMS) of one cached frame (_frame_cache) under explicit noise (n_samples,3)"""
    t = frame_terms(eng, c, theta, noise)
    return dotdict({k: t[k] for k in TERMS})


def regularised_loss(eng, cache, theta, probe, weights, noises, shades=None, **ops):
    """the trainer's loss over the cached frames, summed: img_loss_weight * mse + albedo_sparsity * (H(albedo samples) + H(volume albedo))
    + albedo_smooth_weight * l1(albedo, albedo_jitter) + roughness_smooth_weight * l1(roughness, roughness_jitter) per frame.
    shades: one re-shade op per frame (step_frame's) instead of ops['shade'] / relight_utils.reshade.
    Returns (total, dotdict of the unweighted terms summed over the frames, detached)."""
    w = weights
    grad = (w['albedo_sparsity'] != 0, w['albedo_smooth_weight'] != 0, w['roughness_smooth_weight'] != 0)
    total, sums = 0.0, dotdict()
    for i, (c, noise) in enumerate(zip(cache, noises)):
        if shades is not None:
            ops['shade'] = shades[i]
        t = frame_terms(eng, c, theta, noise, probe, grad, **ops)
        total = total + (w['img_loss_weight'] * t.img_loss + w['albedo_sparsity'] * (t.albedo_entropy + t.volume_entropy) +
                         w['albedo_smooth_weight'] * t.albedo_smooth + w['roughness_smooth_weight'] * t.roughness_smooth)
        for k, v in t.items():
            sums[k] = v.detach() + (sums[k] if k in sums else 0.0)
    return total, sums


def step_options(cfg, light_noise, light_noise_fn, pixels_per_step, pixel_fn):
    """fit_heads' light_noise / light_noise_fn / pixels_per_step / pixel_fn arguments checked: (noisy, std of the default draw, pixels per
    step as an int or None)"""
    if light_noise is not None and light_noise is not True and (isinstance(light_noise, bool) or not isinstance(light_noise, (int, float))):
        raise ValueError('fit_heads: light_noise is None, True or a std')
    std = float(cfg.light_xyz_noise_std) if light_noise is True or light_noise is None else float(light_noise)
    if not std >= 0.0:
        raise ValueError('fit_heads: light_noise must be a std >= 0')
    if light_noise_fn is not None and not callable(light_noise_fn):
        raise ValueError('fit_heads: light_noise_fn(step, frame) -> (L, 3) must be callable')
    if pixels_per_step is not None and (isinstance(pixels_per_step, bool) or not isinstance(pixels_per_step, int) or pixels_per_step < 1):
        raise ValueError('fit_heads: pixels_per_step is None or a positive number of pixels')
    if pixel_fn is not None and (pixels_per_step is None or not callable(pixel_fn)):
        raise ValueError('fit_heads: pixel_fn(step, frame, n_pixels) chooses pixels_per_step pixels: give pixels_per_step')
    return light_noise is not None or light_noise_fn is not None, std, pixels_per_step


def loaded_light_xyz(net, cfg, dev):
    """light_xyz_ (L,3) on the device: the network's buffer, or — for a bare Engine — what the network generates it from (relight_network.py)"""
    xyz = getattr(net, 'light_xyz_', None) if net is not None else None
    if xyz is None:
        xyz = gen_light_xyz(cfg.env_h, cfg.env_w, cfg.env_r)[0]
    return xyz.detach().to(dev, torch.float32).reshape(-1, 3).contiguous()


def step_frame(eng, c, probe, rows=None, light_xyz=None):
    """one frame of one step of fit_heads under a pixel subset and / or moved lights: (view, shade).  view: the frame's cache
    (_frame_cache) restricted to the pixels `rows` (int64 (N,) on the device, distinct indices into the counted pixels; None: all of them)
    — the pixels' rows of every per-pixel table and their samples' rows of every per-sample one, gathered.  light_xyz (L,3): the frame was
    cached with retrace; its batch is set, the lights are moved for the duration of the trace, and view.lvis / view.ldot are
    Engine.light_visibility of the rows under light_xyz with `probe` (h,w,3) as the key-light probe — times acc where the renderer
    premultiplies its maps, as the cached maps are.  shade: relight_utils.reshade carrying light_xyz."""
    v = c
    if rows is not None:
        n, S = c.w.shape[0], c.S
        v = dotdict(c)
        for k in ('w', 'bg', 'scale', 'ray_o', 'surf', 'norm', 'target'):
            v[k] = c[k][rows]
        N = rows.shape[0]
        v.cpts = c.cpts.reshape(n, S, 3)[rows].reshape(N * S, 3)
        v.feat2 = torch.empty(2 * N * S, 256, device=c.feat.device)
        v.feat2[:N * S] = c.feat.reshape(n, S, 256)[rows].reshape(N * S, 256)
        v.feat = v.feat2[:N * S]
        if light_xyz is None:
            v.lvis, v.ldot = c.lvis[rows], c.ldot[rows]
    if light_xyz is None:
        return v, reshade
    if v is c:
        v = dotdict(c)
    with torch.no_grad():      # light visibility carries no gradient (sphere_tracing_renderer.py:265: under no_grad)
        eng.set_frame(c.batch)
        with eng.light_positions(light_xyz):
            lvis, ldot = eng.light_visibility(c.surf_pts, c.norm_pts, c.acc, c.bbox, probe=probe.detach(),
                                              rows=None if rows is None else rows.to(torch.int32))
        if c.premultiplied:
            lvis, ldot = lvis * v.scale[:, None], ldot * v.scale[:, None]
    v.lvis, v.ldot = lvis, ldot
    return v, functools.partial(reshade, light_xyz=light_xyz)


def fit_heads(net_or_eng, frames, *, steps, lr, fit_probe=True, probe_init=None, generator=None, theta_init=None, regularisers=None, noise_fn=None,
              light_noise=None, light_noise_fn=None, pixels_per_step=None, pixel_fn=None):
    """Fit the weights of albedo_network and roughness_network (and the probe) to photographs of traced frames: the relighting stage of
    the reference (relight_trainer.py:113-118) with geometry, surface features and light visibility cached per frame.

    net_or_eng: a relight Network on the GPU, or its Engine.  frames: a list of (batch, maps, target_rgb, mask): maps is what the
    sphere-tracing / novel-light renderer returned for the batch with cfg.ret_raw and cfg.vis_novel_light (acc_map, ray_o, surf_map,
    norm_map, lvis_map, ldot_map, raw); target_rgb (P,3) tone-mapped like the renderer's rgb_map; mask (P,) bool or None.  The pixels that
    count are the hit pixels (acc > 0) inside the mask.
    Per frame, once: set the frame, read the surface samples' big-pose points and occupancies from maps.raw, compute their features
    (Engine.bigpose_features) and the constant compositing weights.  Per step and frame: material_heads -> composite over the n_samples
    surface samples exactly as render_human does (composite_heads) -> reshade -> MSE over the pixels that count; the losses of the frames
    are summed.  One Adam over theta (Engine.heads_params' flat layout; theta_init or the loaded weights) and — with fit_probe — the
    probe parameter (probe = softplus(param), relight_network.py:86-89; started at probe_init (h,w,3) > 0 if given, else at the
    network's own global_env_map_, else as relight_network.py:63-66 initialises it).  A probe that is not fitted is probe_init or the
    network's.
    regularisers: None -> the image MSE alone (no regulariser call is made).  True, or a dict of weights over the cfg's (img_loss_weight,
    albedo_sparsity, albedo_smooth_weight, roughness_smooth_weight) -> the trainer's loss (relight_trainer.py:70-91): regularised_loss.
    The jitter outputs are the heads on the SDF features at cpts + noise (relight_network.py:107-118); noise_fn(step, frame, n) -> (n,3)
    on the device supplies the noise, by default torch.normal(0, cfg.xyz_noise_std) drawn on the device (seeded from `generator`), fresh per
    step and per frame.  A term whose weight is 0 is reported but takes no part in the backward pass.
    light_noise: None -> the lights stay where they were loaded, the cached lvis_map / ldot_map are used and no call beyond today's is made
    (results are bit-identical to a call without the argument).  True -> cfg.light_xyz_noise_std, or a float: that std.  The reference's
    network returns light_xyz_ + randn * std in training mode (relight_network.py:79-84), evaluated once per render call
    (sphere_tracing_renderer.py:1029); that draw moves the shadow rays, the cosines and the probe lookup together.  So per step and
    frame: xyz = light_xyz_ + noise (ONE draw), the rows are chosen, Engine.light_visibility traces them again on the cached surface
    points, normals and acc of the counted pixels with the current probe as the key-light probe, then heads -> composite ->
    reshade(light_xyz=xyz) -> loss.  light_noise_fn(step, frame) -> (L,3) on the device supplies the noise where it must be controlled
    (it alone switches the noise on, too); by default torch.normal(0, std, (L,3)) on the device from a generator seeded from `generator`.
    The cached lvis / ldot tables are not kept then.  The shadow rays' box is batch.wbounds as the frame's render left it (the renderer
    grows it in place, quirk 1): for a frame rendered as one chunk the box its cached visibility was clipped against, for a frame of
    several chunks the LAST chunk's — wider than the box of the earlier chunks' pixels by the margin per chunk.  Frames that share a
    batch object must have been rendered the same way.
    pixels_per_step: None -> every counted pixel every step.  N -> every step and frame uses N of the frame's counted pixels (the
    reference's train batch; the visibility stage of a whole frame every step is the cost of a rendered frame); a frame with fewer counts
    whole.  pixel_fn(step, frame, n_pixels) -> int64 (N,) distinct indices below n_pixels on the device controls the choice (the indices
    are not checked: a check would read them back every step); the default is a randperm prefix drawn on the device.  The entropy and
    smoothness terms then run over the chosen pixels' samples, and noise_fn is asked for N * n_samples rows.  Usable without light
    noise: the rows of the cached visibility are gathered.
    On return and on any exception the engine's light positions are the loaded ones.
    Still out of scope: the training-mode acc (sphere_tracing_renderer.py:593-598: the geometry is frozen); the normal / visibility
    smoothness terms (:93-111) belong to outputs the relighting stage does not train here.
    Returns dotdict(state_dict: the twelve head keys (+ 'global_env_map_' when the probe was fitted) on the host, for
    net.load_state_dict(..., strict=False); theta; probe (h,w,3); loss: `steps + 1` floats, before every step and after the last; with
    regularisers also terms: per name (img_loss and TERMS, unweighted, summed over the frames) a list like loss)."""
    net = None if hasattr(net_or_eng, 'heads_params') else net_or_eng
    noisy, light_std, pixels_per_step = step_options(net_or_eng.cfg, light_noise, light_noise_fn, pixels_per_step, pixel_fn)
    eng = net_or_eng if net is None else net.engine()
    cfg, dev = eng.cfg, eng.device
    premultiplied = not bool(cfg.get('vis_ground_shading', False))
    stepwise = noisy or pixels_per_step is not None      # a frame's tables are rebuilt every step (step_frame)
    with torch.no_grad():
        cache = [_frame_cache(eng, cfg, b, m, t, k, premultiplied, **(dict(retrace=True) if noisy else {})) for b, m, t, k in frames]
        theta = (eng.heads_params() if theta_init is None else theta_init.detach().to(dev, torch.float32).reshape(-1)).clone()
        own = getattr(net, 'global_env_map_', None) if net is not None else None
        if probe_init is not None:
            p_param = _inv_softplus(probe_init.detach().to(dev, torch.float32).reshape(*probe_init.shape[-3:]).clamp_min(1e-6))
        elif own is not None:
            p_param = own.detach().to(dev, torch.float32).clone()
        elif fit_probe:
            p_param = init_probe_param(cfg, None, None, generator).to(dev)
        else:
            raise ValueError('fit_heads: a probe that is not fitted must be given (probe_init, or a network that carries one)')
    theta.requires_grad_(True)
    p_param.requires_grad_(bool(fit_probe))
    opt = torch.optim.Adam([theta] + ([p_param] if fit_probe else []), lr=lr)

    current_probe = lambda: F.softplus(p_param.expand(*p_param.shape[:2], 3))
    history, terms = [], []

    def device_generator():
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(torch.randint(2 ** 62, (1,), generator=generator)))
        return gen

    if regularisers is not None:
        weights = regulariser_weights(cfg, regularisers)
        if noise_fn is None:
            gen = device_generator()
            std = float(cfg.xyz_noise_std)
            noise_fn = lambda step, frame, n: torch.normal(0.0, std, (n, 3), generator=gen, device=dev)
    if noisy:
        xyz0 = loaded_light_xyz(net, cfg, dev)
        if light_noise_fn is None:
            light_gen = device_generator()
            light_noise_fn = lambda step, frame: torch.normal(0.0, light_std, (xyz0.shape[0], 3), generator=light_gen, device=dev)
    if pixels_per_step is not None and pixel_fn is None:
        pixel_gen = device_generator()
        pixel_fn = lambda step, frame, n: torch.randperm(n, generator=pixel_gen, device=dev)[:int(pixels_per_step)]

    def step_frames(step, probe):
        """every frame's view and re-shade op of this step: one noise draw, then one choice of rows, per frame"""
        views, shades = [], []
        for i, c in enumerate(cache):
            xyz = xyz0 + light_noise_fn(step, i).to(dev, torch.float32).reshape(-1, 3) if noisy else None
            n = c.w.shape[0]
            rows = pixel_fn(step, i, n).to(dev, torch.int64).reshape(-1) if pixels_per_step is not None and n > int(pixels_per_step) else None
            v, shade = step_frame(eng, c, probe, rows, xyz)
            views.append(v), shades.append(shade)
        return views, shades

    def loss_fn(step):
        probe = current_probe()
        views, shades = step_frames(step, probe) if stepwise else (cache, None)
        if regularisers is None:
            return heads_loss(eng, views, theta, probe, shades=shades)
        noises = [noise_fn(step, i, c.cpts.shape[0]).to(dev, torch.float32) for i, c in enumerate(views)]
        total, t = regularised_loss(eng, views, theta, probe, weights, noises, shades=shades)
        terms.append(t)
        return total

    try:
        for step in range(steps):
            opt.zero_grad(set_to_none=True)
            loss = loss_fn(step)
            loss.backward()
            opt.step()
            history.append(loss.detach())
        with torch.no_grad():
            history.append(loss_fn(steps))
            probe = current_probe().detach().contiguous()
    finally:
        if noisy:
            eng.set_light_xyz(None)
    sd = eng.heads_state_dict(theta)
    if fit_probe:
        sd['global_env_map_'] = p_param.detach().cpu().clone()
    out = dotdict(state_dict=sd, theta=theta.detach(), probe=probe, loss=[float(x) for x in torch.stack(history).cpu()])
    if regularisers is not None:
        out.terms = dotdict({k: [float(x) for x in torch.stack([t[k] for t in terms]).cpu()] for k in ('img_loss',) + TERMS})
    return out

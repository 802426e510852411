"""Engine: thin Python owner of one ra_ctx (the C ABI context).

PyTorch is plumbing here: it owns device memory (torch tensors whose data_ptr() is handed to the
library) and the stream.  All arithmetic of the render path happens in the HIP library.
"""
import contextlib
import ctypes as C

import torch

from . import _lib
from ._lib import (check, ra_config, ra_counters, ra_frame, ra_ground_out, ra_ground_params, ra_lpips_weights, ra_metrics_params, ra_pose_in, ra_pose_out,
                   ra_render_out, ra_sphere_params, ra_trace_params)
from . import lpips_weights
from .base_utils import dotdict
from .handles import Cloth, Mesh, Topology, _f32, _i32, _ptr, check_closest_backward_args      # the classes: also this module's public names


def _bbox6(bbox6):
    return (C.c_float * 6)(*[float(v) for v in bbox6])


def _probe_hw(probe):
    """(h, w) of an (h,w,3) probe; (0, 0) without one"""
    return (probe.shape[0], probe.shape[1]) if probe is not None else (0, 0)


def _set_box_tables(params, boxes, box_start):
    """the n_boxes / boxes / box_start tables of ra_sphere_params / ra_ground_params (one box: none); returns the arrays params points
    into, which the caller holds until the library call has returned"""
    if boxes is not None and len(boxes) > 1:
        flat = (C.c_float * (6 * len(boxes)))(*[float(v) for b in boxes for v in b])
        starts = (C.c_int * (len(boxes) + 1))(*[int(v) for v in box_start])
        params.n_boxes, params.boxes, params.box_start = len(boxes), C.cast(flat, C.POINTER(C.c_float)), C.cast(starts, C.POINTER(C.c_int))
        return flat, starts
    params.n_boxes, params.boxes, params.box_start = 0, None, None
    return None


class RaysPending:
    """rays generated on the device whose count has not been read yet (Engine.gen_rays_async)"""

    def __init__(self, bufs, host, mask_host, event, H, W, keep):
        self._bufs, self._host, self._mask_host, self._event, self.H, self.W, self._keep = bufs, host, mask_host, event, H, W, keep

    def ready(self):
        return self._event.query()

    def result(self):
        """ray_o, ray_d (P,3), near, far (P,), mask_at_box (H,W) bool on the device; wbounds_host (1,2,3) and — if requested —
        mask_host (H*W,) bool on the host.  Waits for the generating kernels only (an event), not for the stream."""
        self._event.synchronize()
        P = int(self._host[:1].view(torch.int32).item())
        ro, rd, near, far, mask = self._bufs
        # the buffers were allocated on the issuing stream; whoever consumes them on another stream must keep the caching allocator
        # from recycling the blocks under it (advisor, round 4)
        cur = torch.cuda.current_stream(ro.device)
        for b in self._bufs:
            b.record_stream(cur)
        out = dotdict(ray_o=ro[:P], ray_d=rd[:P], near=near[:P], far=far[:P], mask_at_box=mask.view(self.H, self.W).bool(),
                      wbounds_host=self._host[1:7].clone().reshape(1, 2, 3))
        if self._mask_host is not None:
            out.mask_host = self._mask_host.bool()
        return out


class Engine:
    def __init__(self, cfg, device=None, relight=False):
        if not torch.cuda.is_available():
            raise _lib.RaError('relightableavatar_amd needs a HIP device (MI355X); there is no CPU fallback for the render path')
        self.lib = _lib.lib()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.cfg = cfg
        self.ctx = C.c_void_p()
        check(self.lib.ra_ctx_create(C.byref(self.ctx), self.device.index or 0), 'ra_ctx_create')
        self.relight = bool(relight)      # RelightableAvatar heads (17-ch raw) vs AniSDF colour net (16-ch raw)
        c = ra_config(xyz_res=cfg.xyz_res, sdf_res=cfg.sdf_res, view_res=cfg.view_res, n_bones=cfg.n_bones, relight=int(self.relight),
                      resd_limit=cfg.resd_limit, blend_radius=cfg.blend_radius, albedo_slope=cfg.albedo_slope,
                      albedo_bias=cfg.albedo_bias, roughness_slope=cfg.roughness_slope, roughness_bias=cfg.roughness_bias,
                      fresnel_f0=cfg.fresnel_f0, shading_albedo=cfg.shading_albedo, albedo_multiplier=cfg.albedo_multiplier,
                      lambert_only=int(cfg.lambert_only), glossy_only=int(cfg.glossy_only),
                      tonemapping=int(cfg.tonemapping_rendering), bg_brightness=cfg.bg_brightness,
                      mlp_f16=int(cfg.mlp_dtype == 'f16'), query_skip=int(cfg.get('query_skip', True)),
                      k4_batch_slots=int(cfg.get('k4_batch_slots', 0)), trace_precision=int(cfg.get('trace_precision', 1)),
                      clip_near=float(cfg.get('clip_near', 0.02)), clip_far=float(cfg.get('clip_far', 10.0)),
                      only_visibility=int(bool(cfg.get('only_visibility', False))),
                      vis_shade_map=2 if cfg.get('vis_ldot_map', False) else (1 if cfg.get('vis_lvis_map', False) else 0),
                      use_geodesic_filter=int(bool(cfg.get('use_geodesic_filter', True))),
                      key_light_share=float(cfg.get('key_light_share', 0.0078)))
        assert cfg.mlp_dtype in ('f16', 'bf16')
        check(self.lib.ra_set_config(self.ctx, C.byref(c)), 'ra_set_config')
        self._frame_key = None
        self._frame_refs = None
        self._keep = []

    def __del__(self):
        try:
            if getattr(self, 'ctx', None) and self.ctx.value:
                self.lib.ra_ctx_destroy(self.ctx)
                self.ctx = C.c_void_p()
        except Exception:
            pass

    # ------------------------------------------------------------------ plumbing
    @property
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def load_state_dict(self, sd: dict):
        """hand every tensor of the reference state_dict to the packer (host fp32)."""
        for k, v in sd.items():
            if not isinstance(v, torch.Tensor) or not v.dtype.is_floating_point:
                continue
            h = v.detach().to('cpu', torch.float32).contiguous()
            check(self.lib.ra_set_weight(self.ctx, k.encode(), C.c_void_p(h.data_ptr()), h.numel()), f'ra_set_weight({k})')
        check(self.lib.ra_finalize_weights(self.ctx, self.stream), 'ra_finalize_weights')
        self._frame_key = None

    FRAME_KEYS = ('R', 'Th', 'poses', 'A', 'big_A', 'pverts', 'pnorm', 'tverts', 'weights')

    def _cond_fix_source(self, batch):
        """the pose the colour net is conditioned on in eval mode (base_network.py:501-503): with
        `cfg.fix_material >= 0 or cfg.always_fix_material` it is train_motion.poses[:, cfg.fix_material] (so -1 selects the last
        training pose) and a batch without train_motion is an error, exactly as in the reference; otherwise the current pose.
        The relight network has no pose-conditioned head (relight_network.py:91-104)."""
        if self.relight:
            return None
        c = self.cfg
        if c.fix_material >= 0 or c.always_fix_material:
            tm = batch.get('train_motion', None) if hasattr(batch, 'get') else None
            if tm is None or 'poses' not in tm:
                raise ValueError('cfg.fix_material / cfg.always_fix_material need batch.train_motion.poses (base_network.py:502-503)')
            return tm['poses']
        return batch['poses']

    def set_frame(self, batch, force=False):
        """upload the SMPL frame state (batch keys of SURVEY.md section 8b).  The upload is skipped only when every tensor of the
        frame is the SAME live object (held by a strong reference, so its address cannot be recycled for another frame) at the
        same in-place version as in the previous call, and the fixed-material index is unchanged."""
        src = [batch[k] for k in self.FRAME_KEYS]
        cf_src = self._cond_fix_source(batch)
        refs = src + [cf_src]
        key = tuple(None if t is None else t._version for t in refs) + (int(self.cfg.fix_material), bool(self.cfg.always_fix_material))
        if (not force and self._frame_key == key and self._frame_refs is not None and len(self._frame_refs) == len(refs)
                and all(a is b for a, b in zip(self._frame_refs, refs))):
            return
        d = self.device
        t = {k: _f32(batch[k][0], d) for k in self.FRAME_KEYS}
        cond_fix = None
        if cf_src is not None:
            cond_fix = t['poses'] if cf_src is batch['poses'] else _f32(cf_src[0, self.cfg.fix_material], d)
        fr = ra_frame(R=_ptr(t['R']), Th=_ptr(t['Th']), poses=_ptr(t['poses']), cond_fix=_ptr(cond_fix), A=_ptr(t['A']),
                      big_A=_ptr(t['big_A']), pverts=_ptr(t['pverts']), pnorm=_ptr(t['pnorm']), tverts=_ptr(t['tverts']),
                      weights=_ptr(t['weights']), n_verts=int(t['pverts'].shape[0]))
        assert t['weights'].shape[-1] == self.cfg.n_bones, 'batch.weights does not match cfg.n_bones'
        check(self.lib.ra_set_frame(self.ctx, C.byref(fr), self.stream), 'ra_set_frame')
        self._keep = [t, cond_fix]   # the library copies asynchronously on the stream
        self._frame_key, self._frame_refs = key, refs

    # ------------------------------------------------------------------ operators
    def hdq_sdf(self, x: torch.Tensor, dist_th: float, smooth: bool) -> torch.Tensor:
        x = _f32(x.reshape(-1, 3), self.device)
        out = torch.empty(x.shape[0], device=self.device, dtype=torch.float32)
        check(self.lib.ra_hdq_sdf(self.ctx, _ptr(x), x.shape[0], dist_th, int(smooth), _ptr(out), self.stream), 'ra_hdq_sdf')
        return out

    def observed_sdf(self, bpts: torch.Tensor) -> torch.Tensor:
        """SDF(bpts + resd(bpts)) on big-pose points through the production distance-query kernel (no coarse level)."""
        bpts = _f32(bpts.reshape(-1, 3), self.device)
        out = torch.empty(bpts.shape[0], device=self.device, dtype=torch.float32)
        check(self.lib.ra_observed_sdf(self.ctx, _ptr(bpts), bpts.shape[0], _ptr(out), self.stream), 'ra_observed_sdf')
        return out

    def bigpose_transform(self, x: torch.Tensor, R: torch.Tensor, Th: torch.Tensor, invert=False) -> torch.Tensor:
        """(n,4,4) world -> big-pose transforms (or their affine inverses) of the points x against the current frame."""
        x = _f32(x.reshape(-1, 3), self.device)
        R, Th = _f32(R.reshape(3, 3), self.device), _f32(Th.reshape(3), self.device)
        out = torch.empty(x.shape[0], 4, 4, device=self.device, dtype=torch.float32)
        check(self.lib.ra_bigpose_transform(self.ctx, _ptr(x), x.shape[0], _ptr(R), _ptr(Th), int(invert), _ptr(out), self.stream),
              'ra_bigpose_transform')
        return out

    def forward(self, x: torch.Tensor, v, dist_th: float) -> torch.Tensor:
        x = _f32(x.reshape(-1, 3), self.device)
        v = None if v is None else _f32(v.reshape(-1, 3), self.device)
        C_ = self.lib.ra_raw_channels(self.ctx)
        raw = torch.empty(x.shape[0], C_, device=self.device, dtype=torch.float32)
        check(self.lib.ra_forward(self.ctx, _ptr(x), _ptr(v), x.shape[0], dist_th, _ptr(raw), self.stream), 'ra_forward')
        return raw

    def trace_params(self, tc, dist_th, soft, iters=None) -> ra_trace_params:
        st = self.cfg.sphere_tracing
        return ra_trace_params(iters=int(tc.iter if iters is None else iters), tan_i=st.tan_i, tan_i_multiplier=st.tan_i_multiplier,
                               relax=tc.relax, offset=tc.offset, eps=st.eps, shadow_skip_iter=st.shadow_skip_iter,
                               clay_book=int(not self.cfg.no_claybook), soft_shadow=int(soft), dist_th=dist_th)

    def sphere_trace(self, ray_o, ray_d, near, far, params: ra_trace_params, tan_i=None):
        d = self.device
        ray_o, ray_d = _f32(ray_o.reshape(-1, 3), d), _f32(ray_d.reshape(-1, 3), d)
        near, far = _f32(near.reshape(-1), d), _f32(far.reshape(-1), d)
        tan_i = None if tan_i is None else _f32(tan_i.reshape(-1), d)
        n = ray_o.shape[0]
        surf = torch.empty(n, 3, device=d)
        occ, st, ot = (torch.empty(n, device=d) for _ in range(3))
        check(self.lib.ra_sphere_trace(self.ctx, _ptr(ray_o), _ptr(ray_d), _ptr(near), _ptr(far), _ptr(tan_i), n, C.byref(params),
                                       _ptr(surf), _ptr(occ), _ptr(st), _ptr(ot), self.stream), 'ra_sphere_trace')
        return surf, occ, st, ot

    def sphere_params(self) -> ra_sphere_params:
        c = self.cfg
        return ra_sphere_params(surface=self.trace_params(c.sphere_tracing, c.dist_th, False),
                                shadow=self.trace_params(c.obj_lvis, c.obj_lvis.dist_th, not c.no_dfss),
                                shadow_near_offset=c.obj_lvis.near_offset, dist_th=c.dist_th,
                                surf_sample_range=c.surf_sample_range, n_samples=c.n_samples, relighting=int(c.relighting),
                                no_visibility=int(c.no_visibility), local_visibility=int(c.local_visibility), premultiply=1)

    def render_sphere_chunk(self, ray_o, ray_d, near, far, bbox6, probe, params, outs: dict, boxes=None, box_start=None):
        """ray tensors: contiguous fp32 device views (P,3)/(P,); outs: name -> tensor view or missing.
        boxes / box_start: several of the reference's chunks in this one call, the shadow rays of ray r clipped against the box of its own chunk."""
        P = ray_o.shape[0]
        ro = ra_render_out(**{k: _ptr(outs.get(k)) for k in _lib.RENDER_OUT_KEYS})
        bb = _bbox6(bbox6) if bbox6 is not None else None
        ph, pw = _probe_hw(probe)
        tables = _set_box_tables(params, boxes, box_start)      # alive across the call below
        check(self.lib.ra_render_sphere_chunk(self.ctx, _ptr(ray_o), _ptr(ray_d), _ptr(near), _ptr(far), P, bb, _ptr(probe), ph, pw,
                                              C.byref(params), C.byref(ro), self.stream), 'ra_render_sphere_chunk')

    def ground_params(self) -> ra_ground_params:
        c = self.cfg
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
        return ra_ground_params(normal=f3(c.ground_normal), origin=f3(c.ground_origin), albedo=f3(c.ground_albedo),
                                attach_envmap=int(c.ground_attach_envmap), env_r=float(c.env_r),
                                shading_multiplier=float(c.ground_shading_multiplier),
                                shadow=self.trace_params(c.env_lvis, c.env_lvis.dist_th, not c.no_dfss),
                                shadow_near_offset=c.env_lvis.near_offset, no_visibility=int(c.no_visibility),
                                local_visibility=int(c.local_visibility))

    def render_ground_chunk(self, ray_o, ray_d, acc, bbox6, probe, params, outs: dict, boxes=None, box_start=None):
        """N1: one chunk of full-frame rays against the ground plane (render_ground); outs: name -> (P,3)/(P,) views.
        boxes / box_start: several of the reference's chunks in this one call, pixel r clipped against the box of its own chunk."""
        P = ray_o.shape[0]
        go = ra_ground_out(**{k: _ptr(outs.get(k)) for k in _lib.GROUND_OUT_KEYS})
        bb = _bbox6(bbox6)
        tables = _set_box_tables(params, boxes, box_start)      # alive across the call below
        check(self.lib.ra_render_ground_chunk(self.ctx, _ptr(ray_o), _ptr(ray_d), _ptr(acc), P, bb, _ptr(probe), probe.shape[0],
                                              probe.shape[1], C.byref(params), C.byref(go), self.stream), 'ra_render_ground_chunk')

    def debug_key_lights(self, n_lights):
        """(bool mask, share) of the frame's key lights (test hook)"""
        key = torch.empty(n_lights, dtype=torch.uint8, device=self.device)
        share = torch.empty(n_lights, dtype=torch.float32, device=self.device)
        check(self.lib.ra_debug_key_lights(self.ctx, _ptr(key), _ptr(share), self.stream), 'ra_debug_key_lights')
        return key.bool(), share

    def begin_render(self):
        """one top-level render starts: its chunk calls are numbered from here (launch-variant hints; ra_begin_render)"""
        check(self.lib.ra_begin_render(self.ctx), 'ra_begin_render')

    def k3cc_enabled(self) -> bool:
        """the cooperative small-launch distance kernel passed its on-device self-test and is in use (ra_k3cc_enabled)"""
        return bool(self.lib.ra_k3cc_enabled(self.ctx))

    def set_key_probes(self, probe_sets):
        """name the frame's key lights (ra_config.key_light_share) from every probe its cached visibility will be shaded with:
        probe_sets is a list of (n, h, w, 3) / (h, w, 3) tensors (one entry per probe size); an empty list returns to per-call key lights."""
        if not probe_sets:
            check(self.lib.ra_set_key_probes(self.ctx, None, 0, 0, 0, 0, self.stream), 'ra_set_key_probes')
            return
        for i, pr in enumerate(probe_sets):
            pr = _f32(pr if pr.ndim == 4 else pr[None], self.device)
            self._keep.append(pr)
            check(self.lib.ra_set_key_probes(self.ctx, _ptr(pr), pr.shape[0], pr.shape[1], pr.shape[2], int(i > 0), self.stream), 'ra_set_key_probes')

    # ------------------------------------------------------------------ moved lights, re-traced visibility
    def set_light_xyz(self, xyz):
        """move the context's lights (ra_set_light_xyz): xyz (L,3) or anything that reshapes to it — e.g. light_xyz_ plus the trainer's
        noise (relight_network.py:79-84); None restores the loaded positions.  Every later call of this engine follows the new positions
        (renders, light_visibility, reshade and its backward, the key lights); key lights named by set_key_probes are dropped."""
        if xyz is not None:
            xyz = _f32(xyz.reshape(-1, 3), self.device)
            L = int(self.cfg.env_h * self.cfg.env_w)
            if xyz.shape[0] != L:
                raise ValueError(f'set_light_xyz: {xyz.shape[0]} positions for {L} lights')
        check(self.lib.ra_set_light_xyz(self.ctx, _ptr(xyz), self.stream), 'ra_set_light_xyz')      # copied on the stream: xyz may be freed after the call

    @contextlib.contextmanager
    def light_positions(self, xyz):
        """with eng.light_positions(xyz): ... — the lights at xyz inside the block, the loaded positions after it, also on an exception"""
        self.set_light_xyz(xyz)
        try:
            yield self
        finally:
            self.set_light_xyz(None)

    def light_visibility(self, surf, norm, acc, bbox6, probe=None, rows=None, params=None):
        """light_visibility (sphere_tracing_renderer.py:265-344) on cached surface points of the current frame under the current light
        positions (ra_light_visibility): surf, norm (n,3), acc (n,), bbox6 the shadow rays' box -> (lvis, ldot), each (n, L) — or, with
        rows (distinct indices into the n points, any order; int32 on the device is passed as it is), (len(rows), L), row k belonging to
        point rows[k].  probe (h,w,3): the key lights are derived from it as in a render call; params: sphere_params() by default."""
        dv = self.device
        surf, norm, acc = _f32(surf.reshape(-1, 3), dv), _f32(norm.reshape(-1, 3), dv), _f32(acc.reshape(-1), dv)
        n = surf.shape[0]
        if rows is not None:
            rows = _i32(torch.as_tensor(rows).reshape(-1), dv)
        m = n if rows is None else rows.shape[0]
        L = int(self.cfg.env_h * self.cfg.env_w)
        lvis, ldot = torch.empty(m, L, device=dv), torch.empty(m, L, device=dv)
        if m == 0:      # nothing to trace (an empty tensor has no address to hand over)
            return lvis, ldot
        probe = None if probe is None else _f32(probe[0] if probe.ndim == 4 else probe, dv)
        ph, pw = _probe_hw(probe)
        bb = _bbox6(bbox6)
        p = self.sphere_params() if params is None else params
        check(self.lib.ra_light_visibility(self.ctx, _ptr(surf), _ptr(norm), _ptr(acc), n, _ptr(rows), m if rows is not None else 0, bb, _ptr(probe),
                                           ph, pw, C.byref(p), _ptr(lvis), _ptr(ldot), self.stream), 'ra_light_visibility')
        return lvis, ldot

    def reshade_ground(self, ray_d, albedo_map, lvis, ldot, probes, images=None, attach_envmap=True):
        """novel_light_sphere_tracing.render_ground (:70-99) for all probes at once: probes (n,h,w,3), optional images
        (n,ih,iw,3) -> rgb, albedo, shade, spec each (n,P,3)."""
        d = self.device
        ray_d = _f32(ray_d.reshape(-1, 3), d)
        P = ray_d.shape[0]
        albedo_map = None if albedo_map is None else _f32(albedo_map.reshape(P, 3), d)
        lvis, ldot = _f32(lvis.reshape(P, -1), d), _f32(ldot.reshape(P, -1), d)
        probes = _f32(probes, d)
        n, ph, pw = probes.shape[0], probes.shape[1], probes.shape[2]
        images = None if images is None else _f32(images, d)
        ih, iw = (images.shape[1], images.shape[2]) if images is not None else (0, 0)
        outs = [torch.empty(n, P, 3, device=d) for _ in range(4)]
        check(self.lib.ra_reshade_ground(self.ctx, _ptr(ray_d), _ptr(albedo_map), _ptr(lvis), _ptr(ldot), P, _ptr(probes), n, ph, pw,
                                         _ptr(images), ih, iw, int(bool(attach_envmap)), *[_ptr(o) for o in outs], self.stream),
              'ra_reshade_ground')
        return tuple(outs)

    def blend_ground(self, ground, human, inds, acc):
        """blend_output_'s alpha_blend for one map: ground (F,C)/(F,) or None, human (P,C)/(P,) or None, inds (P) int64, acc (F)."""
        ref = ground if ground is not None else human
        flat = ref.ndim == 1
        C_ = 1 if flat else ref.shape[-1]
        F_ = acc.shape[0]
        g = None if ground is None else _f32(ground, self.device).reshape(F_, C_)
        h = None if human is None else _f32(human, self.device).reshape(-1, C_)
        P = 0 if h is None else h.shape[0]
        dst = torch.empty(F_, C_, device=self.device)
        check(self.lib.ra_blend_ground(self.ctx, _ptr(g), _ptr(h), _ptr(inds), _ptr(acc), F_, P, C_, _ptr(dst), self.stream), 'ra_blend_ground')
        return dst[:, 0] if flat else dst

    def render_volume_chunk(self, ray_o, ray_d, near, far, n_samples, dist_th, outs: dict):
        P = ray_o.shape[0]
        ro = ra_render_out(**{k: _ptr(outs.get(k)) for k in _lib.RENDER_OUT_KEYS})
        check(self.lib.ra_render_volume_chunk(self.ctx, _ptr(ray_o), _ptr(ray_d), _ptr(near), _ptr(far), P, n_samples, dist_th,
                                              C.byref(ro), self.stream), 'ra_render_volume_chunk')

    def _reshade_inputs(self, ray_o, surf, norm, albedo, rough, lvis, ldot, probes):
        """the inputs of reshade / reshade_backward as contiguous fp32 device tensors: [ray_o, surf, norm, albedo, rough], lvis, ldot, probes"""
        d = self.device
        a = [_f32(t, d) for t in (ray_o.reshape(-1, 3), surf.reshape(-1, 3), norm.reshape(-1, 3), albedo.reshape(-1, 3), rough.reshape(-1))]
        P = a[0].shape[0]
        return a, _f32(lvis.reshape(P, -1), d), _f32(ldot.reshape(P, -1), d), _f32(probes, d)

    def reshade(self, ray_o, surf, norm, albedo, rough, lvis, ldot, probes, want_spec=True):
        """probes (n,h,w,3) -> rgb, shade, spec each (n,P,3)."""
        d = self.device
        a, lvis, ldot, probes = self._reshade_inputs(ray_o, surf, norm, albedo, rough, lvis, ldot, probes)
        P = a[0].shape[0]
        n, ph, pw = probes.shape[0], probes.shape[1], probes.shape[2]
        rgb, shade = torch.empty(n, P, 3, device=d), torch.empty(n, P, 3, device=d)
        spec = torch.empty(n, P, 3, device=d) if want_spec else None
        check(self.lib.ra_reshade(self.ctx, *[_ptr(t) for t in a], _ptr(lvis), _ptr(ldot), P, _ptr(probes), n, ph, pw,
                                  _ptr(rgb), _ptr(shade), _ptr(spec), self.stream), 'ra_reshade')
        return rgb, shade, spec

    def reshade_backward(self, ray_o, surf, norm, albedo, rough, lvis, ldot, probes, d_rgb, want=(True, True, True)):
        """backward of reshade's rgb: d_rgb (n,P,3) -> d_albedo (P,3), d_rough (P,), d_probes (n,h,w,3); want: which of the three
        to compute (the others are None)."""
        d = self.device
        a, lvis, ldot, probes = self._reshade_inputs(ray_o, surf, norm, albedo, rough, lvis, ldot, probes)
        P = a[0].shape[0]
        n, ph, pw = probes.shape[0], probes.shape[1], probes.shape[2]
        d_rgb = _f32(d_rgb.reshape(n, P, 3), d)
        # zeros, not empty: a call with P == 0 or n == 0 writes nothing, and the gradient of an empty sum is 0
        d_alb = torch.zeros(P, 3, device=d) if want[0] else None
        d_rgh = torch.zeros(P, device=d) if want[1] else None
        d_prb = torch.zeros(n, ph, pw, 3, device=d) if want[2] else None
        check(self.lib.ra_reshade_backward(self.ctx, *[_ptr(t) for t in a], _ptr(lvis), _ptr(ldot), P, _ptr(probes), n, ph, pw,
                                           _ptr(d_rgb), _ptr(d_alb), _ptr(d_rgh), _ptr(d_prb), self.stream), 'ra_reshade_backward')
        return d_alb, d_rgh, d_prb

    # ------------------------------------------------------------------ material heads on cached features (ra_heads.hip)
    HEADS_KEYS = tuple(f'{net}.linears.{l}.{kind}' for net in ('albedo_network', 'roughness_network') for l in range(3) for kind in ('weight', 'bias'))

    def _heads_check(self):
        w, dp = int(self.cfg.get('relight_network_width', 128)), int(self.cfg.get('relight_network_depth', 2))
        if (w, dp) != (128, 2):
            raise _lib.RaError(f'the material-head kernels are compiled for relight_network_width 128 and relight_network_depth 2, not {w} / {dp}')

    def heads_param_count(self) -> int:
        return int(self.lib.ra_heads_param_count(self.ctx))

    def heads_params(self) -> torch.Tensor:
        """the two material heads as loaded (load_state_dict) in the flat layout of include/relightableavatar.h: HEADS_KEYS in order"""
        self._heads_check()
        theta = torch.empty(self.heads_param_count(), device=self.device)
        check(self.lib.ra_heads_get_params(self.ctx, _ptr(theta), self.stream), 'ra_heads_get_params')
        return theta

    def heads_state_dict(self, theta) -> dict:
        """theta split into the twelve state_dict keys (views of a host copy)"""
        shapes = [(128, 256), (128,), (128, 128), (128,), (3, 128), (3,), (128, 256), (128,), (128, 128), (128,), (1, 128), (1,)]
        t = theta.detach().to('cpu', torch.float32).reshape(-1)
        assert t.numel() == sum(int(torch.Size(sh).numel()) for sh in shapes)
        out, o = {}, 0
        for k, sh in zip(self.HEADS_KEYS, shapes):
            n = int(torch.Size(sh).numel())
            out[k] = t[o:o + n].reshape(sh).clone()
            o += n
        return out

    def heads_forward(self, theta, feat):
        """theta (99332,), feat (n,256) -> albedo (n,3), roughness (n,)"""
        self._heads_check()
        d = self.device
        theta, feat = _f32(theta.reshape(-1), d), _f32(feat.reshape(-1, 256), d)
        assert theta.numel() == self.heads_param_count()
        n = feat.shape[0]
        albedo, rough = torch.empty(n, 3, device=d), torch.empty(n, device=d)
        check(self.lib.ra_heads_forward(self.ctx, _ptr(theta), _ptr(feat), n, _ptr(albedo), _ptr(rough), self.stream), 'ra_heads_forward')
        return albedo, rough

    def heads_backward(self, theta, feat, d_albedo, d_rough):
        """d_albedo (n,3) / d_rough (n,) (either may be None: that head's slice is zero) -> d_theta (99332,)"""
        self._heads_check()
        d = self.device
        theta, feat = _f32(theta.reshape(-1), d), _f32(feat.reshape(-1, 256), d)
        assert theta.numel() == self.heads_param_count()
        n = feat.shape[0]
        d_albedo = None if d_albedo is None else _f32(d_albedo.reshape(n, 3), d)
        d_rough = None if d_rough is None else _f32(d_rough.reshape(n), d)
        d_theta = torch.zeros_like(theta)      # zeros, not empty: a call with n == 0 writes nothing, and the gradient of an empty sum is 0
        check(self.lib.ra_heads_backward(self.ctx, _ptr(theta), _ptr(feat), n, _ptr(d_albedo), _ptr(d_rough), _ptr(d_theta), self.stream),
              'ra_heads_backward')
        return d_theta

    def bigpose_features(self, bpts):
        """big-pose points (n,3) of the current frame (raw[:, 3:6]) -> the 256 features the heads see inside the renderer (f16 values)"""
        d = self.device
        bpts = _f32(bpts.reshape(-1, 3), d)
        n = bpts.shape[0]
        feat = torch.empty(n, 256, device=d)
        check(self.lib.ra_bigpose_features(self.ctx, _ptr(bpts), n, _ptr(feat), self.stream), 'ra_bigpose_features')
        return feat

    def canonical_features(self, cpts, out=None):
        """canonical points (n,3) (raw[:, 0:3], plus noise for the jitter regularisers) -> the 256 features of the SDF network in the
        format of bigpose_features; needs no frame.  out: a contiguous (n,256) fp32 device tensor to fill — e.g. the second half of a
        (2n,256) buffer whose first half holds cached features"""
        d = self.device
        cpts = _f32(cpts.reshape(-1, 3), d)
        n = cpts.shape[0]
        if out is None:
            out = torch.empty(n, 256, device=d)
        elif not (out.is_contiguous() and out.dtype == torch.float32 and out.device == d and tuple(out.shape) == (n, 256)):
            raise ValueError('canonical_features: out must be a contiguous fp32 (n, 256) tensor on the engine\'s device')
        check(self.lib.ra_canonical_features(self.ctx, _ptr(cpts), n, _ptr(out), self.stream), 'ra_canonical_features')
        return out

    def gaussian_entropy(self, x, d_value=None, want_grad=True):
        """x (n,3) -> (value: 0-dim tensor, d_x (n,3) or None): gaussian_entropy of the reference (loss_utils.py:51-76; 15 bins on [0, 1])
        and its gradient times d_value (a one-element device tensor; None: 1)"""
        d = self.device
        x = _f32(x.reshape(-1, 3), d)
        n = x.shape[0]
        d_value = None if d_value is None else _f32(d_value.reshape(1), d)
        value = torch.empty((), device=d)
        d_x = torch.empty(n, 3, device=d) if want_grad else None
        check(self.lib.ra_gaussian_entropy(self.ctx, _ptr(x), n, _ptr(d_value), _ptr(value), _ptr(d_x), self.stream), 'ra_gaussian_entropy')
        return value, d_x

    def _image_pair(self, who, pred, gt, H, W, pix, mask, out, n_out):
        """the image pair of image_metrics / lpips on the device, checked: pred, gt, pix, mask, out (allocated with n_out doubles if None)"""
        d = self.device
        pred, gt = _f32(pred.reshape(-1, 3), d), _f32(gt.reshape(-1, 3), d)
        P = pred.shape[0]
        if gt.shape[0] != P:
            raise ValueError(f'{who}: pred and gt differ in size')
        if pix is not None:
            pix = pix.detach().to(device=d, dtype=torch.int64).reshape(-1).contiguous()
            if pix.numel() != P:
                raise ValueError(f'{who}: one pixel index per ray')
        if mask is not None:
            mask = mask.detach().to(device=d).reshape(-1).ne(0).to(torch.uint8).contiguous()
            if mask.numel() != H * W:
                raise ValueError(f'{who}: the mask must have H*W entries')
        if out is None:
            out = torch.empty(n_out, dtype=torch.float64, device=d)
        elif not (out.is_contiguous() and out.dtype == torch.float64 and out.device == d and tuple(out.shape) == (n_out,)):
            raise ValueError(f'{who}: out must be a contiguous float64 ({n_out},) tensor on the engine\'s device')
        return pred, gt, pix, mask, out

    def image_metrics(self, pred, gt, H, W, pix=None, mask=None, bg=0.0, mse_over_rays=False, out=None, data_range=1.0):
        """pred, gt (P,3): all H*W pixels, or a ray list with pix (P,) int64 = the flat pixel of every ray (pixels without a ray hold bg
        in both images) -> float64 device tensor [mse, psnr, ssim, windows] of the reference's evaluator (base_evaluator.py:71-104;
        include/relightableavatar.h: ra_image_metrics).  mask (H*W, nonzero = inside): the SSIM is taken on the mask's bounding rectangle
        (eval_whole_img = False).  out: a contiguous float64 (4,) device tensor to fill, e.g. a row of an (N,4) table.  Nothing is read
        back and nothing synchronises."""
        pred, gt, pix, mask, out = self._image_pair('image_metrics', pred, gt, H, W, pix, mask, out, 4)
        P = pred.shape[0]
        p = ra_metrics_params(H=int(H), W=int(W), bg_brightness=float(bg), data_range=float(data_range), mse_over_rays=int(bool(mse_over_rays)),
                              crop_to_mask=int(mask is not None))
        check(self.lib.ra_image_metrics(self.ctx, C.byref(p), _ptr(pred), _ptr(gt), _ptr(pix), P, _ptr(mask), _ptr(out), self.stream), 'ra_image_metrics')
        return out

    def lpips_load(self, state_dict):
        """load an LPIPS (AlexNet) weight set: `lpips.LPIPS().state_dict()`, torchvision's alexnet keys plus the lin* keys, or the neutral
        conv{k}.weight / conv{k}.bias / lin{k}.weight layout (lpips_weights.py holds the table; a missing key or a wrong shape raises and
        lists the expected names and shapes).  A second call replaces the set."""
        w = lpips_weights.resolve(state_dict)
        c = ra_lpips_weights()
        for k in range(lpips_weights.TAPS):
            c.conv_w[k] = w[f'conv{k}.weight'].ctypes.data
            c.conv_b[k] = w[f'conv{k}.bias'].ctypes.data
            c.lin[k] = w[f'lin{k}.weight'].ctypes.data
        for ch in range(3):
            c.shift[ch], c.scale[ch] = float(w['shift'][ch]), float(w['scale'][ch])
        check(self.lib.ra_lpips_load(self.ctx, C.byref(c), self.stream), 'ra_lpips_load')

    def lpips_loaded(self):
        return bool(self.lib.ra_lpips_loaded(self.ctx))

    def lpips(self, pred, gt, H, W, pix=None, mask=None, bg=0.0, out=None):
        """pred, gt, pix, mask, bg as in image_metrics -> float64 device tensor [lpips, r_0 .. r_4]: lpips.LPIPS() (AlexNet, 0.1) on the
        two assembled images in [0, 1] as the reference's evaluator calls it (base_evaluator.py:50-69), and its five per-tap terms.
        mask: the images are first cropped to its bounding rectangle.  Below 31 in a dimension: six NaNs.  out: a contiguous float64
        (6,) device tensor to fill.  Nothing is read back and nothing synchronises.  Needs lpips_load()."""
        pred, gt, pix, mask, out = self._image_pair('lpips', pred, gt, H, W, pix, mask, out, 6)
        P = pred.shape[0]
        p = ra_metrics_params(H=int(H), W=int(W), bg_brightness=float(bg), data_range=1.0, mse_over_rays=0, crop_to_mask=int(mask is not None))
        check(self.lib.ra_lpips(self.ctx, C.byref(p), _ptr(pred), _ptr(gt), _ptr(pix), P, _ptr(mask), _ptr(out), self.stream), 'ra_lpips')
        return out

    def lpips_features(self, img, tap):
        """img (H,W,3) in [0, 1] -> the post-ReLU activations of tap 0..4 as a (C,h,w) fp32 device tensor (stage hook of the parity tests)"""
        d = self.device
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError('lpips_features: img must be (H, W, 3)')
        H, W = int(img.shape[0]), int(img.shape[1])
        if min(H, W) < 31 or not 0 <= int(tap) < lpips_weights.TAPS:
            raise ValueError('lpips_features: an image below 31 x 31 has no features; tap 0..4')
        img = _f32(img, d)
        side = lambda n: (n - 7) // 4 + 1
        pool = lambda n: (n - 3) // 2 + 1
        h, w = side(H), side(W)
        for _ in range(min(int(tap), 2)):
            h, w = pool(h), pool(w)
        out = torch.empty(lpips_weights.CONV_SHAPES[int(tap)][0], h, w, device=d)
        check(self.lib.ra_lpips_features(self.ctx, _ptr(img), H, W, int(tap), _ptr(out), self.stream), 'ra_lpips_features')
        return out

    def mesh(self, verts, faces, faces_dev=None):
        """verts (V,3) float, faces (F,3) integer -> a Mesh handle for closest-point queries (include/relightableavatar.h: ra_mesh_create).
        The vertices go to the device as they are (a device tensor makes no round trip); the faces are checked on the host against
        [0, V) before anything is launched, so faces on the device cost a read-back (and its wait) here: pass host faces where there
        is a choice.  Otherwise asynchronous; the handle owns nothing of the caller's.  The Mesh keeps the int32 faces and V for
        Mesh.closest_backward, which reads the faces on the device: they are uploaded at the first backward, or never when faces_dev,
        the same (F,3) int32 faces already on the engine's device, is given (a loop that rebuilds its mesh per step)."""
        verts = _f32(verts.reshape(-1, 3), self.device)
        given = faces
        faces = faces.detach().to('cpu', torch.int32).reshape(-1, 3).contiguous()
        if faces_dev is not None and (not torch.is_tensor(faces_dev) or faces_dev.dtype != torch.int32 or tuple(faces_dev.shape) != tuple(faces.shape)
                                      or faces_dev.device != torch.device(self.device) or not faces_dev.is_contiguous()):
            raise ValueError(f'Engine.mesh: faces_dev must be the contiguous int32 faces {tuple(faces.shape)} on {self.device}')
        handle = C.c_void_p()
        check(self.lib.ra_mesh_create(self.ctx, _ptr(verts), verts.shape[0], C.c_void_p(faces.data_ptr()), faces.shape[0], C.byref(handle), self.stream),
              'ra_mesh_create')
        if faces_dev is None:
            # the int32 host faces stay with the Mesh for its backward; a copy only where they are still the caller's own memory
            keep = faces.clone() if faces.data_ptr() == given.data_ptr() else faces
        else:
            keep = faces_dev
        return Mesh(self, handle, faces.shape[0], keep, verts.shape[0])

    check_closest_backward_args = staticmethod(check_closest_backward_args)     # Mesh.closest_backward calls it before any engine exists

    def mesh_closest_backward(self, faces, n_verts, points, out, g_d2=None, g_attr=None, want=Mesh.GRAD_WANT):
        """Mesh.closest_backward without a Mesh (ra_mesh_closest_backward needs none): faces (F,3) integer, n_verts, and the rest as
        there.  Faces that are int32 on the device go in as they are."""
        want, n, Cn = self.check_closest_backward_args(points, out, g_d2, g_attr, want)
        d = self.device
        faces = _i32(faces.reshape(-1, 3), d)
        if faces.shape[0] < 1 or int(n_verts) < 1:
            raise ValueError('closest_backward: needs at least one face and one vertex')
        pts = _f32(points.reshape(-1, 3), d)
        q, bary = _f32(out['closest'], d), _f32(out['bary'], d)
        face = _i32(out['face'], d)
        g = None if g_d2 is None else _f32(g_d2.reshape(-1), d)
        ga = None if g_attr is None else _f32(g_attr, d)
        res = dotdict()
        for k in want:
            res[k] = torch.empty((n, 3) if k == 'dpts' else (int(n_verts), 3 if k == 'dverts' else Cn), dtype=torch.float32, device=d)
        row = lambda t: _ptr(t) if t is not None and n else None
        outs = (row(res.get('dpts')), _ptr(res.get('dverts')), _ptr(res.get('dattr')) if Cn else None)
        if any(o is not None for o in outs):       # else: only empty arrays were asked for
            check(self.lib.ra_mesh_closest_backward(self.ctx, _ptr(faces), faces.shape[0], int(n_verts), row(pts), row(q), row(face), row(bary), n,
                                                    row(g), row(ga) if Cn else None, Cn, *outs, self.stream), 'ra_mesh_closest_backward')
        return res

    def topology(self, faces, n_verts):
        """faces (F,3) integer, n_verts -> a Topology handle (include/relightableavatar.h: ra_topo_create).  Faces on the device make
        no round trip (Engine.marching_cubes' int32 faces go in as they are) and are checked there against [0, n_verts).  One
        blocking read-back."""
        f = _i32(faces.reshape(-1, 3), self.device)
        handle = C.c_void_p()
        check(self.lib.ra_topo_create(self.ctx, _ptr(f) if f.shape[0] else None, f.shape[0], int(n_verts), C.byref(handle), self.stream), 'ra_topo_create')
        return Topology(self, handle)

    @staticmethod
    def _raster_maps(who, raster, device):
        uv, face = _f32(raster.uv, device), _i32(raster.face, device)
        if uv.ndim != 4 or uv.shape[3] != 2 or face.shape != uv.shape[:3]:
            raise ValueError(f'{who}: raster.uv must be (B, H, W, 2) and raster.face (B, H, W)')
        return uv, face

    def rasterize(self, pos_clip, faces, H, W, brute=False):
        """pos_clip (B,V,4) or (V,4) clip-space (x, y, z, w), faces (F,3) integer shared by the views -> dotdict on the device
        (include/relightableavatar.h: ra_rasterize): uv (B,H,W,2) float32 the barycentrics of corners 0 and 1, zw (B,H,W) float32,
        face (B,H,W) int32, -1 where the pixel is empty (uv and zw hold 0 there).  Pixel (ix, iy) is sampled at NDC
        ((2 ix + 1) / W - 1, (2 iy + 1) / H - 1), row 0 at y = -1.  brute: scan every face per pixel without binning (the same bits,
        slower).  One 8-byte read-back per call (the pair count of the binning and the verdict on the face indices)."""
        pos = _f32(pos_clip, self.device)
        pos = pos[None] if pos.ndim == 2 else pos
        if pos.ndim != 3 or pos.shape[2] != 4:
            raise ValueError('Engine.rasterize: pos_clip must be (B, V, 4) or (V, 4)')
        f = _i32(faces.reshape(-1, 3), self.device)
        B, V, H, W = pos.shape[0], pos.shape[1], int(H), int(W)
        shape = (max(B, 0), max(H, 0), max(W, 0))
        out = dotdict(uv=torch.empty(*shape, 2, dtype=torch.float32, device=self.device), zw=torch.empty(shape, dtype=torch.float32, device=self.device),
                      face=torch.empty(shape, dtype=torch.int32, device=self.device))
        check(self.lib.ra_rasterize(self.ctx, _ptr(pos) if pos.numel() else None, B, V, _ptr(f) if f.numel() else None, f.shape[0], H, W,
                                    _lib.RA_RASTER_BRUTE if brute else 0, _ptr(out.uv), _ptr(out.zw), _ptr(out.face), self.stream), 'ra_rasterize')
        return out

    def interpolate(self, attrs, raster, faces):
        """attrs (V,A) shared by the views or (B,V,A), 1 <= A <= 64; raster: Engine.rasterize's dotdict (uv, face) -> (B,H,W,A) float32
        on the device, 0 where a pixel is empty (ra_interpolate).  Nothing is read back."""
        d = self.device
        a = _f32(attrs, d)
        uv, face = self._raster_maps('Engine.interpolate', raster, d)
        B, H, W = face.shape
        if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[0] != B):
            raise ValueError(f'Engine.interpolate: attrs must be (V, A) or ({B}, V, A)')
        f = _i32(faces.reshape(-1, 3), d)
        V, A = a.shape[-2], a.shape[-1]
        out = torch.empty(B, H, W, max(A, 0), dtype=torch.float32, device=d)
        check(self.lib.ra_interpolate(self.ctx, _ptr(a) if a.numel() else None, int(a.ndim == 3), V, A, _ptr(f) if f.numel() else None, f.shape[0], _ptr(uv),
                                      _ptr(face), B, H, W, _ptr(out), self.stream), 'ra_interpolate')
        return out

    def interpolate_backward(self, topology, attrs, raster, dout, want=('dattr', 'duv')):
        """the gradient of Engine.interpolate: dout (B,H,W,A) -> dotdict(dattr shaped like attrs — summed over the views when they are
        shared —, duv (B,H,W,2)) on the device (ra_interpolate_backward).  topology: Engine.topology of the same faces.  No float
        atomics: the same bits every time.  Nothing is read back."""
        d = self.device
        a, g = _f32(attrs, d), _f32(dout, d)
        uv, face = self._raster_maps('Engine.interpolate_backward', raster, d)
        B, H, W = face.shape
        if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[0] != B) or g.shape != (B, H, W, a.shape[-1]):
            raise ValueError(f'Engine.interpolate_backward: attrs must be (V, A) or ({B}, V, A) and dout ({B}, {H}, {W}, A)')
        out = dotdict()
        if 'dattr' in want:
            out.dattr = torch.empty_like(a)
        if 'duv' in want:
            out.duv = torch.empty_like(uv)
        check(self.lib.ra_interpolate_backward(self.ctx, topology._handle, _ptr(a) if a.numel() else None, int(a.ndim == 3), a.shape[-2], a.shape[-1], _ptr(uv),
                                               _ptr(face), B, H, W, _ptr(g), _ptr(out.get('dattr')) if a.numel() else None, _ptr(out.get('duv')), self.stream),
              'ra_interpolate_backward')
        return out

    def rasterize_backward(self, topology, pos_clip, raster, duv):
        """the gradient of Engine.rasterize's uv in the clip-space positions, the face map held fixed: duv (B,H,W,2) -> (B,V,4) float32
        (ra_rasterize_backward; the z component is 0).  Row b depends on view b alone; the same bits every time.  Nothing is read back."""
        d = self.device
        pos = _f32(pos_clip, d)
        pos = pos[None] if pos.ndim == 2 else pos
        uv, face = self._raster_maps('Engine.rasterize_backward', raster, d)
        g = _f32(duv, d)
        B, H, W = face.shape
        if pos.ndim != 3 or pos.shape[0] != B or pos.shape[2] != 4 or g.shape != uv.shape:
            raise ValueError(f'Engine.rasterize_backward: pos_clip must be ({B}, V, 4) and duv ({B}, {H}, {W}, 2)')
        out = torch.empty_like(pos)
        check(self.lib.ra_rasterize_backward(self.ctx, topology._handle, _ptr(pos) if pos.numel() else None, B, pos.shape[1], H, W, _ptr(uv), _ptr(face), _ptr(g),
                                             _ptr(out) if out.numel() else None, self.stream), 'ra_rasterize_backward')
        return out

    def _antialias_args(self, who, color, raster, pos_clip):
        d = self.device
        col, pos = _f32(color, d), _f32(pos_clip, d)
        pos = pos[None] if pos.ndim == 2 else pos
        zw, face = _f32(raster.zw, d), _i32(raster.face, d)
        if col.ndim != 4 or face.shape != col.shape[:3] or zw.shape != face.shape or pos.ndim != 3 or pos.shape[0] != col.shape[0] or pos.shape[2] != 4:
            raise ValueError(f'{who}: color must be (B, H, W, C), raster.zw and raster.face (B, H, W) and pos_clip (B, V, 4)')
        return col, pos, zw, face

    def antialias(self, topology, color, raster, pos_clip):
        """color (B,H,W,C) float32, C >= 1; raster: Engine.rasterize's dotdict (zw, face) of pos_clip (B,V,4); topology: Engine.topology of
        the same faces -> (B,H,W,C) float32 on the device with the silhouettes blended (include/relightableavatar.h: ra_antialias,
        DESIGN.md section 26).  A gather per pixel: no atomics, the same bits every time.  Nothing is read back."""
        col, pos, zw, face = self._antialias_args('Engine.antialias', color, raster, pos_clip)
        B, H, W, Cn = col.shape
        out = torch.empty_like(col)
        check(self.lib.ra_antialias(self.ctx, topology._handle, _ptr(col) if col.numel() else None, Cn, _ptr(pos) if pos.numel() else None, B, pos.shape[1],
                                    _ptr(zw) if zw.numel() else None, _ptr(face) if face.numel() else None, H, W, _ptr(out) if out.numel() else None,
                                    self.stream), 'ra_antialias')
        return out

    def antialias_backward(self, topology, color, raster, pos_clip, dout, pos_gradient_boost=1.0, want=('dcolor', 'dpos')):
        """the gradient of Engine.antialias, the face map and the set of active pairs held fixed: dout (B,H,W,C) -> dotdict(dcolor (B,H,W,C),
        dpos (B,V,4) with a zero z component) on the device (ra_antialias_backward).  pos_gradient_boost multiplies dpos only.  No float
        atomics: the same bits every time, and row b of dpos depends on view b alone.  One 4-byte read-back with dpos (the number of
        active pairs), none without."""
        col, pos, zw, face = self._antialias_args('Engine.antialias_backward', color, raster, pos_clip)
        g = _f32(dout, self.device)
        B, H, W, Cn = col.shape
        if g.shape != col.shape:
            raise ValueError(f'Engine.antialias_backward: dout must be ({B}, {H}, {W}, {Cn})')
        out = dotdict()
        if 'dcolor' in want:
            out.dcolor = torch.empty_like(col)
        if 'dpos' in want:
            out.dpos = torch.empty_like(pos)
        opt = lambda t: _ptr(t) if t is not None and t.numel() else None
        if not want:
            return out
        check(self.lib.ra_antialias_backward(self.ctx, topology._handle, opt(col), Cn, opt(pos), B, pos.shape[1], opt(zw), opt(face), H, W, opt(g),
                                             float(pos_gradient_boost), _ptr(out.get('dcolor')), _ptr(out.get('dpos')), self.stream), 'ra_antialias_backward')
        return out

    def raster_db(self, pos_clip, faces, raster):
        """pos_clip (B,V,4) or (V,4), faces (F,3), raster: Engine.rasterize's dotdict (face) of them -> rast_db (B,H,W,4) float32 on the
        device: the pixel differentials (du/dX, du/dY, dv/dX, dv/dY) of the barycentrics, nvdiffrast's layout, 0 where a pixel is empty
        (include/relightableavatar.h: ra_raster_db).  Nothing is read back."""
        d = self.device
        pos = _f32(pos_clip, d)
        pos = pos[None] if pos.ndim == 2 else pos
        face = _i32(raster.face, d)
        if pos.ndim != 3 or pos.shape[2] != 4 or face.ndim != 3 or face.shape[0] != pos.shape[0]:
            raise ValueError('Engine.raster_db: pos_clip must be (B, V, 4) or (V, 4) and raster.face (B, H, W)')
        f = _i32(faces.reshape(-1, 3), d)
        B, H, W = face.shape
        out = torch.empty(B, H, W, 4, dtype=torch.float32, device=d)
        check(self.lib.ra_raster_db(self.ctx, _ptr(pos) if pos.numel() else None, B, pos.shape[1], _ptr(f) if f.numel() else None, f.shape[0], _ptr(face), H, W,
                                    _ptr(out), self.stream), 'ra_raster_db')
        return out

    def interpolate_da(self, attrs, raster, faces, rast_db, channels):
        """attrs (V,A) or (B,V,A), raster: Engine.rasterize's dotdict (face), rast_db: Engine.raster_db's, channels: 1 .. 64 channel
        indices in [0, A) -> (B,H,W,2n) float32 on the device, (da/dX, da/dY) per selected channel (ra_interpolate_da).  Forward only;
        nothing is read back."""
        d = self.device
        a, db = _f32(attrs, d), _f32(rast_db, d)
        face = _i32(raster.face, d)
        B, H, W = face.shape
        if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[0] != B) or db.shape != (B, H, W, 4):
            raise ValueError(f'Engine.interpolate_da: attrs must be (V, A) or ({B}, V, A) and rast_db ({B}, {H}, {W}, 4)')
        ch = [int(c) for c in channels]
        f = _i32(faces.reshape(-1, 3), d)
        out = torch.empty(B, H, W, 2 * len(ch), dtype=torch.float32, device=d)
        check(self.lib.ra_interpolate_da(self.ctx, _ptr(a) if a.numel() else None, int(a.ndim == 3), a.shape[-2], a.shape[-1], _ptr(f) if f.numel() else None,
                                         f.shape[0], _ptr(face), _ptr(db), B, H, W, (C.c_int * max(len(ch), 1))(*ch), len(ch), _ptr(out), self.stream),
              'ra_interpolate_da')
        return out

    def texture_mips(self, tex, max_mip_level=None):
        """tex (TH,TW,C) or (Bt,TH,TW,C) -> (a list of the chain's levels, each (Bt,h,w,C) float32 on the device, level 0 a copy of tex):
        level l + 1 is the 2 x 2 mean of level l while both extents are even and above 1 (ra_texture_mips).  Nothing is read back."""
        t = _f32(tex, self.device)
        t = t[None] if t.ndim == 3 else t
        Bt, TH, TW, Cn = t.shape
        lmax, off = C.c_int(0), (C.c_longlong * (_lib.RA_TEX_MAX_LEVELS + 1))()
        mm = _lib.RA_TEX_MAX_LEVELS - 1 if max_mip_level is None else int(max_mip_level)
        check(self.lib.ra_texture_mips(None, None, Bt, TH, TW, Cn, mm, None, C.byref(lmax), off, self.stream), 'ra_texture_mips')
        total = off[lmax.value + 1]
        buf = torch.empty(Bt, total, Cn, dtype=torch.float32, device=self.device)
        check(self.lib.ra_texture_mips(self.ctx, _ptr(t), Bt, TH, TW, Cn, mm, _ptr(buf), C.byref(lmax), off, self.stream), 'ra_texture_mips')
        return [buf[:, off[l]:off[l + 1]].reshape(Bt, TH >> l, TW >> l, Cn) for l in range(lmax.value + 1)]

    def _texture_args(self, who, tex, uv, uv_da, filter_mode, boundary_mode, max_mip_level):
        d = self.device
        t, q = _f32(tex, d), _f32(uv, d)
        t = t[None] if t.ndim == 3 else t
        if filter_mode == 'auto':
            filter_mode = 'linear-mipmap-linear' if uv_da is not None else 'linear'
        if filter_mode not in _lib.RA_TEX_FILTERS or boundary_mode not in _lib.RA_TEX_BOUNDARIES:
            raise NotImplementedError(f'{who}: filter_mode {filter_mode!r} / boundary_mode {boundary_mode!r} is not supported '
                                      f'({sorted(_lib.RA_TEX_FILTERS)} and {sorted(_lib.RA_TEX_BOUNDARIES)} are)')
        if t.ndim != 4 or q.ndim != 4 or q.shape[3] != 2 or t.shape[0] not in (1, q.shape[0]):
            raise ValueError(f'{who}: tex must be (TH, TW, C), (1, TH, TW, C) or (B, TH, TW, C) and uv (B, H, W, 2)')
        da = None
        if filter_mode == 'linear-mipmap-linear':
            if uv_da is None:
                raise ValueError(f'{who}: linear-mipmap-linear needs uv_da')
            da = _f32(uv_da, d)
            if da.shape != q.shape[:3] + (4,):
                raise ValueError(f'{who}: uv_da must be (B, H, W, 4)')
        mm = _lib.RA_TEX_MAX_LEVELS - 1 if max_mip_level is None else int(max_mip_level)
        return t, q, da, _lib.RA_TEX_FILTERS[filter_mode], _lib.RA_TEX_BOUNDARIES[boundary_mode], mm

    def texture(self, tex, uv, uv_da=None, filter_mode='auto', boundary_mode='wrap', max_mip_level=None):
        """tex (TH,TW,C), (1,TH,TW,C) shared by the views or (B,TH,TW,C), row 0 at v = 0, 1 <= C <= 64; uv (B,H,W,2); uv_da (B,H,W,4) =
        (du/dX, du/dY, dv/dX, dv/dY) -> (B,H,W,C) float32 on the device (include/relightableavatar.h: ra_texture).
        filter_mode 'nearest', 'linear', 'linear-mipmap-linear' or 'auto' (the last with uv_da, else 'linear'); boundary_mode 'wrap' or
        'clamp'; max_mip_level None: as many levels as the sizes allow.  A non-finite uv gives 0.  Nothing is read back."""
        t, q, da, flt, bnd, mm = self._texture_args('Engine.texture', tex, uv, uv_da, filter_mode, boundary_mode, max_mip_level)
        Bt, TH, TW, Cn = t.shape
        B, H, W = q.shape[:3]
        out = torch.empty(B, H, W, Cn, dtype=torch.float32, device=self.device)
        check(self.lib.ra_texture(self.ctx, _ptr(t), Bt, TH, TW, Cn, _ptr(q), _ptr(da), B, H, W, flt, bnd, mm, _ptr(out), self.stream), 'ra_texture')
        return out

    def texture_backward(self, tex, uv, dout, uv_da=None, filter_mode='auto', boundary_mode='wrap', max_mip_level=None, want=('duv', 'dtex')):
        """the gradient of Engine.texture, first order (the texel cells, the level pair and lod held fixed; none to uv_da): dout (B,H,W,C)
        -> dotdict(duv (B,H,W,2), dtex shaped like tex) on the device (ra_texture_backward).  No float atomics: the same bits every
        time; row t of a per-view dtex depends on view t alone, a shared texture adds the views in ascending order.  Nothing is read
        back."""
        t, q, da, flt, bnd, mm = self._texture_args('Engine.texture_backward', tex, uv, uv_da, filter_mode, boundary_mode, max_mip_level)
        g = _f32(dout, self.device)
        Bt, TH, TW, Cn = t.shape
        B, H, W = q.shape[:3]
        if g.shape != (B, H, W, Cn):
            raise ValueError(f'Engine.texture_backward: dout must be ({B}, {H}, {W}, {Cn})')
        out = dotdict()
        if 'duv' in want:
            out.duv = torch.empty_like(q)
        if 'dtex' in want:
            out.dtex = torch.empty_like(t)
        if not want:
            return out
        check(self.lib.ra_texture_backward(self.ctx, _ptr(t), Bt, TH, TW, Cn, _ptr(q), _ptr(da), B, H, W, flt, bnd, mm, _ptr(g), _ptr(out.get('duv')),
                                           _ptr(out.get('dtex')), self.stream), 'ra_texture_backward')
        if 'dtex' in out and tex.ndim == 3:
            out.dtex = out.dtex[0]
        return out

    def cloth(self, topology, rest_verts, vm, fm, material=None):
        """topology (Engine.topology), rest_verts (V,3), vm (M,2) material coordinates, fm (F,3) integers into vm, material (an
        object or dict with density, thickness, young_modulus, poisson_ratio, bending_multiplier, stretch_multiplier and optionally
        material_multiplier; None: the reference's StVKMaterial defaults) -> a Cloth handle (include/relightableavatar.h:
        ra_cloth_create).  One 4-byte read-back: the verdict on fm."""
        get = (lambda k, d: material.get(k, d)) if isinstance(material, dict) else (lambda k, d: getattr(material, k, d))
        m = _lib.ra_cloth_material(*[float(get(k, d)) for k, d in _lib.CLOTH_MATERIAL_DEFAULTS])
        v = _f32(rest_verts.reshape(-1, 3), self.device)
        vm = _f32(vm.reshape(-1, 2), self.device)
        fm = _i32(fm.reshape(-1, 3), self.device)
        if fm.shape[0] != topology.F:
            raise ValueError(f'Engine.cloth: fm must be ({topology.F}, 3)')
        handle = C.c_void_p()
        check(self.lib.ra_cloth_create(self.ctx, topology._handle, _ptr(v) if v.numel() else None, v.shape[0], _ptr(vm) if vm.numel() else None,
                                       vm.shape[0], _ptr(fm) if fm.numel() else None, C.byref(m), C.byref(handle), self.stream), 'ra_cloth_create')
        coeffs = (C.c_double * 5)()
        check(self.lib.ra_cloth_material_derive(C.byref(m), coeffs), 'ra_cloth_material_derive')
        return Cloth(self, handle, topology, tuple(coeffs))

    def cloth_inertia(self, mass, x_next, x_curr, v_curr, delta_t, accel=None, grads=(True, True, True)):
        """mass (V,), x_next, x_curr, v_curr (rows,V,3) -> (value (rows,) float64 per-row sums, g_next, g_curr, g_vel (rows,V,3) float32
        or None where not wanted) on the device (ra_cloth_inertia): inertia_term, or dynamic_term with accel (3 floats)"""
        d = self.device
        m, a, b, c = _f32(mass.reshape(-1), d), _f32(x_next, d), _f32(x_curr, d), _f32(v_curr, d)
        if a.ndim != 3 or a.shape[1:] != (m.shape[0], 3) or b.shape != a.shape or c.shape != a.shape:
            raise ValueError('cloth_inertia: x_next, x_curr, v_curr must be (rows, V, 3) with V the length of mass')
        value = torch.empty(a.shape[0], dtype=torch.float64, device=d)
        outs = [torch.empty_like(a) if w else None for w in grads]
        acc = (C.c_float * 3)(*[float(t) for t in accel]) if accel is not None else None
        check(self.lib.ra_cloth_inertia(self.ctx, _ptr(m), _ptr(a), _ptr(b), _ptr(c), a.shape[0], a.shape[1], float(delta_t), acc, _ptr(value),
                                        *[_ptr(o) for o in outs], self.stream), 'ra_cloth_inertia')
        return (value, *outs)

    def adam_uniform_step(self, param, grad, g1, g2, step, lr=0.1, betas=(0.9, 0.999)):
        """one AdamUniform step IN PLACE on float32 device tensors (include/relightableavatar.h: ra_adam_uniform_step): param, grad and
        g1 of one shape, g2 a single float; step = 1, 2, ..."""
        for name, t in (('param', param), ('grad', grad), ('g1', g1), ('g2', g2)):
            if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f'Engine.adam_uniform_step: {name} must be a contiguous float32 tensor on the device')
        if grad.shape != param.shape or g1.shape != param.shape or g2.numel() != 1:
            raise ValueError('Engine.adam_uniform_step: grad and g1 must have the shape of param, g2 one element')
        n = param.numel()
        check(self.lib.ra_adam_uniform_step(self.ctx, _ptr(param) if n else None, _ptr(grad) if n else None, _ptr(g1) if n else None, _ptr(g2), n, int(step),
                                            float(lr), float(betas[0]), float(betas[1]), self.stream), 'ra_adam_uniform_step')

    def ray_tri_pairs(self, ray_o, ray_d, tris):
        """ray_o, ray_d (n,3), tris (F,3,3) -> (u, v, t), each (n,F) fp32 on the device: the reference's moller_trumbore for every
        (ray, triangle) pair, no guard (include/relightableavatar.h: ra_ray_tri_pairs).  n x F must stay below 2^31."""
        d = self.device
        o, r, tr = _f32(ray_o.reshape(-1, 3), d), _f32(ray_d.reshape(-1, 3), d), _f32(tris.reshape(-1, 3, 3), d)
        if o.shape != r.shape:
            raise ValueError('ray_tri_pairs: ray_o and ray_d must hold the same number of rays')
        n, f = o.shape[0], tr.shape[0]
        if n * f >= 2 ** 31:
            raise ValueError('ray_tri_pairs: n x F must stay below 2^31')
        u, v, t = (torch.empty(n, f, dtype=torch.float32, device=d) for _ in range(3))
        check(self.lib.ra_ray_tri_pairs(self.ctx, _ptr(o), _ptr(r), n, _ptr(tr), f, _ptr(u), _ptr(v), _ptr(t), self.stream), 'ra_ray_tri_pairs')
        return u, v, t

    def sdf_volume(self, xs, ys, zs, mode, dist_th, fill=-10., pad=10, verts=None, K=None):
        """the padded volume of -sdf for marching cubes (include/relightableavatar.h: ra_sdf_volume).  xs, ys, zs: the axis
        coordinates (data_utils.mesh_grid_axes); mode 'canonical' | 'tpose' | 'posed'; verts (V,3): what the K-NN filter measures
        against — default the current frame's template vertices, which is right for 'canonical' and 'tpose'; 'posed' needs the
        world vertices (batch.wverts).  K: cfg.sample_vert_cnt.  Returns (nx + 2 pad, ny + 2 pad, nz + 2 pad) float32 on the device;
        self.last_kept holds the kept points.  One blocking read-back."""
        if mode not in _lib.RA_VOLUME_MODES:
            raise ValueError(f'sdf_volume: mode must be one of {tuple(_lib.RA_VOLUME_MODES)}')
        d = self.device
        if verts is None:
            if mode == 'posed' or self._frame_refs is None:
                raise ValueError("sdf_volume: mode 'posed' needs verts= (the world vertices), the other modes a frame (set_frame)")
            verts = self._frame_refs[self.FRAME_KEYS.index('tverts')]
        verts = _f32(verts.reshape(-1, 3), d)
        ax = [_f32(torch.as_tensor(a).reshape(-1), d) for a in (xs, ys, zs)]
        pad = int(pad)
        vol = torch.empty(tuple(a.numel() + 2 * pad for a in ax), dtype=torch.float32, device=d)
        kept = C.c_int()
        check(self.lib.ra_sdf_volume(self.ctx, _ptr(ax[0]), ax[0].numel(), _ptr(ax[1]), ax[1].numel(), _ptr(ax[2]), ax[2].numel(), _lib.RA_VOLUME_MODES[mode],
                                     _ptr(verts), verts.shape[0], int(self.cfg.sample_vert_cnt if K is None else K), float(dist_th), float(fill), pad,
                                     _ptr(vol), C.byref(kept), self.stream), 'ra_sdf_volume')
        self.last_kept = kept.value
        return vol

    def marching_cubes(self, volume, iso):
        """volume (nx,ny,nz) float -> (verts (V,3) float32 in index coordinates, faces (F,3) int32) on the device
        (include/relightableavatar.h: ra_marching_cubes).  One blocking read-back: the two counts, to allocate the result."""
        if volume.ndim != 3 or min(volume.shape) < 2:
            raise ValueError('marching_cubes: volume must be (nx, ny, nz) with at least 2 points per axis')
        d = self.device
        vol = _f32(volume, d)
        nx, ny, nz = (int(v) for v in vol.shape)
        nv, nf = C.c_int(), C.c_int()
        check(self.lib.ra_marching_cubes(self.ctx, _ptr(vol), nx, ny, nz, float(iso), None, None, C.byref(nv), C.byref(nf), self.stream), 'ra_marching_cubes')
        verts = torch.empty(nv.value, 3, dtype=torch.float32, device=d)
        faces = torch.empty(nf.value, 3, dtype=torch.int32, device=d)
        if nv.value:        # a crossed edge has a cell with a triangle: faces too
            check(self.lib.ra_marching_cubes(self.ctx, _ptr(vol), nx, ny, nz, float(iso), _ptr(verts), _ptr(faces), None, None, self.stream), 'ra_marching_cubes')
        return verts, faces

    def _mc_volume(self, volume, attrs, who):
        if volume.ndim != 3 or min(volume.shape) < 2:
            raise ValueError(f'{who}: volume must be (nx, ny, nz) with at least 2 points per axis')
        vol = _f32(volume, self.device)
        if attrs is not None:
            if attrs.numel() % vol.numel() or attrs.shape[0] not in (vol.shape[0], vol.numel()):
                raise ValueError(f'{who}: attrs must be (nx, ny, nz, C) or (nx * ny * nz, C)')
            attrs = _f32(attrs, self.device).reshape(vol.numel(), -1)
        return vol, attrs

    def marching_cubes_attrs(self, volume, iso, attrs, n_verts):
        """grid attributes (nx,ny,nz,C) or (n,C) carried to the n_verts vertices of Engine.marching_cubes(volume, iso), in its vertex
        order: (n_verts, C) float32, (1 - t) A[p] + t A[q] along each crossed edge (include/relightableavatar.h:
        ra_marching_cubes_attrs).  Asynchronous: no read-back."""
        vol, A = self._mc_volume(volume, attrs, 'marching_cubes_attrs')
        nx, ny, nz = (int(v) for v in vol.shape)
        out = torch.empty(int(n_verts), A.shape[1], dtype=torch.float32, device=self.device)
        check(self.lib.ra_marching_cubes_attrs(self.ctx, _ptr(vol), nx, ny, nz, float(iso), _ptr(A), A.shape[1], int(n_verts), _ptr(out), self.stream),
              'ra_marching_cubes_attrs')
        return out

    def marching_cubes_backward(self, volume, iso, n_verts, dverts=None, attrs=None, dattr=None, want=('dvolume', 'dattrs')):
        """the backward of Engine.marching_cubes / marching_cubes_attrs at fixed topology (ra_marching_cubes_backward): dverts (n_verts,3)
        and / or dattr (n_verts,C) with the grid attributes -> dotdict(dvolume (nx,ny,nz), dattrs in attrs' shape), those of `want`
        ('dattrs' needs attrs).  A gather over the grid points: bit-reproducible, asynchronous, no read-back."""
        unknown = set(want) - {'dvolume', 'dattrs'}
        if unknown or not want:
            raise ValueError(f"marching_cubes_backward: want must name 'dvolume' and / or 'dattrs', got {tuple(want)}")
        if (attrs is None) != (dattr is None):
            raise ValueError('marching_cubes_backward: attrs and dattr go together')
        if 'dattrs' in want and attrs is None and tuple(want) != ('dvolume', 'dattrs'):
            raise ValueError("marching_cubes_backward: 'dattrs' needs attrs and dattr")
        vol, A = self._mc_volume(volume, attrs, 'marching_cubes_backward')
        nx, ny, nz = (int(v) for v in vol.shape)
        d, n_verts = self.device, int(n_verts)
        Cn = A.shape[1] if A is not None else 0
        if dverts is not None:
            dverts = _f32(dverts, d)
            if tuple(dverts.shape) != (n_verts, 3):
                raise ValueError('marching_cubes_backward: dverts must be (n_verts, 3)')
        if dattr is not None:
            dattr = _f32(dattr, d)
            if tuple(dattr.shape) != (n_verts, Cn):
                raise ValueError('marching_cubes_backward: dattr must be (n_verts, C)')
        out = dotdict()
        if 'dvolume' in want:
            out.dvolume = torch.empty_like(vol)
        if 'dattrs' in want and A is not None:
            out.dattrs = torch.empty(attrs.shape, dtype=torch.float32, device=d)
        if 'dvolume' not in out and not Cn:      # nothing to write
            return out
        check(self.lib.ra_marching_cubes_backward(self.ctx, _ptr(vol), nx, ny, nz, float(iso), _ptr(dverts) if n_verts else None, n_verts,
                                                  _ptr(A), _ptr(dattr) if n_verts else None, Cn, _ptr(out.get('dvolume')),
                                                  _ptr(out.get('dattrs')) if Cn else None, self.stream), 'ra_marching_cubes_backward')
        return out

    def largest_component(self, verts, faces):
        """verts (V,3) float, faces (F,3) integer -> (verts, faces) of the largest component of faces connected through shared edges, on
        the device: the most vertices, then the lowest face index; referenced vertices and faces in their original order
        (include/relightableavatar.h: ra_mesh_largest_component).  One blocking read-back unless the mesh needs more than
        ra_mcubes_tile(1) label passes."""
        d = self.device
        v = _f32(verts.reshape(-1, 3), d)
        f = _i32(faces.reshape(-1, 3), d)
        nv, nf = C.c_int(), C.c_int()
        args = (self.ctx, _ptr(v) if v.shape[0] else None, v.shape[0], _ptr(f) if f.shape[0] else None, f.shape[0])
        check(self.lib.ra_mesh_largest_component(*args, None, None, C.byref(nv), C.byref(nf), self.stream), 'ra_mesh_largest_component')
        ov = torch.empty(nv.value, 3, dtype=torch.float32, device=d)
        of = torch.empty(nf.value, 3, dtype=torch.int32, device=d)
        if nf.value:
            check(self.lib.ra_mesh_largest_component(*args, _ptr(ov), _ptr(of), None, None, self.stream), 'ra_mesh_largest_component')
        return ov, of

    # ------------------------------------------------------------------ measurement
    def counters(self) -> dotdict:
        c = ra_counters()
        check(self.lib.ra_get_counters(self.ctx, C.byref(c), self.stream), 'ra_get_counters')
        return dotdict({k: int(getattr(c, k)) for k, _ in ra_counters._fields_})

    def reset_counters(self):
        check(self.lib.ra_reset_counters(self.ctx, self.stream), 'ra_reset_counters')

    def set_gate(self, gate):
        """attach (or, with None, detach) a pipeline.Gate: contexts sharing one run their light-visibility stages one after the other"""
        check(self.lib.ra_set_gate(self.ctx, gate.handle if gate is not None else C.c_void_p()), 'ra_set_gate')
        self._gate = gate        # keeps it alive as long as the context refers to it

    def set_knn_mode(self, use_bvh=True):
        check(self.lib.ra_set_knn_mode(self.ctx, int(use_bvh)), 'ra_set_knn_mode')
        self._frame_key = None

    def gen_rays(self, H, W, K, R, T, bounds, count=None):
        """N2: rays of an H x W pinhole view culled against the body's bounding box, on the device.
        K, R (3,3), T (3,) or (3,1): anything numpy can read; bounds (2,3).  Returns the reference's
        get_rays_within_bounds outputs as device tensors: ray_o, ray_d (P,3), near, far (P,), mask_at_box (H,W) bool.
        count: the number of in-box rays if the caller knows it (H * W for an unbounded box): skips the read-back and its synchronisation."""
        bufs, cnt = self._gen_rays(H, W, K, R, T, bounds, host_count=count is None)
        P = cnt if count is None else int(count)
        ro, rd, near, far, mask = bufs
        return dotdict(ray_o=ro[:P], ray_d=rd[:P], near=near[:P], far=far[:P], mask_at_box=mask.view(int(H), int(W)).bool())

    def _gen_rays(self, H, W, K, R, T, bounds, host_count, count_dev=None):
        import numpy as np
        Kd = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(9))
        Rd = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(9))
        Td = np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(3))
        on_dev = isinstance(bounds, torch.Tensor) and bounds.is_cuda
        if on_dev:           # a box that is still being computed on the stream (pose_frame's wbounds): read on the device, no round trip
            bdev = _f32(bounds.reshape(6), self.device)
            bd = None
        else:
            bd = np.ascontiguousarray(np.asarray(bounds.detach().cpu() if isinstance(bounds, torch.Tensor) else bounds, dtype=np.float32).reshape(6))
        n = int(H) * int(W)
        d = self.device
        ro, rd = torch.empty(n, 3, device=d), torch.empty(n, 3, device=d)
        near, far = torch.empty(n, device=d), torch.empty(n, device=d)
        mask = torch.empty(n, device=d, dtype=torch.uint8)
        cnt = C.c_int(0)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        check(self.lib.ra_gen_rays(self.ctx, int(H), int(W), dp(Kd), dp(Rd), dp(Td), None if bd is None else bd.ctypes.data_as(C.POINTER(C.c_float)),
                                   _ptr(bdev) if on_dev else None, _ptr(ro), _ptr(rd), _ptr(near), _ptr(far), _ptr(mask),
                                   C.byref(cnt) if host_count else None, None if count_dev is None else _ptr(count_dev), self.stream), 'ra_gen_rays')
        return (ro, rd, near, far, mask), cnt.value

    def gen_rays_async(self, H, W, K, R, T, bounds, mask_to_host=False):
        """N2 for an animation loop: the rays of a frame whose box (`bounds`: a device tensor, e.g. pose_frame's wbounds) may still be on its
        way.  Nothing waits: the ray buffers have the frame's capacity (H * W), the in-box count and the box travel to pinned host memory
        behind an event, and `.result()` — called a pipeline turn later, when the kernels are long done — trims the buffers.  `mask_to_host`
        also brings mask_at_box to the host (the shard plan of an N-rank job is host work: shard.make_plan)."""
        n = int(H) * int(W)
        d = self.device
        count_dev = torch.empty(1, device=d, dtype=torch.int32)
        bufs, _ = self._gen_rays(H, W, K, R, T, bounds, host_count=False, count_dev=count_dev)
        bdev = _f32(bounds.reshape(6), d) if isinstance(bounds, torch.Tensor) else torch.as_tensor(bounds, dtype=torch.float32, device=d).reshape(6)
        host = torch.empty(8, dtype=torch.float32, pin_memory=True)             # [count (int bits) | 6 box floats]
        host[:1].view(torch.int32).copy_(count_dev, non_blocking=True)
        host[1:7].copy_(bdev, non_blocking=True)
        mask_host = None
        if mask_to_host:
            mask_host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
            mask_host.copy_(bufs[4], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(d))
        return RaysPending(bufs, host, mask_host, ev, int(H), int(W), (count_dev, bdev))

    def pose_frame(self, poses, tjoints, parents, tverts, weights, big_A, faces, Rh, Th, padding=0.05):
        """N3: per-frame body state on the device (base_dataset.py:308-397).  Small inputs (poses, tjoints (J,3), parents (J),
        big_A (J,4,4), Rh, Th, faces (F,3)) are read from host memory; tverts (N,3) and weights (N,J) are device tensors
        (moved if needed).  Returns device tensors A (J,4,4), joints, tverts (T pose), pverts, wverts, pnorm, R, pbounds, wbounds, and the
        device copies of poses (J,3) / Th (3).  Asynchronous: nothing waits for the stream (the host inputs are staged in pinned memory)."""
        import numpy as np
        h32 = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)
        hp, hj, hb, hr, ht = h32(poses).reshape(-1, 3), h32(tjoints).reshape(-1, 3), h32(big_A).reshape(-1, 16), h32(Rh).reshape(3), h32(Th).reshape(3)
        par = np.ascontiguousarray(parents.cpu().numpy() if isinstance(parents, torch.Tensor) else parents, dtype=np.int32)
        fc = np.ascontiguousarray(faces.cpu().numpy() if isinstance(faces, torch.Tensor) else faces, dtype=np.int32).reshape(-1, 3)
        d = self.device
        tv, w = _f32(tverts.reshape(-1, 3) if isinstance(tverts, torch.Tensor) else torch.as_tensor(tverts).reshape(-1, 3), d), \
            _f32(weights if isinstance(weights, torch.Tensor) else torch.as_tensor(weights), d)
        w = w.reshape(tv.shape[0], -1)
        J, N = hp.shape[0], tv.shape[0]
        o = dotdict(A=torch.empty(J, 4, 4, device=d), joints=torch.empty(J, 3, device=d), tverts=torch.empty(N, 3, device=d),
                    pverts=torch.empty(N, 3, device=d), wverts=torch.empty(N, 3, device=d), pnorm=torch.empty(N, 3, device=d),
                    R=torch.empty(3, 3, device=d), pbounds=torch.empty(2, 3, device=d), wbounds=torch.empty(2, 3, device=d),
                    poses=torch.empty(J, 3, device=d), Th=torch.empty(3, device=d))
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        pin = ra_pose_in(poses=fp(hp), tjoints=fp(hj), big_A=fp(hb), Rh=fp(hr), Th=fp(ht), parents=par.ctypes.data_as(C.POINTER(C.c_int)),
                         faces=fc.ctypes.data_as(C.POINTER(C.c_int)), n_bones=J, n_faces=fc.shape[0], n_verts=N, tverts=_ptr(tv), weights=_ptr(w),
                         bounds_padding=float(padding))
        pout = ra_pose_out(A=_ptr(o.A), joints=_ptr(o.joints), tpose=_ptr(o.tverts), pverts=_ptr(o.pverts), wverts=_ptr(o.wverts),
                           pnorm=_ptr(o.pnorm), R=_ptr(o.R), pbounds=_ptr(o.pbounds), wbounds=_ptr(o.wbounds), poses=_ptr(o.poses), Th=_ptr(o.Th))
        check(self.lib.ra_pose_frame(self.ctx, C.byref(pin), C.byref(pout), self.stream), 'ra_pose_frame')
        return o

    def grow_bounds(self, wbounds, margin):
        """batch.wbounds (1,2,3) -= / += margin in place, one launch (the reference's per-chunk quirk, sphere_tracing_renderer.py:1020-1022)"""
        assert wbounds.is_cuda and wbounds.dtype == torch.float32 and wbounds.is_contiguous() and wbounds.numel() == 6
        check(self.lib.ra_grow_bounds(self.ctx, _ptr(wbounds), float(margin), self.stream), 'ra_grow_bounds')
        torch.autograd.graph.increment_version(wbounds)      # an in-place write torch did not see: keep its version counter honest
        return wbounds

    def shift_envmap(self, image, shift):
        """N4: rotate_envmap's shift_image: (H,W,C) or (1,H,W,C) -> same shape, shifted `shift` pixels with wrap-around."""
        x = _f32(image, self.device)
        lead = x.shape[:-3]
        x3 = x.reshape(x.shape[-3:])
        out = torch.empty_like(x3)
        check(self.lib.ra_shift_envmap(self.ctx, _ptr(x3), x3.shape[0], x3.shape[1], x3.shape[2], float(shift), _ptr(out), self.stream),
              'ra_shift_envmap')
        return out.reshape(*lead, *x3.shape)

    def add_light_probe(self, rgb, probe, H, W, cam_R, uH, uW):
        """N4: add_light_probe: rgb (..., H*W, 3) gets the probe inset in its top-left uH x uW pixels (in place on a device copy)."""
        import numpy as np
        out = _f32(rgb, self.device).clone()
        pr = _f32(probe[0] if probe.ndim == 4 else probe, self.device)
        R = np.ascontiguousarray(np.asarray(cam_R.detach().cpu() if isinstance(cam_R, torch.Tensor) else cam_R, dtype=np.float32).reshape(9))
        check(self.lib.ra_add_light_probe(self.ctx, _ptr(out), int(H), int(W), _ptr(pr), pr.shape[0], pr.shape[1],
                                          R.ctypes.data_as(C.POINTER(C.c_float)), int(uH), int(uW), self.stream), 'ra_add_light_probe')
        return out

    def enable_timing(self, on=True):
        check(self.lib.ra_enable_timing(self.ctx, int(on)), 'ra_enable_timing')

    def mlp_time(self):
        ms, n = C.c_float(), C.c_int()
        check(self.lib.ra_get_mlp_time(self.ctx, C.byref(ms), C.byref(n), self.stream), 'ra_get_mlp_time')
        return float(ms.value), int(n.value)

    def kernel_time(self, kind):
        """(ms, launches) of one kernel family since the last reset: 0 = fused distance query (K3, every width), 1 = full query (K4),
        2 = the 8-wave K3 only (launches that fill the chip), 3 = the 2- / 4-wave K3, 4 = the compensated distance query (K3C / K3CC)."""
        ms, n = C.c_float(), C.c_int()
        check(self.lib.ra_get_kernel_time(self.ctx, int(kind), C.byref(ms), C.byref(n), self.stream), 'ra_get_kernel_time')
        return float(ms.value), int(n.value)

    # ------------------------------------------------------------------ test hooks
    def debug_mlp(self, bpts, want_feat=True):
        d = self.device
        bpts = _f32(bpts.reshape(-1, 3), d)
        n = bpts.shape[0]
        resd, sdf = torch.empty(n, 3, device=d), torch.empty(n, device=d)
        feat = torch.empty(n, 256, device=d) if want_feat else None
        check(self.lib.ra_debug_mlp(self.ctx, _ptr(bpts), n, _ptr(resd), _ptr(sdf), _ptr(feat), self.stream), 'ra_debug_mlp')
        return resd, sdf, feat

    def debug_full(self, bpts):
        d = self.device
        bpts = _f32(bpts.reshape(-1, 3), d)
        n = bpts.shape[0]
        grad, sdf, feat = torch.empty(n, 3, device=d), torch.empty(n, device=d), torch.empty(n, 256, device=d)
        raw = torch.zeros(n, self.lib.ra_raw_channels(self.ctx), device=d)
        check(self.lib.ra_debug_full(self.ctx, _ptr(bpts), n, _ptr(grad), _ptr(sdf), _ptr(feat), _ptr(raw), self.stream), 'ra_debug_full')
        return grad, sdf, feat, raw

    def debug_aabb(self, o, d, bbox6):
        dv = self.device
        o, d = _f32(o.reshape(-1, 3), dv), _f32(d.reshape(-1, 3), dv)
        n = o.shape[0]
        near, far = torch.empty(n, device=dv), torch.empty(n, device=dv)
        bb = _bbox6(bbox6)
        check(self.lib.ra_debug_aabb(self.ctx, _ptr(o), _ptr(d), n, bb, _ptr(near), _ptr(far), self.stream), 'ra_debug_aabb')
        return near, far

    def debug_lvis(self, surf, norm, acc, bbox6, lvis_cfg=None):
        """light_visibility on given surface points: (n,512) lvis, ldot"""
        dv = self.device
        c = self.cfg
        lv = c.obj_lvis if lvis_cfg is None else lvis_cfg
        surf, norm, acc = _f32(surf.reshape(-1, 3), dv), _f32(norm.reshape(-1, 3), dv), _f32(acc.reshape(-1), dv)
        n = surf.shape[0]
        L = c.env_h * c.env_w
        lvis, ldot = torch.empty(n, L, device=dv), torch.empty(n, L, device=dv)
        bb = _bbox6(bbox6)
        p = self.trace_params(lv, lv.dist_th, not c.no_dfss)
        check(self.lib.ra_debug_lvis(self.ctx, _ptr(surf), _ptr(norm), _ptr(acc), n, bb, C.byref(p), float(lv.near_offset), _ptr(lvis), _ptr(ldot),
                                     self.stream), 'ra_debug_lvis')
        return lvis, ldot

    def debug_brdf(self, p2l, p2c, normal, albedo, rough):
        """p2l (L,N,3), others per point -> (L,N,3)"""
        dv = self.device
        L, N = p2l.shape[0], p2l.shape[1]
        a = [_f32(t, dv) for t in (p2l.reshape(L * N, 3), p2c.reshape(N, 3), normal.reshape(N, 3), albedo.reshape(N, 3), rough.reshape(N))]
        out = torch.empty(L, N, 3, device=dv)
        check(self.lib.ra_debug_brdf(self.ctx, *[_ptr(t) for t in a], L, N, _ptr(out), self.stream), 'ra_debug_brdf')
        return out

    def debug_bvh_ids(self):
        """vertex ids of the frame's box structure in leaf order (numpy int32; padding 0x7fffffff), empty without a structure"""
        import numpy as np
        cap = 32 * 1024
        ids = np.empty(cap, dtype=np.int32)
        n = C.c_int()
        check(self.lib.ra_debug_bvh_ids(self.ctx, ids.ctypes.data_as(C.c_void_p), cap, C.byref(n), self.stream), 'ra_debug_bvh_ids')
        return ids[:n.value].copy()

    def debug_hdq(self, x, dist_th):
        d = self.device
        x = _f32(x.reshape(-1, 3), d)
        n = x.shape[0]
        o = dotdict(sdf_coarse=torch.empty(n, device=d), sdf_batch=torch.empty(n, 3, device=d),
                    nn_batch=torch.empty(n, 3, device=d, dtype=torch.int32), d2=torch.empty(n, 3, device=d),
                    bpts=torch.empty(n, 3, device=d), tpts=torch.empty(n, 3, device=d), mats=torch.empty(n, 24, device=d))
        cnt = C.c_int()
        check(self.lib.ra_debug_hdq(self.ctx, _ptr(x), n, dist_th, _ptr(o.sdf_coarse), _ptr(o.sdf_batch), _ptr(o.nn_batch), _ptr(o.d2),
                                    _ptr(o.bpts), _ptr(o.tpts), _ptr(o.mats), C.byref(cnt), self.stream), 'ra_debug_hdq')
        o.fine_count = int(cnt.value)
        return o

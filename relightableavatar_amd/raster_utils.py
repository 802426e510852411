"""The reference's lib/utils/raster_utils.py on the device rasteriser (Engine.rasterize / Engine.interpolate / Engine.antialias /
Engine.texture, DESIGN.md sections 25, 26 and 27).

The camera helpers are the reference's torch arithmetic.  `rasterize`, `interpolate`, `antialias` and `texture` are autograd ops over the
HIP kernels, first order only, in nvdiffrast's layouts and argument order.  `render_nvdiffrast` is the reference's ATTRIBUTE path and
`render_textured` its two TEXTURE branches (uv + img, with or without attributes).

The texture path has names of its own, because the older calls keep their signatures, values and refusals: `rasterize_db` returns
(rast, rast_db), `interpolate_db` returns (out, out_da), `texture` is nvdiffrast's dr.texture, `render_textured` the reference's call
with uv / img.  `interpolate(rast_db=)` and `render_nvdiffrast(uv=, img=)` still raise NotImplementedError and name these.

Deliberate limits (DESIGN.md sections 6, 25, 26 and 27):
  * `texture` is this project's statement of the published algorithm (Laine et al. 2020, section 3.3; csrc/ra_texture_rules.hpp): first
    order with the texel cells, the level pair and the level of detail held fixed, so uv_da and rast_db carry no gradient (nvdiffrast
    differentiates lod); filter modes nearest, linear, linear-mipmap-linear and auto, boundary modes wrap and clamp;
    linear-mipmap-nearest, mip_level_bias, a prebuilt mip, and the boundary modes zero and cube raise NotImplementedError;
  * `antialias` is this project's statement of the published algorithm (Laine et al. 2020, section 3.4; csrc/ra_antialias_rules.hpp), not
    a reproduction of nvdiffrast's output: no fixed-point snapping, and only the own pixel's face is searched for silhouette edges, as
    in the paper.  render_nvdiffrast applies it only with antialias=True (the reference's behaviour); by default it skips that step, the
    soft mask comes from R_S supersampling alone and no gradient arises at silhouettes;
  * no depth peeling, no range mode, no scissor;
  * the sampling rules are this project's (csrc/ra_raster_rules.hpp), not nvdiffrast's fixed-point snapping.
"""
from typing import Union

import numpy as np
import torch
import torch.nn.functional as F

from .base_utils import dotdict


def get_ndc_perspective_matrix(K: Union[torch.Tensor, np.ndarray], H, W):
    """K (3,3)-like or (B,...) intrinsics -> the (4,4) or (B,4,4) matrix that takes camera-space points to clip space, the reference's:
    x, y to [-1, 1] over the image, z_clip = -2 CLIP_NEAR, w = z.  Pixel coordinate c maps to NDC 2 c / W - 1, so the rasteriser's
    sample of pixel i is the camera pixel coordinate i + 0.5."""
    CLIP_NEAR = 0.01
    if isinstance(K, torch.Tensor):
        ixt = K.new_zeros(K.shape[0], 4, 4) if K.ndim == 3 else K.new_zeros(4, 4)
    elif isinstance(K, np.ndarray):
        ixt = np.zeros((K.shape[0], 4, 4), dtype=K.dtype) if K.ndim == 3 else np.zeros((4, 4), dtype=K.dtype)
    else:
        raise NotImplementedError('unsupport data type for K conversion')
    ixt[..., 0, 0] = (K[..., 0, 0]) * 2.0 / W
    ixt[..., 1, 1] = (K[..., 1, 1]) * 2.0 / H
    ixt[..., 0, 2] = (K[..., 0, 2] - W / 2.0) * 2.0 / W
    ixt[..., 1, 2] = (K[..., 1, 2] - H / 2.0) * 2.0 / H
    ixt[..., 2, 2] = 0
    ixt[..., 2, 3] = -2 * CLIP_NEAR
    ixt[..., 3, 2] = 1
    ixt[..., 3, 3] = 0
    return ixt


def _eye4(like: torch.Tensor):
    return torch.eye(4, 4, device=like.device)[None].expand(like.shape[0], -1, -1).clone()


def make_rotation_y(ry: torch.Tensor):
    """ry (R,) -> (R,4,4) rotations about y"""
    Rs = _eye4(ry)
    siny, cosy = ry.sin(), ry.cos()
    Rs[:, 0, 0] = cosy
    Rs[:, 0, 2] = siny
    Rs[:, 1, 1] = 1.0
    Rs[:, 2, 0] = -siny
    Rs[:, 2, 2] = cosy
    return Rs


def make_rotation(rx: torch.Tensor = None, ry: torch.Tensor = None, rz: torch.Tensor = None):
    """Euler angles (R,) each, a missing one is 0 -> (R,4,4): Rz @ Ry @ Rx"""
    assert not (rx is None and ry is None and rz is None)
    not_none = rx if rx is not None else (ry if ry is not None else rz)
    rx = torch.zeros_like(not_none) if rx is None else rx
    ry = torch.zeros_like(not_none) if ry is None else ry
    rz = torch.zeros_like(not_none) if rz is None else rz
    sinX, sinY, sinZ = rx.sin(), ry.sin(), rz.sin()
    cosX, cosY, cosZ = rx.cos(), ry.cos(), rz.cos()
    Rx = _eye4(ry)
    Rx[:, 1, 1] = cosX
    Rx[:, 1, 2] = -sinX
    Rx[:, 2, 1] = sinX
    Rx[:, 2, 2] = cosX
    Ry = _eye4(ry)
    Ry[:, 0, 0] = cosY
    Ry[:, 0, 2] = sinY
    Ry[:, 2, 0] = -sinY
    Ry[:, 2, 2] = cosY
    Rz = _eye4(ry)
    Rz[:, 0, 0] = cosZ
    Rz[:, 0, 1] = -sinZ
    Rz[:, 1, 0] = sinZ
    Rz[:, 1, 1] = cosZ
    return Rz.matmul(Ry).matmul(Rx)


def bilinear_interpolation(input: torch.Tensor, shape) -> torch.Tensor:
    """input (B,H,W,C) -> (B,*shape,C): F.interpolate, bilinear, align_corners=False"""
    return F.interpolate(input.permute(0, 3, 1, 2), shape, mode='bilinear', align_corners=False).permute(0, 2, 3, 1)


def _engine(engine):
    from .mesh_utils import _engine as get
    return get(engine)


def _split(rast):
    """nvdiffrast's (B,H,W,4) -> the dotdict Engine.interpolate reads"""
    r = rast.detach()
    return dotdict(uv=r[..., :2].contiguous(), zw=r[..., 2].contiguous(), face=(r[..., 3] - 1).to(torch.int32).contiguous())


class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, faces, H, W, engine, topology):
        out = engine.rasterize(pos, faces, H, W)
        rast = torch.cat([out.uv, out.zw[..., None], (out.face + 1).float()[..., None]], dim=-1)       # F < 2^24: a face id survives a float
        ctx.save_for_backward(pos.detach(), rast)
        ctx.engine, ctx.topology, ctx.faces, ctx.like = engine, topology, faces, (pos.shape, pos.dtype, pos.device)
        return rast

    @staticmethod
    def backward(ctx, g):
        pos, rast = ctx.saved_tensors
        topo = ctx.topology if ctx.topology is not None else ctx.engine.topology(ctx.faces, pos.shape[-2])
        shape, dtype, device = ctx.like
        d = ctx.engine.rasterize_backward(topo, pos, _split(rast), g[..., :2])      # zw and face carry no gradient
        return d.reshape(shape).to(device=device, dtype=dtype), None, None, None, None, None


class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attrs, rast, faces, engine, topology):
        out = engine.interpolate(attrs, _split(rast), faces)
        ctx.save_for_backward(attrs.detach(), rast.detach())
        ctx.engine, ctx.topology, ctx.faces = engine, topology, faces
        ctx.like = (attrs.shape, attrs.dtype, attrs.device, rast.dtype, rast.device)
        return out

    @staticmethod
    def backward(ctx, g):
        attrs, rast = ctx.saved_tensors
        topo = ctx.topology if ctx.topology is not None else ctx.engine.topology(ctx.faces, attrs.shape[-2])
        want = tuple(k for k, need in zip(('dattr', 'duv'), ctx.needs_input_grad[:2]) if need)
        a_shape, a_dtype, a_device, r_dtype, r_device = ctx.like
        d = ctx.engine.interpolate_backward(topo, attrs, _split(rast), g, want=want) if want else dotdict()
        dattr = d.dattr.reshape(a_shape).to(device=a_device, dtype=a_dtype) if 'dattr' in d else None
        drast = None
        if 'duv' in d:
            drast = torch.cat([d.duv, torch.zeros_like(d.duv)], dim=-1).to(device=r_device, dtype=r_dtype)
        return dattr, drast, None, None, None


class _Antialias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, rast, pos, faces, boost, engine, topology):
        topo = topology if topology is not None else engine.topology(faces, pos.shape[-2])
        out = engine.antialias(topo, color, _split(rast), pos)
        ctx.save_for_backward(color.detach(), rast.detach(), pos.detach())
        # a topology made here lives as long as the graph: the backward reuses it instead of building a second one
        ctx.engine, ctx.topology, ctx.boost = engine, topo, boost
        ctx.like = (color.dtype, color.device, pos.shape, pos.dtype, pos.device)
        return out.to(device=color.device)

    @staticmethod
    def backward(ctx, g):
        color, rast, pos = ctx.saved_tensors
        want = tuple(k for k, need in zip(('dcolor', 'dpos'), (ctx.needs_input_grad[0], ctx.needs_input_grad[2])) if need)
        c_dtype, c_device, p_shape, p_dtype, p_device = ctx.like
        d = ctx.engine.antialias_backward(ctx.topology, color, _split(rast), pos, g, pos_gradient_boost=ctx.boost, want=want) if want else dotdict()
        dcolor = d.dcolor.to(device=c_device, dtype=c_dtype) if 'dcolor' in d else None
        dpos = d.dpos.reshape(p_shape).to(device=p_device, dtype=p_dtype) if 'dpos' in d else None
        return dcolor, None, dpos, None, None, None, None


class _Texture(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv, uv_da, filter_mode, boundary_mode, max_mip_level, engine):
        out = engine.texture(tex, uv, uv_da, filter_mode, boundary_mode, max_mip_level)
        ctx.save_for_backward(tex.detach(), uv.detach(), None if uv_da is None else uv_da.detach())
        ctx.engine, ctx.modes = engine, (filter_mode, boundary_mode, max_mip_level)
        ctx.like = (tex.dtype, tex.device, uv.dtype, uv.device)
        return out.to(device=uv.device)

    @staticmethod
    def backward(ctx, g):
        tex, uv, uv_da = ctx.saved_tensors
        want = tuple(k for k, need in zip(('dtex', 'duv'), ctx.needs_input_grad[:2]) if need)
        t_dtype, t_device, u_dtype, u_device = ctx.like
        d = ctx.engine.texture_backward(tex, uv, g, uv_da, *ctx.modes, want=want) if want else dotdict()
        dtex = d.dtex.reshape(tex.shape).to(device=t_device, dtype=t_dtype) if 'dtex' in d else None
        duv = d.duv.to(device=u_device, dtype=u_dtype) if 'duv' in d else None
        return dtex, duv, None, None, None, None, None            # uv_da carries no gradient (first order: lod held fixed)


def rasterize(pos: torch.Tensor, faces: torch.Tensor, H: int, W: int, engine=None, topology=None) -> torch.Tensor:
    """pos (B,V,4) clip-space positions, faces (F,3) -> nvdiffrast's (B,H,W,4) float32 on the device: u, v, z/w, face + 1 (0 where the
    pixel is empty).  Differentiable in pos through u and v with the face map held fixed (first order); z/w and the face carry no
    gradient.  topology: Engine.topology(faces, V), which the backward needs — built there when not given (one read-back)."""
    if pos.ndim != 3 or pos.shape[-1] != 4:
        raise ValueError('rasterize: pos must be (B, V, 4); the range mode is not supported')
    return _Rasterize.apply(pos, faces, int(H), int(W), _engine(engine), topology)


def interpolate(attrs: torch.Tensor, rast: torch.Tensor, faces: torch.Tensor, rast_db=None, diff_attrs=None, engine=None, topology=None) -> torch.Tensor:
    """attrs (V,A) or (B,V,A), 1 <= A <= 64; rast: rasterize's output -> (B,H,W,A) float32, 0 where the pixel is empty.  Differentiable
    in attrs and in rast's u, v (first order).  rast_db / diff_attrs (pixel differentials) raise NotImplementedError here: interpolate_db
    takes them."""
    if rast_db is not None or diff_attrs is not None:
        raise NotImplementedError('interpolate: pixel differentials (rast_db, diff_attrs) are returned by interpolate_db, which has its own name '
                                  'because this call returns one tensor')
    return _Interpolate.apply(attrs, rast, faces, _engine(engine), topology)


def antialias(color: torch.Tensor, rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor, topology_hash=None, pos_gradient_boost: float = 1.0,
              engine=None, topology=None) -> torch.Tensor:
    """nvdiffrast's antialias, in its argument order: color (B,H,W,C), rast: rasterize's output, pos (B,V,4) the clip-space positions it was
    rasterised from, tri (F,3) -> (B,H,W,C) float32 with the silhouettes blended (module docstring).
    Differentiable in color and in pos (first order, the face map and the set of blended pixel pairs held fixed); pos_gradient_boost
    multiplies the gradient of pos only.  topology_hash is accepted and ignored; topology: Engine.topology(tri, V), which both passes
    need — built in the forward when not given (one read-back) and kept for the backward."""
    if pos.ndim != 3 or pos.shape[-1] != 4:
        raise ValueError('antialias: pos must be (B, V, 4); the range mode is not supported')
    return _Antialias.apply(color, rast, pos, tri, float(pos_gradient_boost), _engine(engine), topology)


def _to_clip(verts, R, T, K, H, W):
    """the reference's model-view-projection step: verts (B,V,3|4) float32 -> clip-space (B,V,4)"""
    if R is not None and T is not None:
        vverts = verts @ R.mT + T.mT
        homovverts = torch.cat([vverts, vverts.new_ones((*vverts.shape[:-1], 1))], dim=-1)
    elif verts.shape[-1] == 3:
        homovverts = torch.cat([verts, verts.new_ones((*verts.shape[:-1], 1))], dim=-1)
    else:
        homovverts = verts
    if K is None:
        K = get_ndc_perspective_matrix(torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, -2 * 0.001], [0, 0, 1, 0]], device=verts.device, dtype=verts.dtype), H, W)
    return homovverts @ K.mT


def rasterize_db(pos: torch.Tensor, faces: torch.Tensor, H: int, W: int, engine=None, topology=None):
    """`rasterize` with nvdiffrast's second output: -> (rast, rast_db).  rast has rasterize's bits and rasterize's backward; rast_db
    (B,H,W,4) = (du/dX, du/dY, dv/dX, dv/dY), the pixel differentials of the barycentrics, 0 where the pixel is empty, detached."""
    rast = rasterize(pos, faces, H, W, engine=engine, topology=topology)
    return rast, _engine(engine).raster_db(pos, faces, _split(rast))


def interpolate_db(attrs: torch.Tensor, rast: torch.Tensor, faces: torch.Tensor, rast_db: torch.Tensor, diff_attrs, engine=None, topology=None):
    """`interpolate` with pixel differentials: rast_db: rasterize_db's, diff_attrs: a list of channels of attrs or 'all' (at most 64)
    -> (out, out_da).  out has interpolate's bits and interpolate's backward; out_da (B,H,W,2n) = (da_0/dX, da_0/dY, da_1/dX, ...)
    in the order of diff_attrs, nvdiffrast's layout, detached."""
    channels = list(range(attrs.shape[-1])) if isinstance(diff_attrs, str) and diff_attrs == 'all' else [int(c) for c in diff_attrs]
    out = _Interpolate.apply(attrs, rast, faces, _engine(engine), topology)
    return out, _engine(engine).interpolate_da(attrs, _split(rast), faces, rast_db, channels)


def texture(tex: torch.Tensor, uv: torch.Tensor, uv_da: torch.Tensor = None, mip_level_bias=None, mip=None, filter_mode: str = 'auto',
            boundary_mode: str = 'wrap', max_mip_level: int = None, engine=None) -> torch.Tensor:
    """nvdiffrast's texture, in its argument order: tex (1,TH,TW,C) shared by the views or (B,TH,TW,C), row 0 at v = 0; uv (B,H,W,2);
    uv_da (B,H,W,4): interpolate_db's out_da of the two uv channels -> (B,H,W,C) float32 (module docstring).
    filter_mode 'auto' is 'linear-mipmap-linear' with uv_da and 'linear' without.  Differentiable in tex and uv, first order: the texel
    cells, the level pair and the level of detail are held fixed and uv_da carries no gradient.  mip_level_bias, mip, 'linear-mipmap-nearest'
    and the boundary modes 'zero' and 'cube' raise NotImplementedError."""
    if mip_level_bias is not None or mip is not None:
        raise NotImplementedError('texture: mip_level_bias and a prebuilt mip are not supported')
    if filter_mode == 'auto':
        filter_mode = 'linear-mipmap-linear' if uv_da is not None else 'linear'
    if filter_mode not in ('nearest', 'linear', 'linear-mipmap-linear'):
        raise NotImplementedError(f'texture: filter_mode {filter_mode!r} is not supported (nearest, linear, linear-mipmap-linear and auto are)')
    if boundary_mode not in ('wrap', 'clamp'):
        raise NotImplementedError(f'texture: boundary_mode {boundary_mode!r} is not supported (wrap and clamp are)')
    if tex.ndim != 4 or uv.ndim != 4:
        raise ValueError('texture: tex must be (1 or B, TH, TW, C) and uv (B, H, W, 2)')
    if filter_mode != 'linear-mipmap-linear':
        uv_da = None
    return _Texture.apply(tex, uv, uv_da, filter_mode, boundary_mode, max_mip_level, _engine(engine))


def render_nvdiffrast(verts: torch.Tensor, faces: torch.Tensor, attrs: torch.Tensor = None, uv: torch.Tensor = None, img: torch.Tensor = None,
                      H: int = 512, W: int = 512, R: torch.Tensor = None, T: torch.Tensor = None, K: torch.Tensor = None, R_S: int = 2,
                      pos_gradient_boost: float = 1.0, engine=None, topology=None, antialias: bool = False):
    """The reference's render_nvdiffrast, attribute path: verts (B,V,3|4) or (V,3) with R, faces (F,3), attrs (B,V,A) or (V,A), R (B,3,3),
    T (B,3,1), K (B,4,4) clip matrix (None: the reference's default) -> (rast_attrs (B,H,W,A), rast_msk (B,H,W)).  One mesh is expanded
    over the views of R; the maps are rasterised at R_S times the size and resized bilinearly.
    antialias=True is the REFERENCE'S behaviour: `antialias` (this module) is applied to cat([attributes, mask]) before the resize with
    pos_gradient_boost, so the mask is fractional along the outline and carries a gradient to verts.  The default False skips that step
    (the values this call returned before the op existed): the mask is soft through R_S alone, carries no gradient, and
    pos_gradient_boost is unused.  uv / img (the texture path) raise NotImplementedError here: render_textured takes them."""
    if uv is not None or img is not None:
        raise NotImplementedError('render_nvdiffrast: the texture path (uv, img) is render_textured, which has its own name because it returns '
                                  'the image as well')
    assert attrs is not None
    assert int(R_S) == R_S
    if verts.ndim == 2 and R is not None:
        verts = verts[None].expand(R.shape[0], *verts.shape)
    if attrs.ndim == 2 and R is not None:
        attrs = attrs[None].expand(R.shape[0], *attrs.shape)
    verts = verts.float().contiguous()
    attrs = attrs.float().contiguous()
    faces = faces.int().contiguous()
    A = attrs.shape[-1]
    ndcverts = _to_clip(verts, R, T, K, H, W)
    R_S = int(R_S)
    R_H, R_W = int(H * R_S), int(W * R_S)
    rast = rasterize(ndcverts, faces, R_H, R_W, engine=engine, topology=topology)
    rend_msk = rast[:, :, :, 3] != 0
    pattrs = interpolate(attrs, rast, faces, engine=engine, topology=topology)
    aa = torch.cat([pattrs, rend_msk.view(rast.shape[0], R_H, R_W, 1).to(pattrs.dtype)], dim=-1)
    if antialias:
        aa = _Antialias.apply(aa, rast, ndcverts, faces, float(pos_gradient_boost), _engine(engine), topology)
    aa = bilinear_interpolation(aa, [H, W])
    rast_attrs, rast_msk = aa.split([A, 1], dim=-1)
    return rast_attrs, rast_msk[..., 0]


def render_textured(verts: torch.Tensor, faces: torch.Tensor, attrs: torch.Tensor = None, uv: torch.Tensor = None, img: torch.Tensor = None,
                    H: int = 512, W: int = 512, R: torch.Tensor = None, T: torch.Tensor = None, K: torch.Tensor = None, R_S: int = 2,
                    pos_gradient_boost: float = 1.0, engine=None, topology=None, antialias: bool = False):
    """The reference's render_nvdiffrast, its two TEXTURE branches: uv (B,V,2) or (V,2) per-vertex texture coordinates, img (B,TH,TW,C)
    or (1,TH,TW,C) with the image's top row first (it is flipped, as the reference does, so that v = 0 is the bottom row); the other
    arguments as render_nvdiffrast -> (rast_attrs (B,H,W,A), rast_img (B,H,W,C), rast_msk (B,H,W)) with attrs, (rast_img, rast_msk)
    without.  The colour is `texture(img.flip(1), puv, puv_da, max_mip_level=8)` with puv_da the pixel differentials of uv, zeroed
    outside the mask, concatenated with the attributes and the mask, optionally antialiased (antialias=True is the reference's
    behaviour, the default False matches render_nvdiffrast here) and resized bilinearly.  The texture-only call works here; the
    reference's dies on attrs.ndim before it draws."""
    assert uv is not None and img is not None
    assert int(R_S) == R_S
    if verts.ndim == 2 and R is not None:
        verts = verts[None].expand(R.shape[0], *verts.shape)
    verts = verts.float().contiguous()
    B = verts.shape[0]
    if uv.ndim == 2:
        uv = uv[None].expand(B, *uv.shape)
    if attrs is not None and attrs.ndim == 2:
        attrs = attrs[None].expand(B, *attrs.shape)
    uv = uv.float().contiguous()
    faces = faces.int().contiguous()
    ndcverts = _to_clip(verts, R, T, K, H, W)
    R_S = int(R_S)
    R_H, R_W = int(H * R_S), int(W * R_S)
    rast, rast_db = rasterize_db(ndcverts, faces, R_H, R_W, engine=engine, topology=topology)
    rend_msk = rast[:, :, :, 3] != 0
    if attrs is not None:
        A = attrs.shape[-1]
        interp, puv_da = interpolate_db(torch.cat([attrs.float(), uv], dim=-1).contiguous(), rast, faces, rast_db, [A, A + 1], engine=engine, topology=topology)
        pattrs, puv = interp.split([A, 2], dim=-1)
    else:
        puv, puv_da = interpolate_db(uv, rast, faces, rast_db, [0, 1], engine=engine, topology=topology)
    # an empty pixel gets a NaN uv: texture returns 0 there — the reference zeroes the rgb outside the mask — and its backward spends
    # nothing on it (interpolate's 0 would send every empty pixel's taps to the texels around uv = (0, 0): one long run per texel)
    puv = torch.where(rend_msk[..., None], puv, torch.full_like(puv, float('nan')))
    prgb = texture(img.float().flip(1), puv.contiguous(), puv_da.contiguous(), max_mip_level=8, engine=engine)
    msk = rend_msk.view(B, R_H, R_W, 1).to(prgb.dtype)
    aa = torch.cat([pattrs, prgb, msk] if attrs is not None else [prgb, msk], dim=-1)
    if antialias:
        aa = _Antialias.apply(aa, rast, ndcverts, faces, float(pos_gradient_boost), _engine(engine), topology)
    aa = bilinear_interpolation(aa, [H, W])
    Cn = prgb.shape[-1]
    if attrs is not None:
        rast_attrs, rast_img, rast_msk = aa.split([A, Cn, 1], dim=-1)
        return rast_attrs, rast_img, rast_msk[..., 0]
    rast_img, rast_msk = aa.split([Cn, 1], dim=-1)
    return rast_img, rast_msk[..., 0]
